"""What a step of constant-pressure batched molecular dynamics costs on one MI355X: the periodic 216-atom box of the test fixtures
(tests/golden/case_pbc216_rand.npz) as --systems (100) independent systems (21 600 atoms, the scale of BASELINE configs[2]) and
tiled 5 x 4 x 4 into ONE system of 17 280 atoms (above the 16 384 atoms from which a single system runs in Morton order).  Langevin
at 100 K, 0.5 fs, --steps steps (200) after --warmup (20), wall clock around a synchronised region, the median of three fresh runs,
ms per step of
  npt  ConstantPressure.run: model() with the virial head + nnhip_npt_barostat + nnhip_npt_step per step (csrc/npt.hip)
  (a)  Dynamics.run with the same model, virial head included: what the two launches and the second cell buffer add
  (b)  Dynamics.run with a model without the virial head: what the head costs
  (c)  the model with the virial head + the barostat and the integrator written as torch ops on the device tensors
Prints one JSON line per size and writes profiles/npt_batch.json and profiles/npt_single.json (--out-dir).
usage: python tools/bench_npt.py [--steps 200] [--warmup 20] [--systems 100]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import util  # noqa: E402

KW = dict(temperature=100.0, friction=0.02, timestep=0.5)
NPT = dict(pressure=1.0, compressibility=4.5e-5, barostat_time=200.0)


def timed(make, steps, warmup, repeats=3):
    """median over `repeats` fresh runs of ms per step of run(steps) after run(warmup)"""
    out = []
    for _ in range(repeats):
        run = make()
        run(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return round(statistics.median(out), 4)


def make_model(props):
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=list(props))
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    return model


def batch_of_boxes(n_systems):
    z, pos, cell, _, _ = util.case_inputs('pbc216_rand', torch.float32)
    n = pos.shape[0]
    return (z.repeat(n_systems).cuda(), pos.repeat(n_systems, 1).cuda(), cell.repeat(n_systems, 1, 1).cuda(),
            torch.repeat_interleave(torch.arange(n_systems), n).cuda())


def one_tiled_box(reps=(5, 4, 4)):
    z, pos, cell, _, _ = util.case_inputs('pbc216_rand', torch.float32)
    shifts = torch.cartesian_prod(*[torch.arange(r, dtype=torch.float32) for r in reps])             # [T, 3]
    tiled = (pos[None, :, :] + (shifts @ cell[0])[:, None, :]).reshape(-1, 3)
    big = cell.clone()
    big[0] *= torch.tensor(reps, dtype=torch.float32)[:, None]
    n = tiled.shape[0]
    return z.repeat(shifts.shape[0]).cuda(), tiled.cuda(), big.cuda(), torch.zeros(n, dtype=torch.long).cuda()


def torch_ops_npt(model, z, pos, cell, batch):
    """the scheme of newtonnet_amd/npt.py with elementwise torch ops in the place of the two launches"""
    from newtonnet_amd import npt as npt_mod
    from newtonnet_amd.dynamics import FS, langevin_coefficients, maxwell_boltzmann
    from newtonnet_amd.vibrations import table_masses
    B = cell.shape[0]
    m = table_masses(z)
    a, p0, s2 = (t.cuda() for t in npt_mod.barostat_coefficients(KW['timestep'], NPT['barostat_time'], NPT['compressibility'],
                                                                   NPT['pressure'], KW['temperature'], B))
    c1, sigma = langevin_coefficients(KW['timestep'], KW['friction'], KW['temperature'], m, batch)
    hk, dth, sigma, half_m = (0.25 * FS / m)[:, None], 0.25 * FS, sigma[:, None], (0.5 * m)[:, None]
    out = model(z, pos, cell, batch)
    st = dict(x=pos.clone(), v=maxwell_boltzmann(m, batch, KW['temperature'], n_mol=B), c=cell.clone(), f=out.gradient_force,
              w=out.virial)

    def run(n):
        with torch.no_grad():
            x, v, c, f, w = st['x'], st['v'], st['c'], st['f'], st['w']
            for _ in range(n):
                v = v + hk * f
                K = torch.zeros(B, device=x.device).index_add_(0, batch, (half_m * v * v).sum(1))
                V = torch.linalg.det(c)
                P = (2.0 * K + w.diagonal(dim1=1, dim2=2).sum(1)) / (3.0 * V)
                mu = torch.exp((-a * (p0 - P) + torch.sqrt(s2 / V) * torch.randn(B, device=x.device)) / 3.0)
                v = v + hk * f
                x, v, c = mu[batch][:, None] * x, v / mu[batch][:, None], mu[:, None, None] * c
                x = x + dth * v
                v = c1 * v + sigma * torch.randn_like(v)
                x = x + dth * v
                o = model(z, x, c, batch)
                f, w = o.gradient_force, o.virial
            st.update(x=x, v=v, c=c, f=f, w=w)
    return run


def legs(name, inputs, steps, warmup):
    z, pos, cell, batch = inputs
    with_virial, plain = make_model(('energy', 'gradient_force', 'virial')), make_model(('energy', 'gradient_force'))

    def gen():
        return torch.Generator(device='cuda').manual_seed(0)
    rec = dict(case=name, n_systems=int(cell.shape[0]), n_atoms=int(pos.shape[0]), steps=steps, warmup=warmup, **KW, **NPT)
    rec['constant_pressure_run_ms'] = timed(lambda: with_virial.constant_pressure(z, pos, cell, batch, generator=gen(), **KW, **NPT).run,
                                            steps, warmup)
    rec['dynamics_run_with_virial_head_ms'] = timed(lambda: with_virial.dynamics(z, pos, cell, batch, generator=gen(), **KW).run, steps,
                                                    warmup)
    rec['dynamics_run_without_virial_head_ms'] = timed(lambda: plain.dynamics(z, pos, cell, batch, generator=gen(), **KW).run, steps,
                                                       warmup)
    rec['model_plus_torch_barostat_and_integrator_ms'] = timed(lambda: torch_ops_npt(with_virial, z, pos, cell, batch), steps, warmup)
    rec['two_launches_and_cell_buffers_add_ms'] = round(rec['constant_pressure_run_ms'] - rec['dynamics_run_with_virial_head_ms'], 4)
    rec['virial_head_adds_ms'] = round(rec['dynamics_run_with_virial_head_ms'] - rec['dynamics_run_without_virial_head_ms'], 4)
    rec['deferred_stats'] = with_virial.deferred_stats()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--systems', type=int, default=100)
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    for name, inputs in (('batch', batch_of_boxes(a.systems)), ('single', one_tiled_box())):
        line = json.dumps(legs(name, inputs, a.steps, a.warmup))
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f'npt_{name}.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
