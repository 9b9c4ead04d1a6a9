"""What a step of batched molecular dynamics costs on one MI355X: 1024 synthetic aspirins (bench.synthetic_aspirin) and one
aspirin, microcanonical, --steps steps (200) after --warmup (20), wall clock around a synchronised region, ms per step of
  (a) Dynamics.run: model() + one nnhip_md_step launch per step (csrc/md.hip)
  (b) a bare loop of model() calls on the same batch, forces touched every step -- what the package could do before, and the floor
  (c) model() + the same integrator written as torch ops on the device tensors (five elementwise launches per step)
and, for one aspirin, (d) the calculator's MD-loop path (MLAseCalculator.calculate, Verlet-skin list) driven by a host
velocity-Verlet loop in numpy: one structure per call, positions and forces through the host every step.
Prints one JSON line and writes it to profiles/md_aspirin.json (--out).
usage: python tools/bench_md.py [--steps 200] [--warmup 20] [--mols 1024]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tests import util  # noqa: E402


def timed(fn, steps, warmup):
    fn(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


class _Atoms:
    def __init__(self, numbers, positions):
        self.numbers, self.positions = numbers, positions

    def __len__(self):
        return len(self.numbers)

    def get_atomic_numbers(self):
        return self.numbers

    def get_positions(self, wrap=False):
        return self.positions

    def get_cell(self):
        return np.zeros((3, 3))

    def get_pbc(self):
        return np.zeros(3, dtype=bool)


def legs(model, n_mol, steps, warmup):
    from newtonnet_amd import dynamics as dyn_mod
    z, pos, cell, batch = bench.synthetic_aspirin(n_mol, 0, 'cuda')
    gen = torch.Generator(device='cuda').manual_seed(0)
    dyn = model.dynamics(z, pos, cell, batch, temperature=300.0, generator=gen)
    v0 = dyn.velocities
    t_run = timed(lambda n: dyn.run(n), steps, warmup)

    def bare(n):
        for _ in range(n):
            model(z, pos, cell, batch).gradient_force
    t_bare = timed(bare, steps, warmup)

    state = dict(x=pos.clone(), v=v0.clone(), f=model(z, pos, cell, batch).gradient_force)
    hk = (0.25 * dyn_mod.FS / dyn.masses)[:, None]
    dt = 0.5 * dyn_mod.FS

    def torch_ops(n):
        with torch.no_grad():
            x, v, f = state['x'], state['v'], state['f']
            for _ in range(n):
                v = v + hk * f
                x = x + dt * v
                f = model(z, x, cell, batch).gradient_force
                v = v + hk * f
            state.update(x=x, v=v, f=f)
    t_torch = timed(torch_ops, steps, warmup)
    return dict(n_mol=n_mol, n_atoms=int(pos.shape[0]), dynamics_run_ms=round(t_run, 4), bare_model_loop_ms=round(t_bare, 4),
                model_plus_torch_integrator_ms=round(t_torch, 4))


def calculator_leg(model, steps, warmup):
    from newtonnet_amd import dynamics as dyn_mod
    from newtonnet_amd.utils import MLAseCalculator
    from newtonnet_amd.vibrations import table_masses
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda', skin=0.5)
    z, pos, _, _ = bench.synthetic_aspirin(1, 0, 'cpu')
    m = table_masses(z).double().numpy()[:, None]
    dt = 0.5 * dyn_mod.FS
    st = dict(x=pos.double().numpy().copy(), v=np.zeros((21, 3)))
    calc.calculate(_Atoms(z.numpy(), st['x']))
    st['f'] = calc.results['forces'].astype(np.float64)

    def loop(n):
        x, v, f = st['x'], st['v'], st['f']
        for _ in range(n):
            v = v + 0.5 * dt * f / m
            x = x + dt * v
            calc.calculate(_Atoms(z.numpy(), x))
            f = calc.results['forces'].astype(np.float64)
            v = v + 0.5 * dt * f / m
        st.update(x=x, v=v, f=f)
    return round(timed(loop, steps, warmup), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--mols', type=int, default=1024)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    rec = dict(steps=a.steps, warmup=a.warmup, thermostat='none (velocity Verlet)', timestep_fs=0.5,
               batch=legs(model, a.mols, a.steps, a.warmup), single=legs(model, 1, a.steps, a.warmup))
    rec['single']['calculator_md_path_host_verlet_ms'] = calculator_leg(model, a.steps, a.warmup)
    b = rec['batch']
    rec['us_per_molecule_step'] = round(1e3 * b['dynamics_run_ms'] / b['n_mol'], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'md_aspirin.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
