"""What a step of batched geometry relaxation costs on one MI355X: 1024 synthetic aspirins (bench.synthetic_aspirin) and one
aspirin, memory 16 with a FULL history, --steps steps (200) after --warmup (20), wall clock around a synchronised region (the
region and warm-up of tools/bench_md.py), ms per step of
  (a) Relaxation.run: model() + one nnhip_lbfgs_step launch per step (csrc/relax.hip), check_every = 0
  (b) a bare loop of model() calls on the same batch, forces touched every step -- the floor
and the launch's share (a - b) / b of the bare step.  The history is filled by 20 real steps before the warm-up; fmax is set so
low (1e-6 eV/A) that no molecule converges and freezes inside the timed region.
Also reported: the steps 1024 synthetic aspirins take to fmax = 0.01 eV/A (seeded weights: the surface is not a trained one, the
count is a statement about the batch machinery, check_every = 10), and the cost of ONE large periodic system (--box-atoms, a
bench.synthetic_box on a 32^3 lattice of 3.1 A spacing): one wave64 walks all of it, about 2 memory ceil(n / 64) dependent sweeps per step.
Prints one JSON line and writes it to profiles/relax_aspirin.json (--out).
usage: python tools/bench_relax.py [--steps 200] [--warmup 20] [--mols 1024] [--box-atoms 4096]"""
import argparse
import json
import os
import sys
import time

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


def legs(model, inputs, steps, warmup, memory=16):
    z, pos, cell, batch = inputs
    rel = model.relaxation(z, pos, cell, batch, fmax=1e-6, memory=memory)
    rel.run(memory + 4, check_every=0)                      # fill the history
    t_run = timed(lambda n: rel.run(n, check_every=0), steps, warmup)
    pairs = rel.n_pairs
    frozen = int((rel.run(0).converged).sum())

    def bare(n):
        for _ in range(n):
            model(z, pos, cell, batch).gradient_force
    t_bare = timed(bare, steps, warmup)
    return dict(n_mol=int(cell.shape[0]), n_atoms=int(pos.shape[0]), memory=memory, pairs_min=int(pairs.min()),
                pairs_max=int(pairs.max()), frozen_molecules=frozen, relaxation_run_ms=round(t_run, 4),
                bare_model_loop_ms=round(t_bare, 4), launch_share_of_bare_step=round((t_run - t_bare) / t_bare, 4))


def steps_to_converge(model, n_mol, max_steps=600):
    z, pos, cell, batch = bench.synthetic_aspirin(n_mol, 0, 'cuda')
    rel = model.relaxation(z, pos, cell, batch, fmax=0.01, memory=16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = rel.run(max_steps, check_every=10)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    n = res.n_steps.float()
    return dict(n_mol=n_mol, max_steps=max_steps, launches=rel.step_count, converged=int(res.converged.sum()),
                steps_min=int(n.min()), steps_median=float(n.median()), steps_max=int(n.max()), wall_s=round(wall, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--mols', type=int, default=1024)
    ap.add_argument('--box-atoms', type=int, default=4096)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    rec = dict(steps=a.steps, warmup=a.warmup,
               batch=legs(model, bench.synthetic_aspirin(a.mols, 0, 'cuda'), a.steps, a.warmup),
               single=legs(model, bench.synthetic_aspirin(1, 0, 'cuda'), a.steps, a.warmup))
    if a.box_atoms > 0:
        rec['one_large_periodic_system'] = legs(model, bench.synthetic_box(a.box_atoms, 32, 0, 'cuda'), max(a.steps // 4, 10),
                                                max(a.warmup // 4, 3))
    rec['to_fmax_0.01'] = steps_to_converge(model, a.mols)
    b = rec['batch']
    rec['us_per_molecule_step'] = round(1e3 * b['relaxation_run_ms'] / b['n_mol'], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'relax_aspirin.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
