"""What the two forms of the L-BFGS launch cost on LARGE systems on one MI355X: form='wave' (one wave64 per system,
nnhip_lbfgs_step / nnhip_cell_lbfgs_step) against form='workgroup' (one workgroup of 1024 threads per system, the *_wg entry points).
Memory 16 with a FULL history, --steps steps (200) after --warmup (20), wall clock around a synchronised region; the legs alternate
inside one process and every figure is the median of three rounds.

  per step   Relaxation.run under both forms and a bare loop of model() calls (forces touched every step: the floor), on the
             4096-atom periodic system of tools/bench_relax.py (bench.synthetic_box) and on a box of 17 280 atoms (pbc216 tiled
             5 x 4 x 4, as tools/bench_npt.py); the same three legs for CellRelaxation (virial head) on the 4096-atom system.
             fmax = 1e-6 eV/A, so nothing converges inside the timed region; the history is filled by 20 real steps first.
  launches   the raw launch alone, without the model: n in --sizes atoms per system, B = 1 and 64 systems, both forms.  The
             forces are those of a separable quadratic well (stiffness log-uniform in 20 .. 2000 eV/A^2, started about 20 A away, so
             every step is clamped, every pair y = A s is accepted and nothing converges in 240 steps), formed by two torch
             element-wise ops per step; `force_ops_ms` is the time of those two ops alone, to be subtracted.
  wg_auto_min_atoms   the smallest n of the sweep from which on the workgroup launch is no slower than the wave launch at BOTH batch
             sizes -- what relax.WG_AUTO_MIN_ATOMS is set from.
Prints one JSON line and writes it to profiles/relax_large.json (--out).
usage: python tools/bench_relax_large.py [--steps 200] [--warmup 20] [--sizes 64,128,256,512,1024,2048,4096]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tests import util  # noqa: E402

MEMORY = 16
ROUNDS = 3


def timed(fn, steps, warmup):
    fn(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def medians(legs, steps, warmup):
    """legs: name -> fn(n).  The legs alternate; returns name -> median ms per step over ROUNDS rounds"""
    times = {name: [] for name in legs}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            times[name].append(timed(fn, steps, warmup))
    return {name: round(statistics.median(t), 4) for name, t in times.items()}


def make_model(props):
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=list(props))
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    return model


def one_tiled_box(reps=(5, 4, 4)):
    z, pos, cell, _, _ = util.case_inputs('pbc216_rand', torch.float32)
    shifts = torch.cartesian_prod(*[torch.arange(r, dtype=torch.float32) for r in reps])
    tiled = (pos[None, :, :] + (shifts @ cell[0])[:, None, :]).reshape(-1, 3)
    big = cell.clone()
    big[0] *= torch.tensor(reps, dtype=torch.float32)[:, None]
    n = tiled.shape[0]
    return z.repeat(shifts.shape[0]).cuda(), tiled.cuda(), big.cuda(), torch.zeros(n, dtype=torch.long).cuda()


def step_legs(model, inputs, steps, warmup, cell_too):
    z, pos, cell, batch = inputs
    make = model.cell_relaxation if cell_too else model.relaxation
    rels = {form: make(z, pos, cell, batch, fmax=1e-6, memory=MEMORY, form=form) for form in ('wave', 'workgroup')}
    for rel in rels.values():
        rel.run(MEMORY + 4, check_every=0)                  # fill the history

    def bare(n):
        for _ in range(n):
            out = model(z, pos, cell, batch)
            out.gradient_force
            if cell_too:
                out.virial
    legs = {form: (lambda n, rel=rel: rel.run(n, check_every=0)) for form, rel in rels.items()}
    legs['bare_model_loop'] = bare
    t = medians(legs, steps, warmup)
    rec = dict(n_atoms=int(pos.shape[0]), memory=MEMORY, driver='CellRelaxation' if cell_too else 'Relaxation',
               wave_ms=t['wave'], workgroup_ms=t['workgroup'], bare_model_loop_ms=t['bare_model_loop'],
               wave_launch_ms=round(t['wave'] - t['bare_model_loop'], 4),
               workgroup_launch_ms=round(t['workgroup'] - t['bare_model_loop'], 4))
    for form, rel in rels.items():
        rec[f'{form}_pairs'] = int(rel.n_pairs.min())
        res = rel.run(0)
        rec[f'{form}_frozen'] = int(res.converged.sum()) + (int(res.failed.sum()) if cell_too else 0)
    return rec


class RawLoop:
    """hip.lbfgs_step on B systems of n atoms in a separable quadratic well, two position buffers, nothing else"""

    def __init__(self, n, B, wg_min_atoms, seed=0):
        g = torch.Generator().manual_seed(seed)
        N = n * B
        f32 = dict(dtype=torch.float32, device='cuda')
        self.k = torch.exp(torch.empty(N, 3).uniform_(float(np.log(20.0)), float(np.log(2000.0)), generator=g)).cuda()
        self.x0 = torch.zeros(N, 3, **f32)
        self.x = [(torch.randn(N, 3, generator=g) * 20.0).cuda(), torch.empty(N, 3, **f32)]
        self.F, self.tmp = torch.empty(N, 3, **f32), torch.empty(N, 3, **f32)
        self.ptr = (torch.arange(B + 1, dtype=torch.int32) * n).cuda()
        self.ints = [torch.zeros(B, dtype=torch.int32, device='cuda') for _ in range(4)]
        self.S, self.Y = torch.zeros(MEMORY, N, 3, **f32), torch.zeros(MEMORY, N, 3, **f32)
        self.rho, self.f_prev = torch.zeros(B, MEMORY, **f32), torch.zeros(N, 3, **f32)
        self.work, self.fmax = torch.empty(N, 3, **f32), torch.zeros(B, **f32)
        self.cur, self.wg = 0, wg_min_atoms

    def forces(self):
        torch.sub(self.x0, self.x[self.cur], out=self.tmp)
        torch.mul(self.tmp, self.k, out=self.F)

    def run(self, steps):
        from newtonnet_amd import hip
        for _ in range(steps):
            self.forces()
            other = 1 - self.cur
            hip.lbfgs_step(self.x[self.cur], self.F, None, self.ptr, MEMORY, 1e-12, 70.0, 0.2, 0, *self.ints, self.S, self.Y, self.rho,
                           self.f_prev, self.work, self.x[other], self.fmax, wg_min_atoms=self.wg)
            self.cur = other

    def only_forces(self, steps):
        for _ in range(steps):
            self.forces()


def raw_launches(sizes, steps, warmup):
    rows = []
    for B in (1, 64):
        for n in sizes:
            loops = {'wave': RawLoop(n, B, None), 'workgroup': RawLoop(n, B, 0)}
            for loop in loops.values():
                loop.run(MEMORY + 4)
            legs = {form: loop.run for form, loop in loops.items()}
            legs['force_ops'] = loops['wave'].only_forces
            t = medians(legs, steps, warmup)
            rows.append(dict(n=n, B=B, wave_ms=t['wave'], workgroup_ms=t['workgroup'], force_ops_ms=t['force_ops'],
                             pairs=[int(loop.ints[2].min()) for loop in loops.values()],
                             converged=[int(loop.ints[0].sum()) for loop in loops.values()]))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def auto_threshold(rows, sizes):
    """the smallest n of the sweep from which on (every larger n too) the workgroup launch is no slower at every batch size"""
    ok = {n: all(r['workgroup_ms'] <= r['wave_ms'] for r in rows if r['n'] == n) for n in sizes}
    best = None
    for n in sorted(sizes, reverse=True):
        if not ok[n]:
            break
        best = n
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--sizes', default='64,128,256,512,1024,2048,4096')
    ap.add_argument('--skip-model', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(',')]
    rec = dict(steps=a.steps, warmup=a.warmup, rounds=ROUNDS, memory=MEMORY)
    rec['launches'] = raw_launches(sizes, a.steps, a.warmup)
    rec['wg_auto_min_atoms'] = auto_threshold(rec['launches'], sizes)
    if not a.skip_model:
        model = make_model(('energy', 'gradient_force'))
        rec['box_4096'] = step_legs(model, bench.synthetic_box(4096, 32, 0, 'cuda'), a.steps, a.warmup, False)
        rec['box_17280'] = step_legs(model, one_tiled_box(), a.steps, a.warmup, False)
        model = make_model(('energy', 'gradient_force', 'virial'))
        rec['cell_box_4096'] = step_legs(model, bench.synthetic_box(4096, 32, 0, 'cuda'), a.steps, a.warmup, True)
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'relax_large.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
