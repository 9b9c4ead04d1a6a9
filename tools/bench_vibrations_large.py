"""What spectra above the one-workgroup bound cost on one MI355X: the blocked eigensolver (csrc/eig_large.hip, solver='blocked')
on batches of synthetic molecules -- by default 256 blocks at M = 180 (60 atoms) and one block at M = 648 (216 atoms), random
symmetric, unit masses, projection on -- against the host alternative it replaces: the blocks copied to the host, then symmetrise
and numpy.linalg.eigh per molecule on at most 16 threads (without the projection: a lower bound).
The device side is timed with device events, median of --reps (20) after a warm-up, with and without modes, and includes the
derived quantities eig_blocks computes and its one read-back per sweep; the host side with the wall clock, median of 3.
Writes profiles/vibrations_large.json and prints one JSON line per workload.
usage: python tools/bench_vibrations_large.py [--reps 20] [--cases 60x256,216x1]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_vibrations import event_ms  # noqa: E402


def workload(n_atoms, n_mol, seed):
    g = torch.Generator().manual_seed(seed)
    M = 3 * n_atoms
    X = torch.randn(n_mol, M, M, generator=g)
    blocks = (X + X.transpose(1, 2)).reshape(-1).contiguous()
    ptr = torch.arange(n_mol, dtype=torch.long) * M * M
    batch = torch.arange(n_mol).repeat_interleave(n_atoms)
    pos = torch.randn(n_mol * n_atoms, 3, generator=g) * 3.0
    return blocks.cuda(), ptr.cuda(), batch.cuda(), pos.cuda(), torch.zeros(n_mol, 3, 3).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cases', default='60x256,216x1')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vibrations_large.json'))
    a = ap.parse_args()
    from newtonnet_amd import vibrations as vib
    threads = min(16, os.cpu_count() or 1)
    recs = []
    for k, case in enumerate(a.cases.split(',')):
        n_atoms, n_mol = (int(v) for v in case.split('x'))
        M = 3 * n_atoms
        blocks, ptr, batch, pos, cell = workload(n_atoms, n_mol, 100 + k)
        counts = torch.full((n_mol,), n_atoms, dtype=torch.long)

        def run(modes):
            return vib.eig_blocks(blocks, ptr, batch, pos, cell, None, modes=modes, counts=counts, solver='blocked')
        t_modes = event_ms(lambda: run(True), a.reps)
        t_evals = event_ms(lambda: run(False), a.reps)
        nm = run(True)
        sweeps = nm.sweeps.cpu().numpy()

        def host_once():
            t0 = time.perf_counter()
            h = blocks.cpu().numpy().reshape(n_mol, M, M).astype(np.float64)
            t1 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=threads) as ex:
                list(ex.map(lambda b: np.linalg.eigh(0.5 * (h[b] + h[b].T)), range(n_mol)))
            return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0)
        host_once()
        host_ms, copy_ms = sorted(host_once() for _ in range(3))[1]
        rec = dict(case=f'M{M}x{n_mol}', n_mol=n_mol, n_atoms=n_atoms, dim=M, solver='blocked',
                   eig_modes_ms=round(t_modes[0], 3), eig_modes_spread_ms=[round(t_modes[1], 3), round(t_modes[2], 3)],
                   eig_evals_only_ms=round(t_evals[0], 3), eig_evals_only_spread_ms=[round(t_evals[1], 3), round(t_evals[2], 3)],
                   host_copy_plus_eigh_ms=round(host_ms, 1), host_copy_ms=round(copy_ms, 1), host_threads=threads,
                   device_over_host=round(t_modes[0] / host_ms, 3), sweeps_min=int(sweeps.min()), sweeps_max=int(sweeps.max()),
                   n_projected=int(nm.n_projected[0]), status_any=int(nm.status.max()), reps=a.reps, host_reps=3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    with open(a.out, 'w') as fh:
        json.dump(recs, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
