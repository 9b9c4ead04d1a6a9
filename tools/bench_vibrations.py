"""What a batch of spectra costs on one MI355X, for 1024 aspirin conformers (the batch of tools/bench_hessian.py's aspirin1024):
  (a) hessian_blocks alone                                              (newtonnet_amd/hessian.py)
  (b) nnhip_eig_blocks alone on those blocks, with and without modes    (csrc/eig.hip; masses, projection on)
  (c) the host alternative the solver replaces: the blocks copied to the host, then symmetrise / mass-weight and
      numpy.linalg.eigh per molecule, on at most 16 threads (without the translation / rotation projection: a lower bound)
(a) and (b) are timed with device events over --hessian-reps / --reps repeats (20 each) after a warm-up, (b) including the
derived quantities eig_blocks computes (torch ops and one segmented sum); (c) with the wall clock, median of 3.  Prints one JSON line.
usage: python tools/bench_vibrations.py [--reps 20] [--mols 1024]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import util  # noqa: E402


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--hessian-reps', type=int, default=20)
    ap.add_argument('--mols', type=int, default=1024)
    a = ap.parse_args()
    from newtonnet_amd import hessian as nh
    from newtonnet_amd import vibrations as vib
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(util.load_state('ckpt', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    f = util.load_npz('aspirin_frames.npz')
    rng = np.random.default_rng(0)
    B = a.mols
    z = torch.as_tensor(f['z']).long().repeat(B).cuda()
    pos = torch.cat([torch.as_tensor(f['train_pos'][k % 8] + rng.normal(scale=0.02, size=(21, 3))).float() for k in range(B)]).cuda()
    batch = torch.arange(B).repeat_interleave(21).cuda()
    cell = torch.zeros(B, 3, 3).cuda()
    masses = vib.table_masses(z)
    with torch.no_grad():
        blocks, ptr, counts = nh.hessian_blocks_counts(model, z, pos, cell, batch)
        t_h = event_ms(lambda: nh.hessian_blocks(model, z, pos, cell, batch), a.hessian_reps)
        t_modes = event_ms(lambda: vib.eig_blocks(blocks, ptr, batch, pos, cell, masses, counts=counts), a.reps)
        t_evals = event_ms(lambda: vib.eig_blocks(blocks, ptr, batch, pos, cell, masses, modes=False, counts=counts), a.reps)
        nm = vib.eig_blocks(blocks, ptr, batch, pos, cell, masses, counts=counts)
    sweeps = nm.sweeps.cpu().numpy()

    rs = np.repeat(1.0 / np.sqrt(masses[:21].cpu().double().numpy()), 3)

    def host_once():
        t0 = time.perf_counter()
        h = blocks.cpu().numpy().reshape(B, 63, 63).astype(np.float64)
        t1 = time.perf_counter()

        def one(b):
            A = 0.5 * (h[b] + h[b].T) * rs[:, None] * rs[None, :]
            return np.linalg.eigh(A)
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            list(ex.map(one, range(B)))
        return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0)
    host_once()
    host = [host_once() for _ in range(3)]
    host_ms, copy_ms = sorted(host)[1]
    rec = dict(case=f'aspirin{B}', n_mol=B, n_atoms=21 * B, dim=63,
               hessian_blocks_ms=round(t_h[0], 3), eig_modes_ms=round(t_modes[0], 3), eig_modes_spread_ms=[round(t_modes[1], 3), round(t_modes[2], 3)],
               eig_evals_only_ms=round(t_evals[0], 3), eig_evals_only_spread_ms=[round(t_evals[1], 3), round(t_evals[2], 3)],
               eig_includes='one nnhip_eig_blocks launch + frequencies / zero-point energy / imaginary counts (torch ops, one segmented sum)',
               host_copy_plus_eigh_ms=round(host_ms, 1), host_copy_ms=round(copy_ms, 1), host_threads=min(16, os.cpu_count() or 1),
               eig_modes_fraction_of_hessian=round(t_modes[0] / t_h[0], 4), sweeps_min=int(sweeps.min()), sweeps_max=int(sweeps.max()),
               n_projected=int(nm.n_projected[0]), status_any=int(nm.status.max()), reps=a.reps, hessian_reps=a.hessian_reps, host_reps=3)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
