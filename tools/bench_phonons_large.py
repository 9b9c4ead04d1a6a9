"""What the blocked phonon solver (nnhip_phonon_bands_large, csrc/phonon_large.hip; solver='blocked') costs on one MI355X, on
synthetic force constants (random translation-invariant ones, tests/phonon_ref.random_crystal):
  (a) one 84-atom cell (d = 252, the aspirin cell) on a 2 x 2 x 2 supercell, 4^3 mesh        ->  64 problems
  (b) 8 such crystals on a band path of 64 q                                                 -> 512 problems
  (c) one cell at the bound (256 atoms, d = 768) on a 1 x 1 x 1 supercell at 8 q             ->   8 problems
each as ONE Phonons.frequencies call (the upload of q, the output and workspace allocations and the per-sweep read-back of the
done flags included), with and without modes, timed with device events, against the host loop tools/bench_phonons.py uses: Phi
and the image table copied to the host, then per q the complex128 D(q) (numpy, vectorised over the images) and
numpy.linalg.eigvalsh, wall clock.  Medians of three runs.  Prints one JSON line and writes it to profiles/phonons_large.json.
usage: python tools/bench_phonons_large.py [--skip-bound]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import phonon_ref as pr  # noqa: E402
from tools.bench_vibrations import event_ms  # noqa: E402


def crystals(n_cry, n_atoms, S):
    from newtonnet_amd import phonons as ph
    rng = np.random.default_rng(0)
    cell = 9.0 * np.eye(3) + 0.3 * rng.standard_normal((3, 3))
    cell = 0.5 * (cell + cell.T)
    base = pr.random_crystal(n_atoms, S, seed=1)[1]
    fcs, poss, masses = [], [], []
    for _ in range(n_cry):
        fcs.append((base * rng.uniform(0.5, 1.5)).astype(np.float32))
        poss.append(rng.uniform(0.0, 1.0, (n_atoms, 3)) @ cell)
        masses.append(rng.choice([1.008, 12.011, 15.999], n_atoms).astype(np.float32))
    return ph.Phonons.from_force_constants(fcs, np.ones(n_cry * n_atoms, dtype=np.int64), np.concatenate(poss), np.stack([cell] * n_cry), S,
                                           masses=np.concatenate(masses), batch=np.repeat(np.arange(n_cry), n_atoms), device='cuda',
                                           solver='blocked')


def host_loop(p, q):
    """the spectra of every crystal of p (all of one size) at q on the host, fp64: (ms in all, ms of the copies, eigenvalues [B][Q, d])"""
    t0 = time.perf_counter()
    fc = p.fc.cpu().numpy().astype(np.float64)
    start, off = p.img_start.cpu().numpy().astype(np.int64), p.img_off.cpu().numpy()
    m = p.masses.cpu().numpy().astype(np.float64)
    t1 = time.perf_counter()
    out = []
    n, N = p.counts[0], p.sc_counts[0]
    nR = N // n
    for b in range(len(p.counts)):
        f = np.ascontiguousarray(fc[b * 9 * n * N:(b + 1) * 9 * n * N].reshape(n, 3, nR, n, 3).transpose(0, 3, 1, 4, 2))   # [i, j, a, b, R]
        f = f.reshape(n, n, 9, nR)
        st = start[b * (n * N + 1):(b + 1) * (n * N + 1)]
        x = off[st[0]:st[-1]]
        cnt = np.diff(st).astype(np.float64)
        rs = 1.0 / np.sqrt(m[b * n:(b + 1) * n])
        ev = np.empty((len(q), 3 * n))
        for k, qq in enumerate(q):
            w = (np.add.reduceat(np.exp(2j * np.pi * (x @ qq)), st[:-1] - st[0]) / cnt).reshape(n, nR, n)
            D = np.matmul(f, w.transpose(0, 2, 1)[..., None]).reshape(n, n, 3, 3) * (rs[:, None] * rs[None, :])[:, :, None, None]
            D = D.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)
            ev[k] = np.linalg.eigvalsh(0.5 * (D + D.conj().T))
        out.append(ev)
    return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0), out


def leg(p, q, what):
    t = event_ms(lambda: p.frequencies(q), 3)
    t_modes = event_ms(lambda: p.frequencies(q, modes=True), 3)
    bands = p.frequencies(q)
    host_ms, copy_ms, ev = sorted((host_loop(p, q) for _ in range(3)), key=lambda r: r[0])[1]
    err = max(float(np.abs(bands.crystal(b)[0].cpu().double().numpy() - ev[b]).max()) for b in range(len(ev)))
    scale = max(float(np.abs(e).max()) for e in ev)
    rec = dict(case=what, crystals=len(p.counts), wave_vectors=len(q), problems=len(p.counts) * len(q), dim=3 * p.counts[0],
               supercell_atoms=p.sc_counts[0], solver_ms=round(t[0], 3), solver_spread_ms=[round(t[1], 3), round(t[2], 3)],
               solver_with_modes_ms=round(t_modes[0], 3), host_numpy_ms=round(host_ms, 1), host_copy_ms=round(copy_ms, 2),
               max_sweeps=int(bands.sweeps.max()), status=int(bands.status.abs().max()), max_abs_eigenvalue_difference=err,
               largest_eigenvalue=scale)
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def main():
    from newtonnet_amd import phonons as ph
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip-bound', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    path_q = ph.band_path([[0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0], [0, 0, 0]], 21)[0]
    rec = dict(mesh=leg(crystals(1, 84, (2, 2, 2)), ph.monkhorst_pack(4, 4, 4), 'one 84-atom cell, 4^3 mesh'),
               path=leg(crystals(8, 84, (2, 2, 2)), path_q, '8 84-atom cells, band path of 64 q'))
    if not a.skip_bound:
        n = ph.max_dim_large() // 3
        rec['bound'] = leg(crystals(1, n, (1, 1, 1)), np.random.default_rng(2).uniform(-0.5, 0.5, (8, 3)), f'one {n}-atom cell, 8 q')
    rec.update(runs=3, device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'phonons_large.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
