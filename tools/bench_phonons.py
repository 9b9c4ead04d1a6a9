"""What the spectra of a phonon mesh cost on one MI355X, on synthetic force constants (random translation-invariant ones,
tests/phonon_ref.random_crystal: the kernel's work does not depend on where Phi came from):
  (a) one crystal of 8 atoms (d = 24) on a 3 x 3 x 3 supercell, 16^3 mesh  -> 4096 problems
  (b) 64 such crystals, 8^3 meshes                                         -> 32 768 problems
each as ONE Phonons.frequencies call (nnhip_phonon_bands, csrc/phonon.hip: the upload of q and the output allocations included),
timed with device events, against the host loop it replaces: Phi and the image table copied to the host, then per q the
complex128 D(q) (numpy, vectorised over the images) and numpy.linalg.eigvalsh, wall clock.  Medians of three runs.  Prints one
JSON line and writes it to profiles/phonons.json.
usage: python tools/bench_phonons.py [--crystals 64] [--mesh-one 16] [--mesh-many 8]"""
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

N_ATOMS, S = 8, (3, 3, 3)


def crystals(n_cry):
    from newtonnet_amd import phonons as ph
    rng = np.random.default_rng(0)
    cell = 4.0 * np.eye(3) + 0.2 * rng.standard_normal((3, 3))
    cell = 0.5 * (cell + cell.T)
    base = pr.random_crystal(N_ATOMS, S, seed=1)[1]
    fcs, poss, masses = [], [], []
    for _ in range(n_cry):
        fcs.append((base * rng.uniform(0.5, 1.5)).astype(np.float32))
        poss.append(rng.uniform(0.0, 1.0, (N_ATOMS, 3)) @ cell)
        masses.append(rng.choice([1.008, 12.011, 15.999], N_ATOMS).astype(np.float32))
    p = ph.Phonons.from_force_constants(fcs, np.ones(n_cry * N_ATOMS, dtype=np.int64), np.concatenate(poss), np.stack([cell] * n_cry), S,
                                        masses=np.concatenate(masses), batch=np.repeat(np.arange(n_cry), N_ATOMS), device='cuda')
    return p


def host_loop(p, q):
    """the spectra of every crystal of p at q on the host, fp64: (ms in all, ms of the copies, eigenvalues [B][Q, d])"""
    t0 = time.perf_counter()
    fc = p.fc.cpu().numpy().astype(np.float64)
    start, off = p.img_start.cpu().numpy().astype(np.int64), p.img_off.cpu().numpy()
    m = p.masses.cpu().numpy().astype(np.float64)
    t1 = time.perf_counter()
    out = []
    n, N, nR = N_ATOMS, N_ATOMS * 27, 27
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


def leg(p, mesh):
    from newtonnet_amd import phonons as ph
    q = ph.monkhorst_pack(mesh, mesh, mesh)
    t = event_ms(lambda: p.frequencies(q), 3)
    t_modes = event_ms(lambda: p.frequencies(q, modes=True), 3)
    bands = p.frequencies(q)
    host_ms, copy_ms, ev = sorted((host_loop(p, q) for _ in range(3)), key=lambda r: r[0])[1]
    err = max(float(np.abs(bands.crystal(b)[0].cpu().double().numpy() - ev[b]).max()) for b in range(len(ev)))
    scale = max(float(np.abs(e).max()) for e in ev)
    return dict(crystals=len(p.counts), mesh=mesh, problems=len(p.counts) * len(q), dim=3 * N_ATOMS, supercell_atoms=27 * N_ATOMS,
                kernel_ms=round(t[0], 3), kernel_spread_ms=[round(t[1], 3), round(t[2], 3)], kernel_with_modes_ms=round(t_modes[0], 3),
                host_numpy_ms=round(host_ms, 1), host_copy_ms=round(copy_ms, 2), max_sweeps=int(bands.sweeps.max()),
                max_abs_eigenvalue_difference=err, largest_eigenvalue=scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--crystals', type=int, default=64)
    ap.add_argument('--mesh-one', type=int, default=16)
    ap.add_argument('--mesh-many', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rec = dict(one=leg(crystals(1), a.mesh_one), many=leg(crystals(a.crystals), a.mesh_many), runs=3,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'phonons.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
