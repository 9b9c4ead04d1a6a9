"""What phonon group velocities cost on one MI355X (nnhip_phonon_velocities, csrc/phonon_velocity.hip), on the synthetic crystals
of tools/bench_phonons.py and tools/bench_phonons_large.py:
  (a) one crystal of 8 atoms (d = 24) on a 3 x 3 x 3 supercell, 16^3 mesh            -> 4096 problems
  (b) 64 such crystals, 8^3 meshes                                                   -> 32 768 problems
  (c) one 84-atom cell (d = 252) on a 2 x 2 x 2 supercell, 4^3 mesh, solver='blocked' ->     64 problems
Three times per shape: Phonons.frequencies(q, modes=True) (the call as it was before the option existed), the same call with
velocities=True (its launch of nnhip_phonon_bands with modes plus the velocity launch and its allocations), and the host loop the
option replaces -- the modes, Phi and the image table copied to the host, then per q the three complex128 dD/dq_cart,a
(numpy, vectorised over the images) and Re e^H G_a e for every mode, without the treatment of degenerate groups, wall clock.
The two device calls alternate within one run after a warm-up of every shape; device events, medians of three.  Prints one
JSON line and writes it to profiles/phonon_velocities.json.
usage: python tools/bench_phonon_velocities.py [--crystals 64] [--mesh-one 16] [--mesh-many 8] [--mesh-large 4]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import bench_phonons, bench_phonons_large  # noqa: E402


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def host_loop(p, q, bands):
    """d lambda / d q_cart of every mode of every crystal of p (all of one size) on the host, fp64: (ms, gradients [B][Q, d, 3])"""
    t0 = time.perf_counter()
    fc = p.fc.cpu().numpy().astype(np.float64)
    start, off = p.img_start.cpu().numpy().astype(np.int64), p.img_off.cpu().numpy()
    m = p.masses.cpu().numpy().astype(np.float64)
    modes = [bands.crystal(b)[2].cpu().numpy().astype(np.complex128) for b in range(len(p.counts))]
    out = []
    n, N = p.counts[0], p.sc_counts[0]
    nR = N // n
    for b in range(len(p.counts)):
        f = np.ascontiguousarray(fc[b * 9 * n * N:(b + 1) * 9 * n * N].reshape(n, 3, nR, n, 3).transpose(0, 3, 1, 4, 2)).reshape(n, n, 9, nR)
        st = start[b * (n * N + 1):(b + 1) * (n * N + 1)]
        x = off[st[0]:st[-1]]
        r = x @ p._cells[b]
        cnt = np.diff(st).astype(np.float64)
        rs = 1.0 / np.sqrt(m[b * n:(b + 1) * n])
        dl = np.empty((len(q), 3 * n, 3))
        for k, qq in enumerate(q):
            ph = np.exp(2j * np.pi * (x @ qq))
            for a in range(3):
                w = (np.add.reduceat(1j * r[:, a] * ph, st[:-1] - st[0]) / cnt).reshape(n, nR, n)
                G = np.matmul(f, w.transpose(0, 2, 1)[..., None]).reshape(n, n, 3, 3) * (rs[:, None] * rs[None, :])[:, :, None, None]
                G = G.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)
                G = 0.5 * (G + G.conj().T)
                E = modes[b][k]
                dl[k, :, a] = np.real(np.einsum('ki,ki->k', E.conj(), E @ G.T))
        out.append(dl)
    return 1e3 * (time.perf_counter() - t0), out


def leg(p, mesh, host=True):
    from newtonnet_amd import phonons as ph
    q = ph.monkhorst_pack(mesh, mesh, mesh)
    plain, both = [], []
    for _ in range(3):          # alternating, in one run
        plain.append(device_ms(lambda: p.frequencies(q, modes=True)))
        both.append(device_ms(lambda: p.frequencies(q, velocities=True)))
    rec = dict(crystals=len(p.counts), mesh=mesh, problems=len(p.counts) * len(q), dim=3 * p.counts[0], supercell_atoms=p.sc_counts[0],
               bands_with_modes_ms=round(float(np.median(plain)), 3), with_velocities_ms=round(float(np.median(both)), 3),
               bands_with_modes_all_ms=[round(t, 3) for t in plain], with_velocities_all_ms=[round(t, 3) for t in both])
    rec['velocity_launch_ms'] = round(rec['with_velocities_ms'] - rec['bands_with_modes_ms'], 3)
    bands = p.frequencies(q, velocities=True, modes=True)
    rec['largest_status'] = int(bands.status.max())
    if host:
        ms, dl = host_loop(p, q, bands)
        Q = len(q)
        err = 0.0
        for b in range(len(p.counts)):
            d, o = bands._dims[b], bands._offsets[b]
            dev = bands.eigenvalue_gradients[Q * o:Q * (o + d)].view(Q, d, 3).cpu().double().numpy()
            grp = bands.degenerate_group[Q * o:Q * (o + d)].view(Q, d).cpu().numpy()
            single = (grp == np.arange(d)[None, :]) & (np.concatenate([grp[:, 1:], np.full((Q, 1), d)], axis=1) != grp)
            err = max(err, float(np.abs(dev - dl[b])[single].max()))
        rec.update(host_numpy_ms=round(ms, 1), max_abs_gradient_difference_of_single_modes=err,
                   largest_gradient=max(float(np.abs(x).max()) for x in dl))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--crystals', type=int, default=64)
    ap.add_argument('--mesh-one', type=int, default=16)
    ap.add_argument('--mesh-many', type=int, default=8)
    ap.add_argument('--mesh-large', type=int, default=4)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd import phonons as ph
    shapes = [('one', bench_phonons.crystals(1), a.mesh_one), ('many', bench_phonons.crystals(a.crystals), a.mesh_many),
              ('large', bench_phonons_large.crystals(1, 84, (2, 2, 2)), a.mesh_large)]
    for _, p, _ in shapes:          # warm-up of every shape: both calls, a small mesh
        q = ph.monkhorst_pack(2, 2, 2)
        p.frequencies(q, modes=True)
        p.frequencies(q, velocities=True)
    torch.cuda.synchronize()
    rec = {name: leg(p, mesh) for name, p, mesh in shapes}
    rec.update(runs=3, device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'phonon_velocities.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
