"""What the strain slopes of a phonon mesh cost on one MI355X (nnhip_phonon_strain_slopes, csrc/phonon_gruneisen.hip), on the synthetic
crystals of tools/bench_phonons.py:
  (a) one crystal of 8 atoms (d = 24) on a 3 x 3 x 3 supercell, 16^3 mesh  -> 4096 problems
  (b) 64 such crystals, 8^3 meshes                                         -> 32 768 problems
with random planes of force-constant derivatives.  The eigenpairs come from one Phonons.frequencies(q, modes=True) call and stay on
the device; timed per shape, device events, medians of three, alternating in one run after a warm-up:
  the new launch alone with K = 1 plane and with K = 6 (outputs allocated before, the tolerances formed before),
  the velocity launch (nnhip_phonon_velocities) on the same problems and eigenpairs,
and, wall clock, a numpy loop on the host forming Re e^H dD e per q in complex128 from copied modes, K = 1, without the treatment of
degenerate groups.  Reports, not thresholds.  Prints one JSON line and writes it to profiles/gruneisen.json.
usage: python tools/bench_gruneisen.py [--crystals 64] [--mesh-one 16] [--mesh-many 8]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import bench_phonons  # noqa: E402
from tools.bench_phonon_velocities import device_ms  # noqa: E402


def host_loop(p, plane, q, bands):
    """Re e^H dD e of every mode of every crystal of p (all of one size) for one plane on the host, fp64: (ms, slopes [B][Q, d])"""
    t0 = time.perf_counter()
    fc = plane.cpu().numpy().astype(np.float64)
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
        cnt = np.diff(st).astype(np.float64)
        rs = 1.0 / np.sqrt(m[b * n:(b + 1) * n])
        dl = np.empty((len(q), 3 * n))
        for k, qq in enumerate(q):
            w = (np.add.reduceat(np.exp(2j * np.pi * (x @ qq)), st[:-1] - st[0]) / cnt).reshape(n, nR, n)
            G = np.matmul(f, w.transpose(0, 2, 1)[..., None]).reshape(n, n, 3, 3) * (rs[:, None] * rs[None, :])[:, :, None, None]
            G = G.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)
            G = 0.5 * (G + G.conj().T)
            E = modes[b][k]
            dl[k] = np.real(np.einsum('ki,ki->k', E.conj(), E @ G.T))
        out.append(dl)
    return 1e3 * (time.perf_counter() - t0), out


def leg(p, mesh):
    from newtonnet_amd import hip
    from newtonnet_amd import phonons as ph
    L, dev = hip.lib(), p.fc.device
    q = ph.monkhorst_pack(mesh, mesh, mesh)
    bands = p.frequencies(q, modes=True)
    B, Q, n_val = len(p.counts), len(q), 3 * sum(p.counts)
    evals, vec = bands.eigenvalues, torch.view_as_real(bands.modes)
    q_dev = torch.tensor(q, dtype=torch.float64).to(dev)
    scale = torch.stack([bands.crystal(b)[0].abs().max() for b in range(B)])
    tol = (torch.tensor([8.0 * ph.EPS32 * 2 * d for d in p._dims], dtype=torch.float32, device=dev) * scale).contiguous()
    dfc = torch.tensor(np.random.default_rng(4).standard_normal((6, p.fc.numel())).astype(np.float32)).to(dev)
    cells = torch.tensor(np.asarray(p._cells, dtype=np.float64).reshape(B, 3, 3)).to(dev).contiguous()
    out = {K: [torch.zeros(Q * n_val, K, dtype=torch.float32, device=dev) for _ in range(2)] for K in (1, 6)}
    vel, vdl = (torch.zeros(Q * n_val, 3, dtype=torch.float32, device=dev) for _ in range(2))
    group = torch.zeros(Q * n_val, dtype=torch.int32, device=dev)
    defined = torch.zeros(Q * n_val, dtype=torch.uint8, device=dev)
    status = torch.zeros(B, Q, dtype=torch.int32, device=dev)
    common = (hip._ptr(p.fc_ptr), hip._ptr(p.cry_ptr), p._cry_host.data_ptr(), hip._ptr(p.sc_atoms), hip._ptr(p.img_ptr),
              hip._ptr(p.img_start), hip._ptr(p.img_off), hip._ptr(p.masses), hip._ptr(p.out_ptr), B)

    def slopes(K):
        hip._check(L.nnhip_phonon_strain_slopes(hip._ptr(dfc), K, dfc.stride(0), hip._ptr(dfc), *common, hip._ptr(q_dev), Q, hip._ptr(evals),
                                                hip._ptr(vec), hip._ptr(tol), hip._ptr(tol), hip._ptr(out[K][0]), hip._ptr(out[K][1]),
                                                hip._ptr(group), hip._ptr(defined), hip._ptr(status), hip._stream(dev)),
                   'nnhip_phonon_strain_slopes')

    def velocities():
        hip._check(L.nnhip_phonon_velocities(hip._ptr(p.fc), *common, hip._ptr(cells), hip._ptr(q_dev), Q, None, hip._ptr(evals), hip._ptr(vec),
                                             hip._ptr(tol), hip._ptr(tol), hip._ptr(vel), hip._ptr(vdl), hip._ptr(group), hip._ptr(defined),
                                             hip._ptr(status), hip._stream(dev)), 'nnhip_phonon_velocities')

    for fn in (lambda: slopes(1), lambda: slopes(6), velocities):          # warm-up
        fn()
    torch.cuda.synchronize()
    t1, t6, tv = [], [], []
    for _ in range(3):          # alternating, in one run
        t1.append(device_ms(lambda: slopes(1)))
        t6.append(device_ms(lambda: slopes(6)))
        tv.append(device_ms(velocities))
    slopes(1)
    torch.cuda.synchronize()
    rec = dict(crystals=B, mesh=mesh, problems=B * Q, dim=3 * p.counts[0], supercell_atoms=p.sc_counts[0],
               slopes_k1_ms=round(float(np.median(t1)), 3), slopes_k6_ms=round(float(np.median(t6)), 3),
               velocity_launch_ms=round(float(np.median(tv)), 3), slopes_k1_all_ms=[round(t, 3) for t in t1],
               slopes_k6_all_ms=[round(t, 3) for t in t6], velocity_launch_all_ms=[round(t, 3) for t in tv],
               largest_status=int(status.max()))
    ms, dl = host_loop(p, dfc[0], q, bands)
    grp = group.cpu().numpy()
    got = out[1][0].cpu().double().numpy()[:, 0]
    err = 0.0
    for b in range(B):
        d, o = bands._dims[b], bands._offsets[b]
        g = grp[Q * o:Q * (o + d)].reshape(Q, d)
        single = (g == np.arange(d)[None, :]) & (np.concatenate([g[:, 1:], np.full((Q, 1), d)], axis=1) != g)
        err = max(err, float(np.abs(got[Q * o:Q * (o + d)].reshape(Q, d) - dl[b])[single].max()))
    rec.update(host_numpy_k1_ms=round(ms, 1), max_abs_slope_difference_of_single_modes=err, largest_slope=max(float(np.abs(x).max()) for x in dl))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--crystals', type=int, default=64)
    ap.add_argument('--mesh-one', type=int, default=16)
    ap.add_argument('--mesh-many', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    shapes = [('one', bench_phonons.crystals(1), a.mesh_one), ('many', bench_phonons.crystals(a.crystals), a.mesh_many)]
    rec = {name: leg(p, mesh) for name, p, mesh in shapes}
    rec.update(runs=3, device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'gruneisen.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
