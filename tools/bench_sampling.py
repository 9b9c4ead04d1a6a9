"""What a batch of harmonic samples costs on one MI355X, for 1024 aspirin conformers x 32 samples each (the batch of
tools/bench_vibrations.py):
  (a) NormalModes.sample on the packed spectra of model.normal_modes: one nnhip_mode_sample launch (csrc/sample.hip) + the index
      arrays of the sample batch (torch ops), with the draws given and with torch.randn drawing them
  (b) the host alternative it replaces: modes and eigenvalues copied to the host, then per molecule sigma, q = sigma xi and
      dx = q L / sqrt(m) in numpy (fp64), on at most 16 threads; the draws are made beforehand and not timed
  (c) the same call with kernel='tiled' (csrc/sample_large.hip: two launches, the mode matrix streamed from HBM) on the same packed
      modes and draws, which must give the same bits
  (d) above the LDS bound: ONE synthetic molecule of --big-atoms atoms (512: the bound of the tiled kernel) x --big-samples samples
      (256) with kernel='tiled', against (b)'s host alternative for that molecule (copy of the 9.4 MB mode matrix included)
(a), (c) and (d) are timed with device events over --reps repeats (20) after a warm-up, the host legs with the wall clock, median of
3.  Prints one JSON line and writes it to profiles/sampling_aspirin<mols>.json.
usage: python tools/bench_sampling.py [--reps 20] [--mols 1024] [--samples 32] [--big-atoms 512] [--big-samples 256]"""
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
from tests import sample_ref as sr  # noqa: E402
from tests import util  # noqa: E402
from tools.bench_vibrations import event_ms  # noqa: E402


def big_molecule(n, S, T, reps):
    """leg (d): a seeded orthonormal mode matrix and sample_ref's synthetic spectrum for n atoms, as the NormalModes eig_blocks
    would return; the tiled kernel against numpy on the copied arrays"""
    from newtonnet_amd import vibrations as vib
    M = 3 * n
    rng = np.random.default_rng(1)
    modes = torch.from_numpy(np.ascontiguousarray(np.linalg.qr(rng.standard_normal((M, M)))[0].T).astype(np.float32)).cuda()
    evals = torch.from_numpy(sr.synthetic_spectrum(n)).cuda()
    masses = torch.from_numpy(rng.choice(np.array([1.008, 12.011, 15.999], dtype=np.float32), size=n)).cuda()
    pos = torch.from_numpy((1.5 * rng.standard_normal((n, 3))).astype(np.float32)).cuda()
    ptr, zeros = torch.tensor([0, M], device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    freq, thr, n_imag, zpe = vib.derived_quantities(evals, ptr, torch.zeros(n, dtype=torch.long, device='cuda'), 1)
    nm = vib.NormalModes(eigenvalues=evals, frequencies=freq, modes=modes.reshape(-1), ptr=ptr, blk_ptr=torch.zeros(1, dtype=torch.long, device='cuda'),
                         n_projected=zeros, sweeps=zeros, status=zeros, n_imaginary=n_imag, zero_point_energy=zpe, masses=masses,
                         threshold=thr, pos=pos, cell=torch.zeros(1, 3, 3, device='cuda'), z=None, _counts=[n], _offsets=[0],
                         _blk_offsets=[0])
    xi = torch.randn(S * M, device='cuda')
    t = event_ms(lambda: nm.sample(S, T, xi=xi, kernel='tiled'), reps)
    out = nm.sample(S, T, xi=xi, kernel='tiled')
    xi_h, p_h = xi.cpu().numpy().reshape(S, M).astype(np.float64), pos.cpu().numpy().reshape(M).astype(np.float64)
    rs = np.repeat(1.0 / np.sqrt(masses.cpu().double().numpy()), 3)
    kT = vib.K_BOLTZMANN * T

    def host_once():
        t0 = time.perf_counter()
        L = nm.modes.cpu().numpy().reshape(M, M).astype(np.float64)
        lam, th = nm.eigenvalues.cpu().numpy().astype(np.float64), float(nm.threshold.cpu()[0])
        t1 = time.perf_counter()
        live = lam > th
        sig = np.sqrt(np.where(live, kT / np.where(live, lam, 1.0), 0.0))
        res = p_h[None, :] + ((sig[None, :] * xi_h) @ L) * rs[None, :]
        return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0), res
    host_once()
    host_ms, copy_ms, res = sorted((host_once() for _ in range(3)), key=lambda r: r[0])[1]
    err = float(np.abs(res.reshape(S * n, 3) - out.pos.cpu().double().numpy()).max())
    n_tiles = (S + 31) // 32
    return dict(big_atoms=n, big_dim=M, big_samples=S, big_tiled_ms=round(t[0], 3), big_tiled_spread_ms=[round(t[1], 3), round(t[2], 3)],
                big_mode_matrix_bytes_read=n_tiles * 4 * M * M, big_flops=2 * S * M * M,
                big_host_copy_plus_numpy_ms=round(host_ms, 1), big_host_copy_ms=round(copy_ms, 1),
                big_max_abs_difference_to_host_fp64_A=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--mols', type=int, default=1024)
    ap.add_argument('--samples', type=int, default=32)
    ap.add_argument('--temperature', type=float, default=300.0)
    ap.add_argument('--big-atoms', type=int, default=512)
    ap.add_argument('--big-samples', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd import vibrations as vib
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(util.load_state('ckpt', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    f = util.load_npz('aspirin_frames.npz')
    rng = np.random.default_rng(0)
    B, S, T = a.mols, a.samples, a.temperature
    z = torch.as_tensor(f['z']).long().repeat(B).cuda()
    pos = torch.cat([torch.as_tensor(f['train_pos'][k % 8] + rng.normal(scale=0.02, size=(21, 3))).float() for k in range(B)]).cuda()
    batch = torch.arange(B).repeat_interleave(21).cuda()
    cell = torch.zeros(B, 3, 3).cuda()
    nm = model.normal_modes(z, pos, cell, batch)
    xi = torch.randn(B * S * 63, device='cuda')
    t_given = event_ms(lambda: nm.sample(S, T, xi=xi), a.reps)
    t_drawn = event_ms(lambda: nm.sample(S, T), a.reps)
    t_wigner = event_ms(lambda: nm.sample(S, T, quantum=True, xi=xi), a.reps)
    t_thermo = event_ms(lambda: nm.thermochemistry(T), a.reps)
    t_tiled = event_ms(lambda: nm.sample(S, T, xi=xi, kernel='tiled'), a.reps)
    t_given2 = event_ms(lambda: nm.sample(S, T, xi=xi), a.reps)           # the LDS kernel again, after the tiled one
    out = nm.sample(S, T, xi=xi)
    tiled = nm.sample(S, T, xi=xi, kernel='tiled')
    tiled_bitwise = all(torch.equal(getattr(out, k), getattr(tiled, k)) for k in ('pos', 'amplitudes', 'harmonic_energy',
                                                                                   'n_skipped_imaginary'))

    rs = np.repeat(1.0 / np.sqrt(nm.masses[:21].cpu().double().numpy()), 3)
    xi_h = xi.cpu().numpy().reshape(B, S, 63).astype(np.float64)
    p_h = pos.cpu().numpy().reshape(B, 63).astype(np.float64)
    kT = vib.K_BOLTZMANN * T
    threads = min(16, os.cpu_count() or 1)

    def host_once():
        t0 = time.perf_counter()
        L = nm.modes.cpu().numpy().reshape(B, 63, 63).astype(np.float64)
        lam = nm.eigenvalues.cpu().numpy().reshape(B, 63).astype(np.float64)
        thr = nm.threshold.cpu().numpy().astype(np.float64)
        t1 = time.perf_counter()

        def one(b):
            live = lam[b] > thr[b]
            sig = np.sqrt(np.where(live, kT / np.where(live, lam[b], 1.0), 0.0))
            return p_h[b][None, :] + ((sig[None, :] * xi_h[b]) @ L[b]) * rs[None, :]
        with ThreadPoolExecutor(max_workers=threads) as ex:
            res = list(ex.map(one, range(B)))
        return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0), res
    host_once()
    host = sorted((host_once() for _ in range(3)), key=lambda r: r[0])
    host_ms, copy_ms, res = host[1]
    err = float(np.abs(np.stack(res).reshape(B * S * 21, 3) - out.pos.cpu().double().numpy()).max())
    rec = dict(case=f'aspirin{B}', n_mol=B, n_samples=S, n_atoms=21 * B, dim=63, temperature=T,
               sample_ms=round(t_given[0], 3), sample_spread_ms=[round(t_given[1], 3), round(t_given[2], 3)],
               sample_with_randn_ms=round(t_drawn[0], 3), sample_wigner_ms=round(t_wigner[0], 3),
               thermochemistry_ms=round(t_thermo[0], 3),
               sample_tiled_ms=round(t_tiled[0], 3), sample_tiled_spread_ms=[round(t_tiled[1], 3), round(t_tiled[2], 3)],
               sample_lds_again_ms=round(t_given2[0], 3), tiled_bitwise_equal_to_lds=tiled_bitwise,
               sample_includes='one nnhip_mode_sample launch + the index arrays of the sample batch (z, batch, cell: torch ops)',
               host_copy_plus_numpy_ms=round(host_ms, 1), host_copy_ms=round(copy_ms, 1), host_threads=threads,
               max_abs_difference_to_host_fp64_A=err, n_skipped_imaginary_max=int(out.n_skipped_imaginary.max()),
               reps=a.reps, host_reps=3)
    if a.big_atoms > 0:
        rec.update(big_molecule(a.big_atoms, a.big_samples, T, a.reps))
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', f'sampling_aspirin{B}.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
