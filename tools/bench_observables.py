"""What the trajectory observables cost on one MI355X (csrc/observables.hip), on synthetic frames of the sizes users run:
  rdf_boxes     100 cubic boxes (13 A) x 216 atoms x 100 frames, r_max 6 A, 300 bins, 3 species
  rdf_aspirins  1024 molecules of 21 atoms x 100 frames, same bins
  vacf          1024 molecules of 21 atoms x 2000 frames x 500 lags
Timed with device events, medians of three, alternating in one run after a warm-up of every shape:
  the library's launch (RadialDistribution.add / velocity_autocorrelation on frames that are on the device),
  torch on the device, a loop over frames and systems (pairwise differences or cdist, bucketize, bincount: what a user writes today),
  torch on the device, all frames and systems of one size in one batched call (the fairest torch form; needs equal sizes),
  the velocity autocorrelation by torch.fft (Wiener-Khinchin, zero-padded) on the device,
and, wall clock and once, numpy on frames copied to the host (the copy included).  The torch and numpy histograms count all pairs into
one histogram; the library's per-pair-of-species counts are summed for the comparison and the number of differing counters is
reported (the torch forms bin sqrt(r2) in fp32, the library thresholds r2: pairs within an ulp of an edge may differ).
Reports, not thresholds.  Prints one JSON line and writes it to profiles/observables.json.
usage: python tools/bench_observables.py [--boxes 100] [--molecules 1024] [--rdf-frames 100] [--vacf-frames 2000] [--lags 500]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_MAX, N_BINS, BOX = 6.0, 300, 13.0
ASPIRIN_Z = [6] * 9 + [1] * 8 + [8] * 4


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median3(fns):
    """{name: (median ms, [ms, ms, ms])} of the callables, alternating, after one warm-up each"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            t[k].append(device_ms(fn))
    return {k: (round(float(np.median(v)), 3), [round(x, 3) for x in v]) for k, v in t.items()}


def frames_of(n_sys, n_per, n_frames, box, seed):
    """(z, batch, pos [F,N,3] on the device, cell [B,3,3]): a random start and a random walk of 0.05 A per frame (unwrapped)"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    N = n_sys * n_per
    start = torch.rand(N, 3, generator=g, device='cuda') * (box if box else 6.0)
    walk = torch.randn(n_frames, N, 3, generator=g, device='cuda').mul_(0.05).cumsum_(0)
    pos = (walk + start[None]).contiguous()
    z = torch.tensor(([8, 1, 1] * n_per)[:n_per] if box else ASPIRIN_Z, device='cuda').repeat(n_sys)
    batch = torch.arange(n_sys, device='cuda').repeat_interleave(n_per)
    cell = torch.eye(3, device='cuda').mul(box or 0.0).expand(n_sys, 3, 3).contiguous()
    return z, batch, pos, cell


def torch_loop(pos, n_sys, n_per, box, edges):
    """one histogram of all pairs per system: a loop over frames and systems on the device"""
    out = torch.zeros(n_sys, N_BINS, dtype=torch.int64, device=pos.device)
    iu = torch.triu_indices(n_per, n_per, 1, device=pos.device)
    for f in range(pos.shape[0]):
        for b in range(n_sys):
            x = pos[f, b * n_per:(b + 1) * n_per]
            if box:
                d = x[:, None, :] - x[None, :, :]
                d = d - box * torch.round(d / box)
                r = d.norm(dim=2)
            else:
                r = torch.cdist(x, x)
            k = torch.bucketize(r[iu[0], iu[1]], edges, right=True) - 1
            out[b] += torch.bincount(k[k < N_BINS], minlength=N_BINS)
    return out


def torch_batched(pos, n_sys, n_per, box, edges, chunk=10):
    """the same histograms with every frame and system of `chunk` frames in one call (systems of one size)"""
    out = torch.zeros(n_sys * N_BINS, dtype=torch.int64, device=pos.device)
    iu = torch.triu_indices(n_per, n_per, 1, device=pos.device)
    sys_off = (torch.arange(n_sys, device=pos.device) * N_BINS)[None, :, None]
    for f0 in range(0, pos.shape[0], chunk):
        x = pos[f0:f0 + chunk].reshape(-1, n_sys, n_per, 3)
        d = x[:, :, iu[0]] - x[:, :, iu[1]]
        if box:
            d = d - box * torch.round(d / box)
        k = torch.bucketize(d.norm(dim=3), edges, right=True) - 1
        flat = (k + sys_off)[k < N_BINS]
        out += torch.bincount(flat, minlength=n_sys * N_BINS)
    return out.view(n_sys, N_BINS)


def numpy_loop(pos, n_sys, n_per, box, edges):
    """(ms, histograms): frames copied to the host, a numpy loop over frames and systems"""
    t0 = time.perf_counter()
    x = pos.cpu().numpy()
    e = edges.cpu().numpy()
    out = np.zeros((n_sys, N_BINS), np.int64)
    iu = np.triu_indices(n_per, 1)
    for f in range(x.shape[0]):
        for b in range(n_sys):
            p = x[f, b * n_per:(b + 1) * n_per]
            d = p[iu[0]] - p[iu[1]]
            if box:
                d -= box * np.rint(d / box)
            out[b] += np.histogram(np.sqrt((d * d).sum(1)), bins=e)[0]
    return 1e3 * (time.perf_counter() - t0), out


def rdf_leg(n_sys, n_per, n_frames, box, seed):
    from newtonnet_amd import observables as ob
    z, batch, pos, cell = frames_of(n_sys, n_per, n_frames, box, seed)
    edges = torch.from_numpy(ob.bin_edges(R_MAX, N_BINS)[0]).cuda()
    rdf = ob.RadialDistribution(z, batch, R_MAX, N_BINS, cell=cell)
    keep = {}

    def library():
        rdf.counts.zero_()
        rdf.add(pos)

    def loop():
        keep['loop'] = torch_loop(pos, n_sys, n_per, box, edges)

    def batched():
        keep['batched'] = torch_batched(pos, n_sys, n_per, box, edges)

    t = median3(dict(library=library, torch_loop=loop, torch_batched=batched))
    ms_np, h_np = numpy_loop(pos, n_sys, n_per, box, edges)
    got = rdf.counts.sum(dim=1)
    rec = dict(systems=n_sys, atoms_per_system=n_per, frames=n_frames, r_max=R_MAX, bins=N_BINS, pair_kinds=len(rdf.pairs),
               pairs_counted=int(got.sum()), pairs_examined=n_sys * n_frames * n_per * (n_per - 1) // 2,
               library_ms=t['library'][0], torch_loop_ms=t['torch_loop'][0], torch_batched_ms=t['torch_batched'][0],
               library_all_ms=t['library'][1], torch_loop_all_ms=t['torch_loop'][1], torch_batched_all_ms=t['torch_batched'][1],
               numpy_on_copied_frames_ms=round(ms_np, 1),
               counters_differing_from_torch_loop=int((got != keep['loop']).sum()),
               counters_differing_from_torch_batched=int((got != keep['batched']).sum()),
               counters_differing_from_numpy=int((got.cpu().numpy() != h_np).sum()))
    return rec


def fft_vacf(vel, n_sys, n_per, lags, kind, n_kinds):
    """sum over atoms of a system and kind of the autocorrelation sums for lags 0 .. lags, by zero-padded FFT (all origins)"""
    F = vel.shape[0]
    n_fft = 1 << int(np.ceil(np.log2(2 * F)))
    out = torch.zeros(n_sys * n_kinds, lags + 1, dtype=torch.float64, device=vel.device)
    rows = (torch.arange(n_sys, device=vel.device).repeat_interleave(n_per) * n_kinds + kind.long())
    step = 4096                                   # atoms per call: the spectrum of a slice is [n_fft / 2 + 1, step, 3] complex
    for a0 in range(0, vel.shape[1], step):
        spec = torch.fft.rfft(vel[:, a0:a0 + step], n=n_fft, dim=0)
        c = torch.fft.irfft(spec.real ** 2 + spec.imag ** 2, n=n_fft, dim=0)[:lags + 1].sum(dim=2)       # [lags + 1, atoms]
        out.index_add_(0, rows[a0:a0 + step], c.t().double())
    return out.view(n_sys, n_kinds, lags + 1)


def vacf_leg(n_sys, n_per, n_frames, lags, seed):
    from newtonnet_amd import observables as ob
    g = torch.Generator(device='cuda').manual_seed(seed)
    vel = torch.randn(n_frames, n_sys * n_per, 3, generator=g, device='cuda')
    z = torch.tensor(ASPIRIN_Z, device='cuda').repeat(n_sys)
    batch = torch.arange(n_sys, device='cuda').repeat_interleave(n_per)
    acc = ob.VACF(z, batch, 1.0, lags)
    keep = {}

    def library():
        acc.sums.zero_()
        acc.n_origins.zero_()
        acc.add(vel)

    def fft():
        keep['fft'] = fft_vacf(vel, n_sys, n_per, lags, acc._kind, len(acc.species))

    t = median3(dict(library=library, torch_fft=fft))
    diff = (acc.sums - keep['fft']).abs().max().item()
    return dict(systems=n_sys, atoms_per_system=n_per, frames=n_frames, lags=lags, species=len(acc.species),
                terms=n_sys * n_per * sum(n_frames - l for l in range(lags + 1)),
                library_ms=t['library'][0], torch_fft_ms=t['torch_fft'][0], library_all_ms=t['library'][1],
                torch_fft_all_ms=t['torch_fft'][1], max_abs_difference_of_sums=diff, largest_sum=acc.sums.abs().max().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--boxes', type=int, default=100)
    ap.add_argument('--molecules', type=int, default=1024)
    ap.add_argument('--rdf-frames', type=int, default=100)
    ap.add_argument('--vacf-frames', type=int, default=2000)
    ap.add_argument('--lags', type=int, default=500)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_observables.py measures on an MI355X: no device found')
    rec = dict(rdf_boxes=rdf_leg(a.boxes, 216, a.rdf_frames, BOX, 1),
               rdf_aspirins=rdf_leg(a.molecules, 21, a.rdf_frames, 0.0, 2),
               vacf=vacf_leg(a.molecules, 21, a.vacf_frames, a.lags, 3),
               runs=3, device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'observables.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
