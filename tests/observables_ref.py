"""The statement of the trajectory observables (csrc/observables.hip), for tests/test_observables_host.py (CPU) and
tests/test_hip_observables.py (GPU).  Numpy only, no GPU.

The HISTOGRAM is restated in fp32 bit for bit on top of tests/graph_ref.py (pair_disp, cut2_of, fma32 are imported, not copied): r2 of
a pair i < j is graph_ref.pair_disp(pos_i, pos_j, cell)'s, the edges are thresholds on r2, edge2[k] = cut2_of(fl32(k r_max / n_bins))
with edge2[0] = 0, and a pair sits in bin k where edge2[k] <= r2 < edge2[k+1].  brute_force_histogram is the fp64 yardstick of that
statement: the true minimum image over a wide range of lattice translations and bins of the fp64 distance.

The CORRELATIONS are stated in fp64 from the fp32 inputs: exact products and sums up to fp64 rounding, next to A = sum |term|, the
scale of the device's fp32 rounding of every term.
"""
import numpy as np

from tests import graph_ref as G

f32, f64 = np.float32, np.float64


def bin_table(r_max, n_bins):
    """(r fp32 [n_bins + 1], edge2 fp32 [n_bins + 1])"""
    r = (np.arange(n_bins + 1, dtype=f64) * float(r_max) / n_bins).astype(f32)
    edge2 = np.array([f32(0)] + [G.cut2_of(x) for x in r[1:]], dtype=f32)
    return r, edge2


def n_pair_kinds(S):
    return S * (S + 1) // 2


def pair_kind_index(a, c, S):
    a, c = np.minimum(a, c), np.maximum(a, c)
    return a * S - a * (a - 1) // 2 + (c - a)


def pairs_of(mol_ptr, kind):
    """(i, j, system) of every unordered pair i < j of counted atoms of one system"""
    ii, jj, bb = [], [], []
    for b in range(len(mol_ptr) - 1):
        idx = np.arange(mol_ptr[b], mol_ptr[b + 1])
        idx = idx[kind[idx] >= 0]
        a, c = np.triu_indices(len(idx), k=1)
        ii.append(idx[a])
        jj.append(idx[c])
        bb.append(np.full(len(a), b))
    return np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64), np.concatenate(bb).astype(np.int64)


def histogram(pos, cell, mol_ptr, kind, S, r_max, n_bins, with_pairs=False):
    """counts int64 [B][P][n_bins] of the frames pos [F][N][3] under cell [B][3][3] or [F][B][3][3]: the fp32 statement.
    with_pairs: also (r2 fp32, bin (-1: not counted), tie) of the pairs of the LAST frame, in the order of pairs_of."""
    pos = np.asarray(pos, f32)
    pos = pos.reshape((-1,) + pos.shape[-2:])
    F, B = len(pos), len(mol_ptr) - 1
    cell = np.asarray(cell, f32).reshape(-1, B, 9)
    kind = np.asarray(kind)
    _, edge2 = bin_table(r_max, n_bins)
    counts = np.zeros((B, n_pair_kinds(S), n_bins), np.int64)
    ii, jj, bb = pairs_of(mol_ptr, kind)
    last = None
    for f in range(F):
        c = cell[f if len(cell) > 1 else 0]
        _, r2, tie = G.pair_disp(pos[f][ii], pos[f][jj], c[bb])
        k = np.searchsorted(edge2, r2, side='right') - 1          # edge2[k] <= r2 < edge2[k+1]
        ok = (k >= 0) & (k < n_bins)
        p = pair_kind_index(kind[ii], kind[jj], S)
        np.add.at(counts, (bb[ok], p[ok], k[ok]), 1)
        last = (r2, np.where(ok, k, -1), tie)
    return (counts, last) if with_pairs else counts


def brute_force_distances(pos, cell, ii, jj, images=3):
    """fp64 minimum-image distance of the pairs over the translations -images .. images of every lattice vector"""
    pos, cell = np.asarray(pos, f32).astype(f64), np.asarray(cell, f32).astype(f64).reshape(3, 3)
    d = pos[ii] - pos[jj]
    if not cell.any():
        return np.sqrt((d * d).sum(1))
    rng = np.arange(-images, images + 1)
    T = np.array([(a, b, c) for a in rng for b in rng for c in rng], f64) @ cell        # rows = lattice vectors
    best = np.full(len(d), np.inf)
    for t in T:
        e = d - t
        best = np.minimum(best, (e * e).sum(1))
    return np.sqrt(best)


def correlation(x, mol_ptr, kind, S, mode, max_lag, origin_every=1, weight=None):
    """(sums, A) fp64 [B][S][max_lag + 1]: sum over origins 0, origin_every, .. (t0 + l < F) and the atoms of (system, kind) of
    w x(t0) . x(t0 + l) (mode 0) or w |x(t0 + l) - x(t0)|^2 (mode 1), and the same sum of |term|."""
    x = np.asarray(x, f32).astype(f64)
    F, N = x.shape[:2]
    B = len(mol_ptr) - 1
    w = np.ones(N) if weight is None else np.asarray(weight, f32).astype(f64)
    sums, A = np.zeros((B, S, max_lag + 1)), np.zeros((B, S, max_lag + 1))
    batch = np.repeat(np.arange(B), np.diff(mol_ptr))
    kind = np.asarray(kind)
    ok = kind >= 0
    flat = (batch * S + np.clip(kind, 0, None))[ok]
    for lag in range(max_lag + 1):
        t0 = np.arange(0, F - lag, origin_every)
        a, c = x[t0], x[t0 + lag]
        term = (a * c).sum(2) if mode == 0 else ((c - a) ** 2).sum(2)
        term = term * w[None, :]
        sums[:, :, lag] = np.bincount(flat, weights=term.sum(0)[ok], minlength=B * S).reshape(B, S)
        A[:, :, lag] = np.bincount(flat, weights=np.abs(term).sum(0)[ok], minlength=B * S).reshape(B, S)
    return sums, A
