"""The statement of the neighbour-list builders and of the edge geometry (csrc/graph.hip), for tests/test_graph_ref_host.py (CPU) and
tests/test_hip_graph_stages.py (GPU).  Numpy only, no GPU.

The LIST is restated in fp32 bit for bit: pair_disp with every rounding written out (differences, the exact division of a diagonal
cell or the product with the fp32 image of the fp64 cofactor inverse of a general one, rint half-even, d - ((c0 n0 + c1 n1) + c2 n2),
r2 = fma(dz, dz, fma(dy, dy, dx dx))), the threshold cut2_of (the smallest float T with sqrt_rn(T) >= cutoff) next to the
reference's own predicate sqrt_rn(r2) < cutoff -- build_list asserts that the two agree on every candidate pair of every case --
and the receiver CSR with ascending senders.  rev / pid / pair_ptr come from tests/edge_ref.py: csr_arrays (no second copy).

fma32 is EXACT: the product of two fp32 numbers is exact in float64; the float64 sum s = p + c rounds once and two_sum gives its
error e exactly.  Rounding s to fp32 is the correctly rounded fma unless s lies exactly on an fp32 midpoint while e != 0 (RN64 is
monotone, so the true value p + c is on the same side of every fp32 midpoint as s, or s IS the midpoint): there the neighbour on
the side of e is taken.  (No input here comes near the overflow or subnormal range.)

General cells.  The device forms the inverse in fp64 code the compiler may contract, so the last bit of an fp32 inverse entry is not
pinned: each entry may move by one fp32 ulp.  That moves a fractional separation f = (inv0 dx + inv1 dy) + inv2 dz by at most
u_f = ulp(|inv0 dx| + |inv1 dy| + |inv2 dz|), and the image rint(f) -- hence the pair's displacement -- depends on that bit only
where f lies within 4 u_f of +-0.5 (mod 1).  `tie_share` counts those pairs; the GPU inputs are built so that there are none and
both test files assert it.

The EDGE GEOMETRY is stated in numpy.longdouble (64-bit significand on x86: a unit roundoff of 2^-64, 2^-12 of the fp64 terms
below; where longdouble is plain float64 the host test's mpmath comparison says so) with componentwise bounds; u = 2^-24,
eps = 2^-52:
  geo = (d / r, r)          u |ref| (1 + 2^-20): one rounding of an fp64 value whose own error is a few 2^-53.
  xg on a live edge         the interval index exact (inputs keep x FT_G 1e-9 from an integer, asserted); the fraction within
                            2^-24 + FT_G 2^-52 absolute.
  xg on a masked candidate  (FT_ZERO_ROW, 0) exactly; masked = the fp32 predicate fma(dz, dz, fma(dy, dy, dx dx)) >= cut2, NOT x >= 1.
  rbf = env(x) sin(w x) / x u |ref| (1 + 2^-20) + eps A_env |sin(w x) / x| + eps |env| (1 + w x) / x.
                            A_env is the magnitude of the terms the kernel's fp64 envelope cancels: p = 9:
                            1 + 55 x^9 + 99 x^10 + 45 x^11;  general p: 1 + 5 (a x^p + b x^(p+1) + c x^(p+2)) with the polynomial's
                            coefficients a, b, c (pow() and four products per term: five roundings);  cosine 0.5 (1 + cos(pi x)):
                            1 + (1 + pi x), the second part the rounding of the argument pi x and of the cosine.
                            The last term is the ARGUMENT of the sine: w x is rounded before the sine is taken (2^-53 w x) and the
                            sine itself is good to an ulp of 1: an absolute error of the sine that |sin| does not scale, which
                            matters only where sin(w x) is within 1e-7 of a zero.
  drbf = denv bes + env dbes, bes = sin(w x) / x, dbes = (w cos(w x) - bes) / x:
                            u |ref| (1 + 2^-20) + eps [ A_denv |bes| + |denv| (1 + w x) / x + A_env |dbes| + |env| E_d ],
                            E_d = (2 (|w cos| + |bes|) + (w + 1 / x) (1 + w x)) / x: the cancellation w cos - bes (the named one at
                            x -> 0) and the argument error in both the cosine and bes;  A_denv = 4 |denv| (p = 9), 6 |denv| (general
                            p), (pi / 2) (2 |sin(pi x)| + 1 + pi x) (cosine).
  masked rows of rbf / drbf are exactly zero.
The reference evaluates the polynomial envelope in a cancellation-free form, the regularised incomplete beta function
env_p(x) = sum_{k=3}^{p+2} C(p+2, k) (1-x)^k x^(p+2-k) (all terms positive; d/dx = -p(p+1)(p+2)/2 x^(p-1) (1-x)^2 as the
kernel's), and the cosine envelope as sin^2(pi (1-x) / 2), so the reference itself is not the limit near x -> 1.

The CELL LIST.  bin_coord32 / make_grid32 emulate csrc/graph.hip: bin_coord / make_grid in fp32.  margin_search takes, per axis,
the extreme floats on either side of every bin boundary and evaluates the 1-D pair predicate between atoms two bins apart: a pair
the predicate admits there is a pair the cell list loses.  Its result, and the analysis next to CELL_LIST_MAX_COORD below, give the
supported coordinate range that newtonnet_amd/hip.py enforces.
"""
import functools
from math import comb

import numpy as np

from tests import edge_ref as E

f32, f64, ld = np.float32, np.float64, np.longdouble
U = 2.0 ** -24
EPS = 2.0 ** -52
FT_G, FT_ZERO_ROW = E.FT_G, E.FT_ZERO_ROW
MOL_STAGE_MAX = E.MOL_STAGE_MAX
N_ELEMENTS = 119
MG_MAX_ATOMS, SG_MAX_ATOMS, MAX_NB, COSINE = 1024, 1024, 32, -1
CW_CAP, MG_LDS_EDGES, MG_SUM_MAX, SCAN_TILE = 256, 4096, 8192, 1024
BIN_FACTOR = f32(1.0001)
# newtonnet_amd/hip.py sends a box to the cell list only while every |coordinate| <= P = CELL_LIST_MAX_COORD cutoffs and every box
# length L <= 2 P.  Why 128.  A bin is W >= 1.0001 cutoff (1 - 2^-22) wide: a margin of 0.9999e-4 cutoff.  Take atoms i, j that
# bin_coord puts two bins apart.  s = fl(p fl(1/L)) is off by 2^-24 |p| / L (the product) and by the relative error of fl(1/L),
# which moves every boundary of one image alike (2^-24 |p_i - p_j| between two images); s - floor(s) is exact; fl(s nb) is off by
# 2^-24 nb.  In length: each of the two boundaries around the middle bin moves by at most 2^-24 (P + L), so the true separation
# (modulo L) is at least W - 2^-23 (P + L) - 2^-23 P.  The pair predicate is exact for two atoms of one image (the difference of
# two floats that close is exact and n = 0); across images fl(p_i - p_j) is off by 2^-24 2 P, fl(L n) by 2^-24 2 P and their
# difference is exact: 2^-22 P.  A pair is lost only if  2^-23 (P + L) + 2^-23 P + 2^-22 P = 2^-23 (4 P + L) <= 6 2^-23 P  reaches
# the margin: P >= 139 cutoffs.  128 is the power of two below (6 2^-23 128 = 0.916e-4).  margin_search finds the first lost pairs
# at |p| of about 2500 cutoffs: the analysis is the guarantee, the search shows it is not vacuous.
CELL_LIST_MAX_COORD = 128.0


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """a b + c rounded ONCE to fp32 (exact: see the module)"""
    p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
    c = np.broadcast_to(np.asarray(c, f32).astype(f64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(f32)
    r64 = r.astype(f64)
    other = np.where(r64 > s, np.nextafter(r, f32(-np.inf)), np.nextafter(r, f32(np.inf))).astype(f64)
    tie = (r64 != s) & (np.abs(r64 - s) == np.abs(other - s)) & (err != 0)
    hi, lo = np.maximum(r64, other), np.minimum(r64, other)
    return np.where(tie, np.where(err > 0, hi, lo), r64).astype(f32)


def cut2_of(cutoff):
    """the smallest float T with sqrt_rn(T) >= cutoff (numpy's fp32 sqrt is correctly rounded)"""
    cutoff = f32(cutoff)
    t = f32(cutoff * cutoff)
    while t > 0 and np.sqrt(t) >= cutoff:
        t = np.nextafter(t, f32(0))
    while np.sqrt(t) < cutoff:
        t = np.nextafter(t, f32(np.inf))
    return f32(t)


def cell_inverse32(cell):
    """fp32 image of the fp64 cofactor inverse of cell^T, [..., 9] as load_cell lays it out"""
    c = np.asarray(cell, f32).reshape(-1, 3, 3).astype(f64)
    a = np.transpose(c, (0, 2, 1)).reshape(-1, 9)
    c00 = a[:, 4] * a[:, 8] - a[:, 5] * a[:, 7]
    c01 = a[:, 5] * a[:, 6] - a[:, 3] * a[:, 8]
    c02 = a[:, 3] * a[:, 7] - a[:, 4] * a[:, 6]
    det = a[:, 0] * c00 + a[:, 1] * c01 + a[:, 2] * c02
    with np.errstate(divide='ignore', invalid='ignore'):
        idet = 1.0 / det
        inv = np.stack([c00 * idet, (a[:, 2] * a[:, 7] - a[:, 1] * a[:, 8]) * idet, (a[:, 1] * a[:, 5] - a[:, 2] * a[:, 4]) * idet,
                        c01 * idet, (a[:, 0] * a[:, 8] - a[:, 2] * a[:, 6]) * idet, (a[:, 2] * a[:, 3] - a[:, 0] * a[:, 5]) * idet,
                        c02 * idet, (a[:, 1] * a[:, 6] - a[:, 0] * a[:, 7]) * idet, (a[:, 0] * a[:, 4] - a[:, 1] * a[:, 3]) * idet], axis=1)
    return inv.astype(f32)


def cell_kind(cell):
    """0: no cell, 1: diagonal, 2: general -- per molecule, as load_cell decides"""
    c = np.asarray(cell, f32).reshape(-1, 9)
    any_ = (c != 0).any(axis=1)
    off = c[:, [1, 2, 3, 5, 6, 7]]
    diag = (off == 0).all(axis=1) & (c[:, [0, 4, 8]] != 0).all(axis=1)
    return np.where(~any_, 0, np.where(diag, 1, 2))


class Rules:
    """The choices of pair_disp a WRONG builder could make differently; the CPU test's mutations flip them one at a time."""
    strict = True           # r2 < cut2 (False: <=)
    fused = True            # r2 by the fma chain (False: (x^2 + y^2) + z^2)
    divide = True           # diagonal cell: d / L (False: d * fl(1 / L))
    half_even = True        # rint (False: round half away from zero)
    cut2_exact = True       # cut2_of (False: cutoff^2)


def _round(fr, rules):
    return np.rint(fr) if rules.half_even else (np.sign(fr) * np.floor(np.abs(fr) + f32(0.5))).astype(f32)


def pair_disp(pi, pj, cell, rules=Rules):
    """pi, pj [P][3] fp32, cell [P][9] fp32 (the receiver's molecule) -> (d [P][3], r2 [P], tie [P]): the displacement after the
    single-image shift, |d|^2, and whether the pair's image depends on the last bit of a general cell's inverse"""
    pi, pj, cell = np.asarray(pi, f32).reshape(-1, 3), np.asarray(pj, f32).reshape(-1, 3), np.asarray(cell, f32).reshape(-1, 9)
    d = pi - pj
    kind = cell_kind(cell)
    tie = np.zeros(len(d), bool)
    out = d.copy()
    k1 = np.flatnonzero(kind == 1)
    k2 = np.flatnonzero(kind == 2)
    for sel, general in ((k1, False), (k2, True)):
        if not sel.size:
            continue
        c, dd = cell[sel], d[sel]
        if general:
            inv = cell_inverse32(c)
            fr = np.stack([(inv[:, 3 * k] * dd[:, 0] + inv[:, 3 * k + 1] * dd[:, 1]) + inv[:, 3 * k + 2] * dd[:, 2] for k in range(3)], axis=1)
            mag = np.stack([np.abs(inv[:, 3 * k] * dd[:, 0]) + np.abs(inv[:, 3 * k + 1] * dd[:, 1]) + np.abs(inv[:, 3 * k + 2] * dd[:, 2])
                            for k in range(3)], axis=1)
            uf = np.spacing(np.maximum(mag, f32(1e-30)).astype(f32))
            half = np.abs(np.abs(fr - np.floor(fr)) - f32(0.5))
            tie[sel] = (half <= 4 * uf).any(axis=1)
        elif rules.divide:
            fr = dd / c[:, [0, 4, 8]]
        else:
            fr = dd * (f32(1) / c[:, [0, 4, 8]])
        n = _round(fr.astype(f32), rules)
        sh = np.stack([(c[:, 3 * k] * n[:, 0] + c[:, 3 * k + 1] * n[:, 1]) + c[:, 3 * k + 2] * n[:, 2] for k in range(3)], axis=1)
        out[sel] = dd - sh
    x, y, z = out[:, 0], out[:, 1], out[:, 2]
    r2 = fma32(z, z, fma32(y, y, x * x)) if rules.fused else ((x * x + y * y) + z * z).astype(f32)
    return out, r2, tie


def r2_of(d):
    d = np.asarray(d, f32).reshape(-1, 3)
    return fma32(d[:, 2], d[:, 2], fma32(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))


# ---------------------------------------------------------------------------------------------------------------------------
# the list
# ---------------------------------------------------------------------------------------------------------------------------
def mol_ptr_of(batch, n_mol):
    """mol_ptr [B+1] of a sorted batch vector, empty slots included (mol_ptr_kernel)"""
    return np.searchsorted(np.asarray(batch, np.int64), np.arange(n_mol + 1), side='left').astype(np.int32)


def status_bits(batch, n_mol, z=None, route='pairs'):
    """1: batch unsorted or outside [0, B); 2: z outside [0, 119); 8: a molecule above NNHIP_MOL_STAGE_MAX atoms; 16: a molecule
    above MG_MAX_ATOMS (the per-molecule route only; it comes with 8)"""
    batch = np.asarray(batch, np.int64)
    st = 0
    prev = np.concatenate([[-1], batch[:-1]])
    if ((batch < prev) | (batch < 0) | (batch >= n_mol)).any():
        st |= 1
    if z is not None and ((np.asarray(z) < 0) | (np.asarray(z) >= N_ELEMENTS)).any():
        st |= 2
    if not st & 1:
        sizes = np.diff(mol_ptr_of(batch, n_mol))
        if (sizes > MOL_STAGE_MAX).any():
            st |= 8
        if route == 'mol' and (sizes > MG_MAX_ATOMS).any():
            st |= 8 | 16
    return st


class List:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def candidates(mol_ptr, batch):
    """every ordered pair (i, j != i) of one molecule, (i, j) ascending"""
    n = len(batch)
    sizes = np.diff(mol_ptr)[batch]
    start = mol_ptr[:-1][batch].astype(np.int64)
    ii = np.repeat(np.arange(n, dtype=np.int64), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    jj = start[ii] + (np.arange(ii.size, dtype=np.int64) - np.repeat(first, sizes))
    keep = ii != jj
    return ii[keep], jj[keep]


def build_list(pos, cell, batch, cutoff, rules=Rules, order=None):
    """The neighbour list of a valid batch: mol_ptr, row_ptr, col, edge_index, disp, rev, pid, pair_ptr (tests/edge_ref.py:
    csr_arrays), cut2, tie_share.  order(i, js) -> a permutation of the row's positions (the CPU test's mutations only)."""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    cell = np.asarray(cell, f32).reshape(-1, 9)
    batch = np.asarray(batch, np.int64)
    B, N = len(cell), len(pos)
    cutoff = f32(cutoff)
    mol_ptr = mol_ptr_of(batch, B)
    cut2 = cut2_of(cutoff) if rules.cut2_exact else f32(cutoff * cutoff)
    ii, jj = candidates(mol_ptr, batch) if N else (np.zeros(0, np.int64),) * 2
    d, r2, tie = pair_disp(pos[ii], pos[jj], cell[batch[ii]], rules)
    hit = (r2 < cut2) if rules.strict else (r2 <= cut2)
    if rules is Rules:
        assert np.array_equal(hit, np.sqrt(r2) < cutoff), 'cut2_of and the predicate sqrt_rn(r2) < cutoff disagree'
    i, j, disp = ii[hit], jj[hit], d[hit]
    row_ptr, col, rev, pid, pair_ptr, edge_index = E.csr_arrays(N, list(zip(i.tolist(), j.tolist())))
    assert np.array_equal(edge_index[0], i) and np.array_equal(edge_index[1], j)
    out = List(N=N, B=B, E=int(col.size), cutoff=float(cutoff), cut2=cut2, mol_ptr=mol_ptr, row_ptr=row_ptr, col=col, rev=rev, pid=pid,
               pair_ptr=pair_ptr, edge_index=edge_index, disp=disp, tie_share=float(tie.mean()) if tie.size else 0.0,
               n_candidates=int(ii.size))
    if order is not None:
        for a in range(N):
            s, e = row_ptr[a], row_ptr[a + 1]
            perm = np.asarray(order(a, col[s:e].copy()), np.int64)
            out.col[s:e], out.disp[s:e] = col[s:e][perm], disp[s:e][perm]
            out.edge_index[1, s:e] = out.col[s:e]
    return out


def emptied_guard(row_ptr):
    """graph_guard_kernel's emptied graph: every row_ptr[k < N] = count, row_ptr[N] untouched, pair_ptr all zero"""
    n = len(row_ptr) - 1
    return np.full(n + 1, row_ptr[n], np.int32), np.zeros(n + 1, np.int32)


def emptied_small(n_atoms):
    """graph_small_kernel's: row_ptr and pair_ptr all zero (tail[0] still carries the true count)"""
    return np.zeros(n_atoms + 1, np.int32), np.zeros(n_atoms + 1, np.int32)


def disp_of_edges(pos, cell, batch, edge_index):
    """nnhip_edge_disp of a fixed candidate list"""
    i, j = np.asarray(edge_index[0], np.int64), np.asarray(edge_index[1], np.int64)
    d, r2, tie = pair_disp(np.asarray(pos, f32)[i], np.asarray(pos, f32)[j], np.asarray(cell, f32).reshape(-1, 9)[np.asarray(batch)[i]])
    return d, r2, tie


# ---------------------------------------------------------------------------------------------------------------------------
# edge geometry (longdouble) with bounds
# ---------------------------------------------------------------------------------------------------------------------------
def envelope(x, env):
    """(env, denv, A_env, A_denv) in longdouble; env: 9, another integer p >= 1, or COSINE"""
    x = np.asarray(x, ld)
    y = ld(1) - x
    if env == COSINE:
        pi = ld(np.pi) + ld(1.2246467991473532e-16)
        e = np.sin(pi * y / 2) ** 2
        de = -pi / 2 * np.sin(pi * x)
        A = 1 + (1 + np.pi * np.abs(x))
        Ad = (np.pi / 2) * (2 * np.abs(np.sin(pi * x)) + 1 + np.pi * np.abs(x))
        return e, de, A.astype(f64), Ad.astype(f64)
    p = int(env)
    e = sum(ld(comb(p + 2, k)) * y ** k * x ** (p + 2 - k) for k in range(3, p + 3))
    de = -ld(p * (p + 1) * (p + 2)) / 2 * x ** (p - 1) * y * y
    a, b, c = 0.5 * (p + 1) * (p + 2), p * (p + 2.0), 0.5 * p * (p + 1)
    xa = np.abs(x).astype(f64)
    mag = a * xa ** p + b * xa ** (p + 1) + c * xa ** (p + 2)
    if p == 9:
        return e, de, 1 + mag, 4 * np.abs(de).astype(f64)
    return e, de, 1 + 5 * mag, 6 * np.abs(de).astype(f64)


def edge_geometry(disp, cutoff, freq=None, env=9, cut2=None, mask_rule='fp32'):
    """{name: (ref, bound)} of geo [E][4], xg_index [E] (exact), xg_frac [E], rbf / drbf [E][nb] (when freq is given), and
    'masked' [E]: the candidates the fp32 predicate puts outside the cutoff (mask_rule 'fp64': x >= 1 instead -- the CPU test's
    mutation)."""
    d32 = np.asarray(disp, f32).reshape(-1, 3)
    cutoff = f32(cutoff)
    cut2 = cut2_of(cutoff) if cut2 is None else cut2
    d = d32.astype(ld)
    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    geo = np.concatenate([d / r[:, None], r[:, None]], axis=1)
    x = r / ld(cutoff)
    t = x * FT_G
    g0 = np.clip(np.floor(t), 0, FT_G - 1)
    near = np.abs(t - np.rint(t)).astype(f64)
    frac = t - g0
    masked = ~(r2_of(d32) < cut2) if mask_rule == 'fp32' else np.asarray(x >= 1)
    out = {'geo': (geo, U * np.abs(geo).astype(f64) * (1 + 2.0 ** -20)), 'masked': masked,
           'xg_index': np.where(masked, FT_ZERO_ROW, g0.astype(np.int64)).astype(np.int32),
           'xg_frac': (np.where(masked, 0, frac), np.where(masked, 0.0, 2.0 ** -24 + FT_G * 2.0 ** -52)),
           'grid_distance': np.where(masked, 1.0, near), 'x': x}
    if freq is None:
        return out
    w = np.asarray(freq, f32).astype(ld)[None, :]
    xx = x[:, None]
    e, de, A, Ad = envelope(xx, env)
    s, c = np.sin(w * xx), np.cos(w * xx)
    bes = s / xx
    dbes = (w * c - bes) / xx
    rbf = e * bes
    drbf = de * bes + e * dbes
    a = lambda v: np.abs(v).astype(f64)            # noqa: E731
    w64, x64 = w.astype(f64), xx.astype(f64)
    arg = (1 + w64 * x64) / x64
    Brbf = U * a(rbf) * (1 + 2.0 ** -20) + EPS * (A * a(bes) + a(e) * arg)
    Ed = (2 * (a(w * c) + a(bes)) + (w64 + 1 / x64) * (1 + w64 * x64)) / x64
    Bdrbf = U * a(drbf) * (1 + 2.0 ** -20) + EPS * (Ad * a(bes) + a(de) * arg + A * a(dbes) + a(e) * Ed)
    m = masked[:, None]
    out['rbf'] = (np.where(m, 0, rbf), np.where(m, 0.0, Brbf))
    out['drbf'] = (np.where(m, 0, drbf), np.where(m, 0.0, Bdrbf))
    out['fp64_term'] = {'rbf': EPS * (A * a(bes) + a(e) * arg), 'drbf': EPS * (Ad * a(bes) + a(de) * arg + A * a(dbes) + a(e) * Ed)}
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the cell list's grid in fp32
# ---------------------------------------------------------------------------------------------------------------------------
def make_grid32(box, cutoff, factor=BIN_FACTOR):
    """(nb [3], inv_len [3]) or None where make_grid refuses the box"""
    box = np.asarray(box, f32).reshape(3)
    if not (box > 0).all():
        return None
    width = f32(f32(cutoff) * f32(factor))
    nb = np.floor((box / width).astype(f32)).astype(np.int64)
    if (nb < 3).any():
        return None
    return np.minimum(nb, 1024), (f32(1) / box).astype(f32)


def bin_coord32(p, inv_len, nb):
    p = np.asarray(p, f32)
    s = (p * f32(inv_len)).astype(f32)
    s = (s - np.floor(s)).astype(f32)
    b = (s * f32(nb)).astype(f32).astype(np.int64)
    return np.clip(b, 0, nb - 1)


def eligible(box, cutoff, pos=None):
    """newtonnet_amd/hip.py's test for the cell list: make_grid accepts the box, every length <= 2 CELL_LIST_MAX_COORD cutoffs, every
    |coordinate| <= CELL_LIST_MAX_COORD cutoffs"""
    box = np.asarray(box, f32).reshape(3)
    if make_grid32(box, cutoff) is None or not (box <= f32(2 * CELL_LIST_MAX_COORD * float(cutoff))).all():
        return False
    return pos is None or bool(np.abs(np.asarray(pos, f32)).max(initial=0) <= f32(CELL_LIST_MAX_COORD * float(cutoff)))


def pred1d(pi, pj, L, cutoff):
    """the pair predicate for two atoms on one axis of a diagonal cell: (admitted, |d|)"""
    z = np.zeros_like(np.asarray(pi, f32))
    cell = np.zeros((z.size, 9), f32)
    cell[:, 0] = cell[:, 4] = cell[:, 8] = f32(L)
    d, r2, _ = pair_disp(np.stack([pi, z, z], 1), np.stack([np.asarray(pj, f32), z, z], 1), cell)
    return r2 < cut2_of(cutoff), np.abs(d[:, 0])


def _around(p, n):
    """the 2 n + 1 floats around p"""
    p = f32(p)
    out, lo, hi = [p], p, p
    for _ in range(n):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        out += [lo, hi]
    return np.sort(np.array(out, f32))


def margin_search(L, cutoff, offsets_i, offsets_j=None, ulps=40, factor=BIN_FACTOR, boundaries=None, with_pair=False):
    """Per bin boundary m of the box [0, L) displaced by offsets_i whole box lengths: the floats within `ulps` of the boundaries m and
    m + 1 (the latter displaced by offsets_j box lengths, default the same), every pair (i below m, j at or above m + 1) that the
    grid puts two or more bins apart, and the 1-D predicate on it.
    Returns (smallest |d| two bins apart, the admitted pairs [(p_i, p_j)] = the pairs a cell list would lose)."""
    L = f32(L)
    grid = make_grid32([L, L, L], cutoff, factor)
    assert grid is not None
    nb, inv = int(grid[0][0]), grid[1][0]
    offsets_j = offsets_i if offsets_j is None else offsets_j
    best, lost, pair = np.inf, [], None
    ms = range(nb) if boundaries is None else boundaries
    for ki, kj in zip(offsets_i, offsets_j):
        for m in ms:
            pi = _around(f32(ki * float(L) + m * float(L) / nb), ulps)
            pj = _around(f32(kj * float(L) + (m + 1) * float(L) / nb), ulps)
            bi, bj = bin_coord32(pi, inv, nb), bin_coord32(pj, inv, nb)
            a, b = np.meshgrid(np.arange(pi.size), np.arange(pj.size), indexing='ij')
            gap = (bj[b] - bi[a]) % nb
            far = (gap >= 2) & (gap <= nb - 2)
            if not far.any():
                continue
            ok, dist = pred1d(pi[a[far]], pj[b[far]], L, cutoff)
            if float(dist.min()) < best:
                q = int(dist.argmin())
                best, pair = float(dist.min()), (pi[a[far]][q], pj[b[far]][q])
            for q in np.flatnonzero(ok):
                lost.append((float(pi[a[far]][q]), float(pj[b[far]][q])))
    return (best, lost, pair) if with_pair else (best, lost)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: the cases of tests/test_hip_graph_stages.py (the CPU tests run the statement and its mutations on the same ones)
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """pos [N][3] fp32, cell [B][9] fp32, batch [N] int64 (sorted), cutoff, z [N] int64"""

    def __init__(self, name, pos, cell, batch, cutoff, z=None):
        self.name, self.pos, self.cutoff = name, np.ascontiguousarray(pos, f32).reshape(-1, 3), float(f32(cutoff))
        self.cell = np.ascontiguousarray(cell, f32).reshape(-1, 9)
        self.batch = np.ascontiguousarray(batch, np.int64)
        self.N, self.B = len(self.pos), len(self.cell)
        self.z = np.ones(self.N, np.int64) if z is None else np.ascontiguousarray(z, np.int64)
        self._list = None

    @property
    def list(self):
        """the statement's list, computed once and shared (treat as read-only)"""
        if self._list is None:
            self._list = build_list(self.pos, self.cell, self.batch, self.cutoff)
        return self._list


def _batch_of(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


def diag_cell(lx, ly, lz):
    c = np.zeros(9, f32)
    c[0], c[4], c[8] = lx, ly, lz
    return c


SHEARED = np.array([11.0, 0.0, 0.0, 2.5, 12.0, 0.0, -1.5, 3.0, 13.0], f32)


def on_threshold(cutoff, seed=0):
    """three vectors [3][3] with r2 = the float below cut2, cut2 itself, the float above -- constructed, not in the xy plane only"""
    rng = np.random.default_rng(seed)
    c2 = cut2_of(cutoff)
    want = [np.nextafter(c2, f32(0)), c2, np.nextafter(c2, f32(np.inf))]
    out = []
    for target in want:
        while True:
            v = rng.standard_normal(3)
            v = (v / np.linalg.norm(v) * np.sqrt(float(target))).astype(f32)
            found = False
            for _ in range(64):
                r2 = r2_of(v)[0]
                if r2 == target:
                    found = True
                    break
                k = int(np.argmax(np.abs(v)))
                v[k] = np.nextafter(v[k], f32(0) if r2 > target else f32(np.sign(v[k]) * np.inf))
            if found:
                out.append(v.copy())
                break
    return np.array(out, f32)


def case_sizes():
    """molecule sizes 1, 2, 63, 64, 65, 128, 129 with empty slots first, in the middle and last; diagonal, sheared and zero cells in
    one batch; cutoff 5"""
    sizes = [0, 1, 2, 63, 0, 0, 64, 65, 128, 129, 0]
    rng = np.random.default_rng(101)
    cells = [np.zeros(9, f32), np.zeros(9, f32), diag_cell(11, 12.5, 14), SHEARED, np.zeros(9, f32), SHEARED, np.zeros(9, f32),
             diag_cell(12, 12, 12), SHEARED, diag_cell(16, 11, 13), diag_cell(11, 11, 11)]
    pos = np.concatenate([rng.random((n, 3)) * 11.0 + rng.integers(-2, 3, (1, 3)) * 12.0 for n in sizes])
    return Case('sizes', pos, np.array(cells), _batch_of(sizes), 5.0, z=rng.integers(0, N_ELEMENTS, sum(sizes)))


def _ball(rng, n, diameter):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * (0.5 * diameter * rng.random((n, 1)) ** (1 / 3))


def case_full(sizes=(65, 66), cutoff=6.3, name='full'):
    """an isolated first atom, fully connected molecules (degree size - 1), a two-atom molecule whose atoms do not see each other:
    the last atom is isolated"""
    rng = np.random.default_rng(7 + sum(sizes))
    parts, all_sizes = [np.zeros((1, 3))], [1]
    for n in sizes:
        parts.append(_ball(rng, n, 0.9 * cutoff) + rng.standard_normal((1, 3)) * 3)
        all_sizes.append(n)
    parts.append(np.array([[0.0, 0, 0], [3.0 * cutoff, 0, 0]]))
    all_sizes.append(2)
    c = Case(name, np.concatenate(parts), np.zeros((len(all_sizes), 9), f32), _batch_of(all_sizes), cutoff)
    deg = np.diff(c.list.row_ptr)
    assert deg[0] == 0 and deg[-1] == 0 and all((deg[_batch_of(all_sizes) == k + 1] == n - 1).all() for k, n in enumerate(sizes))
    return c


def case_chain(n, cutoff=1.0, cell=None):
    """n atoms on a gently bent line, 0.9 cutoff apart: every inner atom sees its two neighbours"""
    t = np.arange(n) * 0.9 * cutoff
    pos = np.stack([t, 0.01 * np.sin(t), 0.02 * np.cos(0.3 * t)], axis=1)
    return Case(f'chain{n}', pos, np.zeros((1, 9), f32) if cell is None else cell, np.zeros(n, np.int64), cutoff)


def inverse_sensitive(cutoff, seed=0):
    """(L, dx): a box length and a separation near 1.5 L for which the exact division dx / L and the product dx fl(1 / L) round to
    different images (0.5 L < cutoff: the pair is an edge either way, with opposite displacements)"""
    rng = np.random.default_rng(seed)
    while True:
        L = f32(f32(cutoff) * f32(rng.uniform(1.2, 1.9)))
        dx = f32(f32(1.5) * L)
        for _ in range(6):
            if np.rint(dx / L) != np.rint(dx * (f32(1) / L)):
                return L, dx
            dx = np.nextafter(dx, f32(0))


def case_ties(cutoff):
    """two-atom molecules on each axis at cutoff - 1 ulp, cutoff, cutoff + 1 ulp; the constructed r2 = cut2 -+ 1 ulp vectors; diagonal
    periodic pairs at exactly half a box length (rint half-even keeps the image, half-away would take the other)"""
    cutoff = f32(cutoff)
    ds = [np.nextafter(cutoff, f32(0)), cutoff, np.nextafter(cutoff, f32(np.inf))]
    pos, cells = [], []
    origin = np.zeros(3, f32)
    for axis in range(3):
        for d in ds:
            v = np.zeros(3, f32)
            v[axis] = d
            pos += [np.zeros(3, f32), v]                          # (from the origin: the difference is exact)
            cells.append(np.zeros(9, f32))
    for seed in range(4):
        for v in on_threshold(cutoff, seed):
            pos += [np.zeros(3, f32), v]
            cells.append(np.zeros(9, f32))
    L = f32(1.55) * cutoff                                         # half a box length < cutoff: frac = +-0.5 exactly
    for axis in range(3):
        v = np.zeros(3, f32)
        v[axis] = L / 2
        pos += [origin, origin + v]
        assert (origin + v - origin)[axis] == L / 2
        cells.append(diag_cell(L, L, L))
    for axis in range(3):
        L, dx = inverse_sensitive(cutoff, axis)
        v = np.zeros(3, f32)
        v[axis] = dx
        pos += [origin, v]
        cells.append(diag_cell(L, L, L))
    B = len(cells)
    return Case(f'ties{float(cutoff):g}', np.array(pos), np.array(cells), _batch_of([2] * B), cutoff)


def _golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'case_boundary.npz'))


def case_boundary_a():
    """the 3-D near-tie vectors of tests/golden/case_boundary.npz (no cell)"""
    g = _golden()
    B = int(g['a_batch'].max()) + 1
    return Case('boundary a', g['a_pos'], np.zeros((B, 9), f32), g['a_batch'], float(g['cutoff']))


def case_boundary_b_diag():
    """the periodic pairs of the fixture at fractional separations +-0.5 +- k ulp, the molecules with a DIAGONAL cell (exact
    division: pinned; the general cells of the fixture are ties by design and stay with tests/test_hip_parity.py)"""
    g = _golden()
    cell = g['b_cell'].reshape(-1, 9)
    keep = np.flatnonzero(cell_kind(cell) == 1)
    sel = np.isin(g['b_batch'], keep)
    new = np.searchsorted(keep, g['b_batch'][sel])
    return Case('boundary b diagonal', g['b_pos'][sel], cell[keep], new, float(g['cutoff']))


def case_small_mols(B, seed=3):
    """B molecules of one or two atoms (the two atoms 0.8 cutoff apart), a few empty slots among them"""
    rng = np.random.default_rng(seed + B)
    sizes = rng.integers(1, 3, B)
    sizes[[1, B // 2]] = 0
    sizes[0], sizes[-1] = 2, 1
    n = int(sizes.sum())
    pos = rng.standard_normal((n, 3)) * 3
    first = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    two = np.flatnonzero(sizes == 2)
    pos[first[two] + 1] = pos[first[two]] + np.array([0.8, 0, 0])
    return Case(f'mols{B}', pos, np.zeros((B, 9), f32), _batch_of(sizes), 1.0)


def case_mol_sizes():
    """per-molecule route: sizes 1, 2, 7, 8, 9, 63, 64, 65 with empty slots first, in the middle and last (the last workgroup owns
    row_ptr[N]); periodic slots, diagonal and sheared"""
    sizes = [0, 1, 2, 7, 0, 8, 9, 63, 64, 65, 0]
    rng = np.random.default_rng(55)
    cells = [np.zeros(9, f32)] * 3 + [diag_cell(11, 12, 13), SHEARED, SHEARED, np.zeros(9, f32), diag_cell(12, 12, 12), SHEARED,
                                      np.zeros(9, f32), np.zeros(9, f32)]
    pos = np.concatenate([rng.random((n, 3)) * 10.5 for n in sizes])
    return Case('mol sizes', pos, np.array(cells), _batch_of(sizes), 5.0)


def case_small(n, seed=0):
    """single-launch route: n atoms in three molecules (an empty slot between them when n allows), diagonal and sheared cells"""
    rng = np.random.default_rng(900 + n + seed)
    if n < 3:
        sizes, cells = [n], [np.zeros(9, f32)]
    else:
        a = n // 3
        sizes, cells = [a, 0, a, n - 2 * a], [diag_cell(11, 12, 13), np.zeros(9, f32), SHEARED, np.zeros(9, f32)]
    side = 6.0 if n <= 128 else 6.0 * (n / 128.0) ** (1 / 3)
    pos = np.concatenate([rng.random((m, 3)) * (side if k != 3 else 1.5 * side) for k, m in enumerate(sizes)])
    if n == 2:
        pos = np.array([[0, 0, 0], [1.0, 2.0, 2.0]])
    cut = 5.0 if n <= 128 else 3.0
    return Case(f'small{n}', pos, np.array(cells), _batch_of(sizes), cut)


CELLS_CUTOFF = 0.9


def cells_box(cutoff=CELLS_CUTOFF):
    """(3, 4, 5) bins: the first length is the smallest float hip.py and make_grid accept; with bins exactly one cutoff wide (the
    CPU test's mutation) the second axis would have 5"""
    lo = f32(3.0003 * cutoff)
    while make_grid32([lo, lo, lo], cutoff) is not None:
        lo = np.nextafter(lo, f32(0))
    lo = np.nextafter(lo, f32(np.inf))
    box = np.array([lo, f32(5.0 * cutoff), f32(5.5 * cutoff)], f32)
    assert list(make_grid32(box, cutoff)[0]) == [3, 4, 5] and list(make_grid32(box, cutoff, f32(1))[0]) == [3, 5, 5]
    return box


def tight_pairs(L, cutoff, factor=BIN_FACTOR, want_lost=False):
    """per offset decade up to the supported range: the tightest pair two bins apart margin_search finds on a box length L (the
    lost pairs themselves when want_lost)"""
    out = []
    kmax = int(CELL_LIST_MAX_COORD * cutoff / float(L)) - 3
    if want_lost:
        ks = list(range(-kmax, kmax))
        for cross in (0, 1):
            out += margin_search(L, cutoff, ks, [k + cross for k in ks], factor=factor)[1][:3]
        return out
    for K in sorted({0, 1, 3, 10, kmax // 2, kmax, -1, -kmax}):
        if abs(K) > kmax:
            continue
        for kj in (K, K + 1 if K >= 0 else K - 1):
            best, lost, pair = margin_search(L, cutoff, [K], [kj], factor=factor, with_pair=True)
            if pair is not None:
                out.append(pair)
    return out


def case_cells(n_ball, cutoff=CELLS_CUTOFF):
    """One orthorhombic box of (3, 4, 5) bins.  A ball of n_ball atoms of diameter 0.9 cutoff with nothing else within two cutoffs of
    its centre (every row of the ball has degree n_ball - 1 exactly: 256 is the rank sort's full list, 257 the serial form; more
    than 64 atoms in one bin); an atom with no neighbour; atoms at exactly 0, -0.0, L, the float below L and at negative
    coordinates; random atoms; the tightest pairs two bins apart of the constructive search on the second and third axis, real
    grid and bins-exactly-one-cutoff grid; then every atom but the special ones displaced by whole box lengths, out to
    CELL_LIST_MAX_COORD cutoffs."""
    rng = np.random.default_rng(4242 + n_ball)
    box = cells_box(cutoff)
    b64 = box.astype(f64)
    centre = np.array([0.5, 0.5, 0.5]) * b64 / np.array([3, 4, 5]) + np.array([1, 2, 3]) * b64 / np.array([3, 4, 5])
    lonely = centre + np.array([0.0, -2.3 * cutoff, -2.6 * cutoff])
    rnd = rng.random((900, 3)) * b64

    def mi(d):
        return d - b64 * np.rint(d / b64)
    keep = (np.linalg.norm(mi(rnd - centre), axis=1) > 2.0 * cutoff) & (np.linalg.norm(mi(rnd - lonely), axis=1) > 1.2 * cutoff)
    rnd = rnd[keep][:420]
    k = rng.integers(-40, 41, (len(rnd), 3))
    kmax = np.floor(CELL_LIST_MAX_COORD * cutoff / b64).astype(int) - 1
    k = np.clip(k, -kmax, kmax)
    shifted = (rnd + k * b64)
    ball = _ball(rng, n_ball, 0.9 * cutoff) + centre + np.array([0, 1, -2]) * b64
    special = []
    for axis in range(3):
        L = box[axis]
        for v in (f32(0.0), f32(-0.0), L, np.nextafter(L, f32(0)), f32(-0.25) * L, -L, f32(-1e-8)):
            p = lonely + (np.array([1.3, 1.4, 1.5]) + len(special) * np.array([0.011, 0.007, 0.005])) * cutoff
            p = p.astype(f32)
            p[axis] = v
            special.append(p)
    pairs = []
    for axis in (1, 2):
        for factor in (BIN_FACTOR, f32(1)):
            for (pi, pj) in tight_pairs(box[axis], cutoff, factor, want_lost=factor == 1):
                base = (lonely + np.array([0.0, 0.0, 0.0])).astype(f32)
                a, b = base.copy(), base.copy()
                a[axis], b[axis] = pi, pj
                other = 2 if axis == 1 else 1
                a[other] = b[other] = f32(lonely[other] + (1.1 + 0.0065 * len(pairs)) * cutoff)    # (no two pairs are images of each other)
                a[0] = b[0] = f32(lonely[0] + 0.0041 * len(pairs) * cutoff)
                pairs += [a, b]
    pos = np.concatenate([shifted, ball, [lonely], np.array(special), np.array(pairs).reshape(-1, 3)]).astype(f32)
    order = rng.permutation(len(pos))
    pos = pos[order]
    assert np.abs(pos).max() <= CELL_LIST_MAX_COORD * cutoff
    cell = diag_cell(*box)
    return Case(f'cells{n_ball}', pos, cell[None], np.zeros(len(pos), np.int64), cutoff), box


def cells_candidates(case, box, factor=BIN_FACTOR):
    """the ordered pairs a cell list with this grid looks at (27 surrounding bins), as a boolean [N][N]"""
    nb, inv = make_grid32(box, case.cutoff, factor)
    b = np.stack([bin_coord32(case.pos[:, k], inv[k], int(nb[k])) for k in range(3)], axis=1)
    near = np.ones((case.N, case.N), bool)
    for k in range(3):
        gap = (b[:, None, k] - b[None, :, k]) % int(nb[k])
        near &= (gap <= 1) | (gap >= int(nb[k]) - 1)
    return near, b, nb


def reuse_inputs(cutoff=5.0, skin=1.0):
    """A candidate list (built with cutoff + skin on pos0) and the positions pos1 it is re-evaluated at: candidates inside and outside
    the cutoff, on r2 = cut2 and one ulp to either side (constructed), a whole row outside, x near 0 and within 1e-6 of 1."""
    rng = np.random.default_rng(77)
    parts0, parts1, cells = [], [], []
    a = rng.random((14, 3)) * 7.0
    parts0.append(a), parts1.append(a + rng.standard_normal(a.shape) * 0.25), cells.append(np.zeros(9, f32))
    b = rng.random((12, 3)) * 9.0
    parts0.append(b), parts1.append(b + rng.standard_normal(b.shape) * 0.25 + np.array([9.5, 0, -19.0]) * rng.integers(-1, 2, (12, 1)))
    cells.append(diag_cell(9.5, 10.0, 9.5))
    s = rng.random((10, 3)) * 8.0
    parts0.append(s), parts1.append(s + rng.standard_normal(s.shape) * 0.25), cells.append(SHEARED)
    th = on_threshold(cutoff, 11)
    for v in list(th) + [np.array([1e-3 * cutoff, 0, 0], f32) * np.array([0.6, 0.64, 0.48], f32) / f32(0.6),
                         (np.array([0.6, 0.64, 0.48]) * cutoff * (1 - 5e-7)).astype(f32)]:
        parts0.append(np.array([[0, 0, 0], [4.0, 1.0, 0.5]])), parts1.append(np.array([np.zeros(3), v])), cells.append(np.zeros(9, f32))
    parts0.append(np.array([[0.0, 0, 0], [4, 0, 0], [0, 4, 0]]))
    parts1.append(np.array([[-1.5, -1.5, 0], [4, 0, 0], [0, 4, 0]])), cells.append(np.zeros(9, f32))
    sizes = [len(p) for p in parts0]
    c0 = Case('reuse (build)', np.concatenate(parts0), np.array(cells), _batch_of(sizes), cutoff + skin)
    pos1 = np.concatenate(parts1).astype(f32)
    return c0, pos1, float(f32(cutoff))


def all_pairs_cases():
    return [case_sizes(), case_full(), case_chain(1023), case_chain(1024), case_chain(1025), case_chain(2049),
            case_ties(5.0), case_ties(1.0), case_ties(6.3), case_boundary_a(), case_boundary_b_diag()]


SMALL_N = (1, 2, 15, 16, 17, 64, 65, 1023, 1024)
MOL_B = (511, 512, 513, 8192, 8193)


@functools.lru_cache(None)
def gpu_cases():
    """{name: Case} of everything tests/test_hip_graph_stages.py builds a list of (the cell-list cases carry their box)"""
    cases = all_pairs_cases()
    cases += [case_mol_sizes(), case_full((64,), 5.0, 'full64'), case_full((65,), 5.0, 'full65'), case_full((64, 65), 5.0, 'full64+65')]
    cases += [case_small_mols(b) for b in MOL_B] + [case_small(n) for n in SMALL_N]
    out = {c.name: c for c in cases}
    for n in (257, 258):
        c, box = case_cells(n)
        c.box = box
        out[c.name] = c
    out['reuse (build)'] = reuse_inputs()[0]
    return out
