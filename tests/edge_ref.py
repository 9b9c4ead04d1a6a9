"""Float64 statements of the edge and pair stages the C interface exports one by one (include/newtonnet_hip.h, "Per-stage entry
points": nnhip_embed, nnhip_message_fwd / _bwd, nnhip_force_message_fwd / _bwd, nnhip_edge_embed_bwd, nnhip_head_out,
nnhip_edge_tangent_geom, nnhip_message_tan_fwd / _bwd, nnhip_force_message_tan_fwd / _bwd, nnhip_pair_rbf), each with a
COMPONENTWISE error bound computed in float64 from the magnitudes, in the manner of tests/dense_ref.py, so that
tests/test_hip_edge_stages.py asserts |got - ref| <= B element by element.  Numpy only, no GPU.

Every statement returns {output name: (reference, bound, defined)}; `defined` is a boolean array of the output's leading shape:
False where the interface leaves the entry unwritten (the kernel test then wants its NaN sentinel back bit for bit).

Bounds, u = 2^-24.  A sum of n fp32 terms in ANY order, each term formed with c roundings, is within (n + c + 2) u sum|term| of the
exact sum of the exact terms (|term| = the product of the factors' magnitudes; a fused multiply-add rounds once, and that rounding
is one of the n; the 2 covers the second-order products of roundings, as the 2 of dense_ref.product does).  The constants:

  FILTER_VALUE_C = 10   one read of the radial filter (csrc/edge_common.h:149-182).  Lagrange: a weight is a product of three
      correctly rounded factors (u - 1, u - 2, u + 1: one rounding each) and three multiplications: 6 u relative; the four-term
      fused chain adds 4 u of sum |w_k T_k|.  Hermite value T + a S + b D0 + c D1: a, b, c are products of at most five rounded
      quantities (5 u), the chain of three fused multiply-adds 3 u, 2 spare.  Both within 10 u A, A = sum |weight| |row|.
  FILTER_DERIV_C = 7    the Hermite derivative da S + db D0 + dc D1: da = 6 u v has 3 roundings; db = v (1 - 3u) and dc = u (3u - 2)
      hold a difference that may cancel, so their error is relative to the MAGNITUDES |v| (3u + |1 - 3u|) and u (3u + |3u - 2|):
      3 u of those, one more for v; the chain 3 u.  Within 7 u A', A' = sum magnitude |row|.
  G_C = 2               G = g_msg[p] + g_a[i] + g_a[j]: two additions, relative to |g_msg| + |g_a_i| + |g_a_j|.
  dot products over the 128 features (g_x, g_u, the head): n = 128 terms in the order of the lane reduction, whatever it is.
  activations: dense_ref.act_eval_err (4 u (1 + |x|)^2 absolute per evaluation).
  1 / r and 1 / cutoff: 3 u relative (a division, correctly rounded or not, and its use as a factor).
Each statement's docstring counts its own c.

Masked candidates (Verlet-skin lists: xg[e].x == FT_ZERO_ROW, both directions of a pair):
  * the message stages (message_fwd / _bwd, message_tan_*) do not test the mask: they read the table at FT_ZERO_ROW, whose rows are
    all zero, so eps = d eps = 0 and the edge contributes exactly nothing; the pair rows it owns are WRITTEN with zeros (msg,
    dmsg, g_x; g_eps = G m_i m_j and dg_eps do not read the filter and are written as for any pair).
  * the force stages skip a masked edge when xg is passed: it contributes nothing to f_out / g_fin / df_out / dg_fin, and the rows
    its pair owns -- g_h12, dg_h12, g_u of both directions -- are written with zeros.  With xg = NULL (nnhip_force_message_fwd /
    _bwd only) nothing is masked.
Undefined entries:
  * g_x[e] of message_bwd is defined only as the pair sum g_x[e] + g_x[rev e] (the owner's edge carries all of it today); the
    statement gives 'g_x_pair' [P] and the kernel test compares that sum.
  * g_m with need_gm = 0, the phi2 half of g_h12 / dg_h12 and g_fin / dg_fin with f_in = NULL, g_d without a virial: unwritten.
  * g_u[e][3], rb[p][nb:32], rb[p][32 + nb:64]: written as zero.
Ownership: a pair row is written from the edge of the LOWER endpoint.  For the value stages that cannot be read off the value: msg,
g_h12, g_eps and the g_x pair sum are symmetric under i <-> j (u_ji = -u_ij and x, eps are shared), so there a wrong owner only
shows as a row written twice or never, which the kernel test's sentinel and guard rows see.  Where a pair row is formed from a
per-directed-edge array that the interface does not require to be consistent over a pair -- tgeo (dmsg through dx_e, the first
half of dg_h12 through du_e), rbf / drbf (rb) -- the owner's edge is part of the statement, the inputs of the kernel tests differ
between the two directions, and the CPU tests check that rows taken from the other endpoint's edge leave the bound.
"""
import numpy as np

from tests import dense_ref as D

U = D.U
F = 128
FT_G = 3072                       # csrc/common.h
FT_ROWS = FT_G + 8
FT_ZERO_ROW = FT_G + 3
EDGE_ROWS = 4                     # csrc/edge_common.h
MOL_STAGE_MAX = 24                # NNHIP_MOL_STAGE_MAX
FILTER_VALUE_C, FILTER_DERIV_C, G_C, INV_C = 10, 7, 2, 3


# ---------------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------------
class Graph:
    """row_ptr [N+1], col [E] (ascending within a row), rev [E], pid [E], pair_ptr [N+1], mol_ptr [B+1], edge_index [2][E] int64
    (receiver; sender), geo [E][4] = (u, r) fp32 with u antisymmetric under reversal, xg [E][2] int32 = (table interval, fp32 bits
    of the fraction) of x = r / cutoff or (FT_ZERO_ROW, 0) for a masked candidate, masked [E] bool, xg_live: xg as if nothing
    were masked, cutoff."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def i(self):
        return self.edge_index[0]

    @property
    def j(self):
        return self.edge_index[1]

    @property
    def own(self):
        return self.j > self.i


def csr_arrays(n_atoms, pairs):
    """(row_ptr, col, rev, pid, pair_ptr) of the undirected pairs [(i, j)], by the conventions of csrc/graph.hip, "Undirected
    pairs": receiver CSR with ascending senders; pairs numbered in CSR order of their upper edge (i < j), so the upper edges of a
    row -- its LAST edges -- own a contiguous run of pair rows starting at pair_ptr[i]."""
    pairs = sorted({(min(a, b), max(a, b)) for a, b in pairs})
    assert all(0 <= a < b < n_atoms for a, b in pairs), 'pairs join two different atoms of the graph'
    ii = np.array([a for a, b in pairs] + [b for a, b in pairs], np.int64)
    jj = np.array([b for a, b in pairs] + [a for a, b in pairs], np.int64)
    order = np.lexsort((jj, ii))
    ii, jj = ii[order], jj[order]
    E = ii.size
    row_ptr = np.zeros(n_atoms + 1, np.int32)
    np.add.at(row_ptr, ii + 1, 1)
    row_ptr = np.cumsum(row_ptr).astype(np.int32)
    where = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(ii, jj))}
    rev = np.array([where[(int(b), int(a))] for a, b in zip(ii, jj)], np.int32).reshape(E)
    upper = jj > ii
    pid = np.zeros(E, np.int32)
    pid[upper] = np.arange(int(upper.sum()), dtype=np.int32)
    pid[~upper] = pid[rev[~upper]]
    pair_ptr = np.zeros(n_atoms + 1, np.int32)
    np.add.at(pair_ptr, ii[upper] + 1, 1)
    pair_ptr = np.cumsum(pair_ptr).astype(np.int32)
    return row_ptr, jj.astype(np.int32), rev, pid, pair_ptr, np.stack([ii, jj])


def stage_graph(adjacency, mol_sizes, masked_pairs=(), cutoff=5.0, seed=0, pos=None):
    """A graph for the stage tests from a list of undirected pairs, whatever geometry would produce it: the directions u are
    random unit vectors (antisymmetric under reversal), the distances random in (0.12, 0.97) cutoff, the table position follows
    from r as csrc/graph.hip:377-381 forms it (pos [N][3]: the directions and distances of that geometry instead).  Atoms of one
    molecule are consecutive; no pair may join two molecules (the
    molecule-resident kernels index a molecule's rows and edges relative to its first atom)."""
    n_atoms = int(np.sum(mol_sizes))
    mol_ptr = np.concatenate([[0], np.cumsum(mol_sizes)]).astype(np.int32)
    row_ptr, col, rev, pid, pair_ptr, edge_index = csr_arrays(n_atoms, adjacency)
    mol_of = np.repeat(np.arange(len(mol_sizes)), mol_sizes)
    assert (mol_of[edge_index[0]] == mol_of[edge_index[1]]).all(), 'a pair joins two molecules'
    E, P = col.size, col.size // 2
    rng = np.random.default_rng(seed)
    up = rng.standard_normal((P, 3))
    up = (up / np.linalg.norm(up, axis=1, keepdims=True)).astype(np.float32)
    rp = (cutoff * rng.uniform(0.12, 0.97, P)).astype(np.float32)
    own = edge_index[1] > edge_index[0]
    geo = np.zeros((E, 4), np.float32)
    geo[:, :3] = np.where(own[:, None], up[pid], -up[pid])
    geo[:, 3] = rp[pid]
    if pos is not None:
        d = (np.asarray(pos, np.float32)[edge_index[0]] - np.asarray(pos, np.float32)[edge_index[1]]).astype(np.float64)
        r = np.linalg.norm(d, axis=1, keepdims=True)
        geo = np.concatenate([d / r, r], axis=1).astype(np.float32)
    t = geo[:, 3].astype(np.float64) / cutoff * FT_G
    g0 = np.clip(np.floor(t).astype(np.int64), 0, FT_G - 1)
    frac = (t - g0).astype(np.float32)
    xg_live = np.stack([g0.astype(np.int32), frac.view(np.int32)], axis=1).astype(np.int32)
    masked_pairs = {(min(a, b), max(a, b)) for a, b in masked_pairs}
    masked = np.array([(min(a, b), max(a, b)) in masked_pairs for a, b in edge_index.T], bool).reshape(E)
    xg = xg_live.copy()
    xg[masked] = (FT_ZERO_ROW, 0)
    return Graph(N=n_atoms, E=E, P=P, B=len(mol_sizes), row_ptr=row_ptr, col=col, rev=rev, pid=pid, pair_ptr=pair_ptr,
                 mol_ptr=mol_ptr, edge_index=edge_index, geo=geo, xg=xg, xg_live=xg_live, masked=masked, cutoff=float(cutoff))


def degrees(g):
    return np.diff(g.row_ptr)


def _havel_hakimi(target):
    """pairs of a simple graph with exactly these degrees (asserts that the sequence is graphical)"""
    left = [[d, k] for k, d in enumerate(target)]
    pairs = []
    while True:
        left.sort(key=lambda t: (-t[0], t[1]))
        d, k = left[0]
        if d == 0:
            return pairs
        assert d < len(left) and all(left[q][0] > 0 for q in range(1, d + 1)), 'not a graphical degree sequence'
        left[0][0] = 0
        for q in range(1, d + 1):
            left[q][0] -= 1
            pairs.append((k, left[q][1]))


DEGREES_WANTED = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17)


def degrees_pairs():
    """37 atoms: degrees 17, 16, 15, 9, 8, 7, 3, 2, 1, then 26 atoms of degree 3 and one of 4, relabelled by a fixed permutation
    (atom 0 then has all its neighbours above it, atom 35 all below); atom 36 stays isolated"""
    target = [17, 16, 15, 9, 8, 7, 3, 2, 1] + [3] * 26 + [4]
    perm = np.random.default_rng(37).permutation(36)
    return [(int(perm[a]), int(perm[b])) for a, b in _havel_hakimi(target)]


def _row_pairs(pairs, i):
    return sorted((min(a, b), max(a, b)) for a, b in pairs if i in (a, b))


def graph_degrees(masked=False):
    """N = 37 in one molecule: 10 / 19 / 37 workgroups at 1 / 2 / 4 waves per row, none a multiple of 8.  masked: about a quarter
    of the pairs are masked candidates, among them every pair of one row and the last edge of a row of odd degree."""
    pairs = degrees_pairs()
    mp = ()
    if masked:
        g = stage_graph(pairs, [37])
        deg = degrees(g)
        rng = np.random.default_rng(5)
        und = sorted({(min(a, b), max(a, b)) for a, b in pairs})
        mp = {und[k] for k in rng.choice(len(und), len(und) // 5, replace=False)}
        all_row = int(np.flatnonzero((deg == 3) & (np.arange(37) > 0))[0])   # every edge of this row (not the molecule's first)
        mp |= set(_row_pairs(pairs, all_row))
        odd = int(np.flatnonzero((deg == 9) | (deg == 7))[0])                # the last edge of an odd row
        mp.add((min(odd, int(g.col[g.row_ptr[odd + 1] - 1])), max(odd, int(g.col[g.row_ptr[odd + 1] - 1]))))
    return stage_graph(pairs, [37], masked_pairs=mp, seed=1)


def graph_wide_row():
    """N = 135: atom 67 of degree 130 (70 neighbours below, 60 above: three ballot chunks of row_mid with the split inside the
    second) and atom 20 of degree 65, plus a few cross edges"""
    n = 135
    pairs = [(67, a) for a in range(n) if a not in (67, 1, 2, 133, 134)]
    odd = [a for a in range(1, n, 2) if a not in (67, 131, 133)]
    pairs += [(20, a) for a in odd] + [(1, 2), (2, 3), (100, 101), (5, 130)]
    g = stage_graph(pairs, [n], seed=2)
    assert degrees(g)[67] == 130 and degrees(g)[20] == 65
    return g


MOLECULE_SIZES = (1, 2, 8, 9, 24, 25, 30)


def graph_molecules():
    """sizes 1, 2, 8, 9, 24, 25, 30 (N = 99, B = 7: 8 B <= N <= 24 B).  The 24-atom molecule is fully connected: 552 directed edges,
    the most a staged molecule's geometry adjoint holds in LDS; 25 and 30 are not staged; 30 has more rows than the 8 waves."""
    rng = np.random.default_rng(9)
    pairs, a0 = [], 0
    for n in MOLECULE_SIZES:
        p = 1.0 if n in (2, 24) else 0.6
        pairs += [(a0 + a, a0 + b) for a in range(n) for b in range(a + 1, n) if rng.random() < p]
        a0 += n
    return stage_graph(pairs, list(MOLECULE_SIZES), seed=3)


def geometry_positions():
    """12 atoms in a 5.5 A cube: some pairs beyond the 5 A cutoff"""
    return (np.random.default_rng(21).random((12, 3)) * 5.5).astype(np.float32)


def graph_geometry():
    """the list of a real geometry (the kernel tests build the same one with hip.build_graph and compare the arrays)"""
    pos = geometry_positions()
    d = pos[:, None, :] - pos[None, :, :]
    r2 = (d[..., 2] * d[..., 2] + (d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0]))
    pairs = [(a, b) for a in range(12) for b in range(a + 1, 12) if r2[a, b] < np.float32(25.0)]
    return stage_graph(pairs, [12], pos=pos)


def graph_trivial(n):
    return stage_graph([], [n] if n else [])


GRAPHS = {'degrees': graph_degrees, 'wide row': graph_wide_row, 'molecules': graph_molecules,
          'masked': lambda: graph_degrees(masked=True), 'geometry': graph_geometry}


def xcd_tile(b, n_blocks):
    """csrc/common.h:190"""
    q, r = n_blocks >> 3, n_blocks & 7
    x, k = b & 7, b >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + k


# ---------------------------------------------------------------------------------------------------------------------------
# radial filter
# ---------------------------------------------------------------------------------------------------------------------------
def host_filter_table(W, freq, envelope=9):
    """The three planes T | S | D [3][FT_ROWS][F] of nnhip_filter_tables for eps(x) = W (env(x) sin(freq x) / x), formed in float64
    and rounded once (row = node + 1, nodes x_g = g / FT_G; zero from the cutoff on).  For the CPU tests: the kernel tests read
    the device-built table."""
    W, w = np.asarray(W, np.float64), np.asarray(freq, np.float64)
    g = np.arange(-1, FT_ROWS)                                  # one node more: the secant of the last row
    x = np.where(g == 0, 1e-9, g / FT_G)[:, None]
    p = float(envelope)
    env = 1 - 0.5 * (p + 1) * (p + 2) * x ** p + p * (p + 2) * x ** (p + 1) - 0.5 * p * (p + 1) * x ** (p + 2)
    denv = -0.5 * p * (p + 1) * (p + 2) * x ** (p - 1) * (1 - x) ** 2
    bes = np.sin(w * x) / x
    dbes = (w * np.cos(w * x) - bes) / x
    inside = (g < FT_G)[:, None]
    val = np.where(inside, (env * bes) @ W.T, 0.0)
    der = np.where(inside, (denv * bes + env * dbes) @ W.T, 0.0)
    return np.stack([val[:-1], (val[1:] - val[:-1]) * FT_G, der[:-1]]).astype(np.float32)


class TableFilter:
    """The radial filter as the kernels read it: float64 evaluation of the formulas of csrc/edge_common.h:149-182 on the fp32
    table [3][FT_ROWS][F] from the fp32 fraction stored in xg.  value(e): 4-point Lagrange on the T plane (eps, bound);
    hermite(e): (eps, d eps/dx, bound of eps, bound of d eps)."""

    def __init__(self, table, xg):
        self.tab = np.asarray(table, np.float64).reshape(3, FT_ROWS, F)
        xg = np.asarray(xg, np.int32).reshape(-1, 2)
        self.g0 = xg[:, 0].astype(np.int64)
        self.u = np.ascontiguousarray(xg[:, 1]).view(np.float32).astype(np.float64)

    def value(self, e):
        u, g0, T = self.u[e][:, None], self.g0[e], self.tab[0]
        w = [-u * (u - 1) * (u - 2) / 6, (u + 1) * (u - 1) * (u - 2) / 2, -(u + 1) * u * (u - 2) / 2, (u + 1) * u * (u - 1) / 6]
        eps = sum(w[k] * T[g0 + k] for k in range(4))
        mag = sum(np.abs(w[k] * T[g0 + k]) for k in range(4))
        return eps, FILTER_VALUE_C * U * mag

    def hermite(self, e):
        u, n0 = self.u[e][:, None], self.g0[e] + 1
        T0, S0, D0, D1 = self.tab[0][n0], self.tab[1][n0], self.tab[2][n0], self.tab[2][n0 + 1]
        h, v = 1.0 / FT_G, 1 - u
        a, b, c = h * u * u * (3 - 2 * u), h * u * v * v, -h * u * u * v
        eps = T0 + a * S0 + b * D0 + c * D1
        mag = np.abs(T0) + np.abs(a * S0) + np.abs(b * D0) + np.abs(c * D1)
        da, db, dc = 6 * u * v, v * (1 - 3 * u), u * (3 * u - 2)
        deps = da * S0 + db * D0 + dc * D1
        dmag = np.abs(da * S0) + np.abs(v) * (3 * u + np.abs(1 - 3 * u)) * np.abs(D0) + u * (3 * u + np.abs(3 * u - 2)) * np.abs(D1)
        return eps, deps, FILTER_VALUE_C * U * mag, FILTER_DERIV_C * U * dmag


class ExactFilter:
    """eps [E][F] and d eps/dx [E][F] given directly (no table, no rounding): the CPU tests of the derivative structure"""

    def __init__(self, eps, deps):
        self.eps, self.deps = np.asarray(eps, np.float64), np.asarray(deps, np.float64)

    def value(self, e):
        return self.eps[e], np.zeros_like(self.eps[e])

    def hermite(self, e):
        z = np.zeros_like(self.eps[e])
        return self.eps[e], self.deps[e], z, z


# ---------------------------------------------------------------------------------------------------------------------------
# what a statement reads of the graph
# ---------------------------------------------------------------------------------------------------------------------------
class View:
    """What a kernel reads of the graph, per directed edge: the receiver i, the sender j it gathers from, the weight of the edge in
    its row's sum, whether it is live (not masked), the direction u and distance r, the table position xg, which edge of a pair
    writes the pair's rows (`owner`: the lower endpoint's), the weight of g_a[j] in G and the sign with which the other endpoint's
    rows enter a pair row (u_ji = -u_ij); per atom, the rows nobody computes.  The statements take the plain view; the CPU tests
    hand them views of WRONG kernels (tests/test_edge_ref_host.py: mutated_view) to see that the bounds tell them apart."""

    def __init__(self, g, use_mask=True):
        self.g = g
        self.i, self.j = g.i.copy(), g.j.copy()
        self.w = np.ones(g.E)
        self.live = ~g.masked if use_mask else np.ones(g.E, bool)
        self.u = g.geo[:, :3].astype(np.float64)
        self.r = g.geo[:, 3].astype(np.float64)
        self.skip = np.zeros(g.N, bool)
        self.xg = g.xg
        self.owner = g.own
        self.ga_j, self.pair_sign = 1.0, 1.0

    def rows(self, terms, width):
        """sum of the per-edge rows `terms` [E][...] over each receiver's edges"""
        out = np.zeros((self.g.N,) + tuple(width))
        if self.g.E:
            w = self.w.reshape((-1,) + (1,) * len(width))
            np.add.at(out, self.i, w * terms)
        return out

    def done(self, rows):
        rows[self.skip] = 0.0
        return rows


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _n_edges(g):
    return degrees(g).astype(np.float64)


def _all(n):
    return np.ones(n, bool)


# ---------------------------------------------------------------------------------------------------------------------------
# value stages (csrc/edge.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def embed(z, table):
    """out[i] = table[z_i]: a copy, bound 0"""
    out = np.asarray(table, np.float64)[np.asarray(z)]
    return {'out': (out, np.zeros_like(out), _all(len(z)))}


def message_fwd(g, filt, m, a_in, view=None):
    """msg[p] = eps_e m_i m_j (owner's edge; Lagrange value);  a_mid[i] = a_in[i] + sum_e msg_e.
    msg: the filter's 10 u and two products, one spare: Beps |m_i m_j| + 3 u |msg|.  a_mid: n = deg + 1 terms, c = 10 + 2."""
    v = view or View(g)
    m, a_in = _f64(m), _f64(a_in)
    e = np.arange(g.E)
    eps, Be = TableFilter(filt.tab, v.xg).value(e) if isinstance(filt, TableFilter) else filt.value(e)
    mm = m[v.i] * m[v.j]
    t, mag = eps * mm, (Be / (FILTER_VALUE_C * U) if isinstance(filt, TableFilter) else np.abs(eps)) * np.abs(mm)
    own = v.owner
    msg, Bm = np.zeros((g.P, F)), np.zeros((g.P, F))
    msg[g.pid[own]], Bm[g.pid[own]] = t[own], (Be * np.abs(mm) + 3 * U * np.abs(t))[own]
    a_mid = v.done(a_in + v.rows(t, (F,)))
    n = _n_edges(g)[:, None] + 1
    Ba = (n + FILTER_VALUE_C + 2 + 2) * U * (np.abs(a_in) + v.rows(mag, (F,)))
    return {'msg': (msg, Bm, _all(g.P)), 'a_mid': (a_mid, Ba, _all(g.N))}


def _G(g, v, g_msg, g_a):
    G = g_msg[g.pid] + g_a[v.i] + v.ga_j * g_a[v.j]
    MG = np.abs(g_msg[g.pid]) + np.abs(g_a[v.i]) + np.abs(g_a[v.j])
    return G, MG


def _filter_for(filt, v):
    return TableFilter(filt.tab, v.xg) if isinstance(filt, TableFilter) else filt


def _split_filter(g, filt, v):
    """(eps, magnitude of eps, d eps, magnitude of d eps) per directed edge as message_bwd reads them: Hermite for the edges whose
    row owns the pair, Lagrange value alone for the others"""
    filt = _filter_for(filt, v)
    e = np.arange(g.E)
    table = isinstance(filt, TableFilter)
    ev, Bv = filt.value(e)
    eh, dh, Bh, Bd = filt.hermite(e)
    own = g.own[:, None]                 # (which form a row reads follows its two ranges, not who writes)
    eps = np.where(own, eh, ev)
    Me = np.where(own, Bh, Bv) / (FILTER_VALUE_C * U) if table else np.abs(eps)
    Md = Bd / (FILTER_DERIV_C * U) if table else np.abs(dh)
    return eps, Me, dh, Md


def message_bwd(g, filt, g_msg, g_a, m, need_gm=1, view=None):
    """G = g_msg[p] + g_a[i] + g_a[j];  g_m[i] = sum_e G eps m_j (need_gm; eps: Hermite on the pairs the row owns, Lagrange on the
    others);  g_x_pair[p] = < G m_i m_j, d eps/dx > of the owner's edge (the only defined combination of g_x, see the module).
    g_m: n = deg terms, c = 2 (G) + 10 (eps) + 1 (G eps).  g_x: n = 128, c = 2 (G) + 7 (d eps) + 3 products."""
    v = view or View(g)
    g_msg, g_a, m = _f64(g_msg), _f64(g_a), _f64(m)
    G, MG = _G(g, v, g_msg, g_a)
    eps, Me, deps, Md = _split_filter(g, filt, v)
    out = {}
    t, mag = G * eps * m[v.j], MG * Me * np.abs(m[v.j])
    g_m = v.done(v.rows(t, (F,)))
    Bg = (_n_edges(g)[:, None] + G_C + FILTER_VALUE_C + 1 + 2) * U * v.rows(mag, (F,))
    out['g_m'] = (g_m, Bg, _all(g.N) if need_gm else ~_all(g.N))
    own = v.owner
    mm = m[v.i] * m[v.j]
    gx, Bx = np.zeros(g.P), np.zeros(g.P)
    gx[g.pid[own]] = (G * mm * deps).sum(axis=1)[own]
    Bx[g.pid[own]] = ((F + G_C + FILTER_DERIV_C + 3 + 2) * U * (MG * np.abs(mm) * Md).sum(axis=1))[own]
    gx[g.pid[own & v.skip[g.i]]] = 0.0
    out['g_x_pair'] = (gx, Bx, _all(g.P))
    return out


def force_message_fwd(g, phi1, phi2, f_in=None, use_mask=True, view=None):
    """f_out[i][k] = f_in[i][k] + sum_e phi1[p] u_e[k] + phi2[p] f_in[j][k]   (f_in NULL: the first layer, no phi2 term; masked edges
    skipped when xg is passed).  Every term is one fused multiply-add: n = deg (1 or 2) + 1, c = 0."""
    v = view or View(g, use_mask)
    phi1, phi2 = _f64(phi1), _f64(phi2)
    live = v.live[:, None, None]
    t = phi1[g.pid][:, None, :] * v.u[:, :, None]
    mag = np.abs(t)
    per = 1
    f0 = np.zeros((g.N, 3, F))
    if f_in is not None:
        f0 = _f64(f_in)
        t2 = phi2[g.pid][:, None, :] * f0[v.j]
        t, mag, per = t + t2, mag + np.abs(t2), 2
    f_out = v.done(f0 + v.rows(np.where(live, t, 0.0), (3, F)))
    n = per * _n_edges(g)[:, None, None] + 1
    B = (n + 2) * U * (np.abs(f0) + v.rows(np.where(live, mag, 0.0), (3, F)))
    return {'f_out': (f_out, B, _all(g.N))}


def force_message_bwd(g, gf, phi1, phi2, f_in=None, use_mask=True, view=None):
    """g_h12[p] = ( sum_k (gf_i - gf_j)[k] u_e[k]  |  sum_k gf_i[k] f_j[k] + gf_j[k] f_i[k] )  for the owner's edge (i < j), zeros for
    a masked pair; the phi2 half only with f_in;  g_u[e] = (< gf_i[k], phi1[p] >_k, 0), zeros for a masked edge;
    g_fin[i][k] = gf[i][k] + sum_e phi2[p] gf[j][k]  (only with f_in).
    g_h12 first half: 3 terms, one subtraction each: (3 + 1 + 2) u;  second half: 6 fused terms: (6 + 2) u;  g_u: n = 128;
    g_fin: n = deg + 1."""
    v = view or View(g, use_mask)
    gf = _f64(gf)
    phi1, phi2 = _f64(phi1), _f64(phi2)
    own, live = v.owner, v.live
    has_f = f_in is not None
    out = {}
    gh, Bh = np.zeros((g.P, 2 * F)), np.zeros((g.P, 2 * F))
    d = gf[v.i] - v.pair_sign * gf[v.j]                  # (u_ji = -u_ij: the other endpoint's rows enter with the opposite sign)
    u3 = v.u[:, :, None]
    first = (d * u3).sum(axis=1)
    Bfirst = 6 * U * ((np.abs(gf[v.i]) + np.abs(gf[v.j])) * np.abs(u3)).sum(axis=1)
    sel = own & live
    gh[g.pid[sel], :F], Bh[g.pid[sel], :F] = first[sel], Bfirst[sel]
    if has_f:
        f0 = _f64(f_in)
        second = (gf[v.i] * f0[v.j] + gf[v.j] * f0[v.i]).sum(axis=1)
        Bsecond = 8 * U * (np.abs(gf[v.i] * f0[v.j]) + np.abs(gf[v.j] * f0[v.i])).sum(axis=1)
        gh[g.pid[sel], F:], Bh[g.pid[sel], F:] = second[sel], Bsecond[sel]
    dh = np.ones((g.P, 2 * F), bool)
    dh[:, F:] = has_f
    out['g_h12'] = (gh, Bh, dh)
    gu, Bu = np.zeros((g.E, 4)), np.zeros((g.E, 4))
    p1 = phi1[g.pid][:, None, :]
    gu[:, :3] = np.where(live[:, None], (gf[v.i] * p1).sum(axis=2), 0.0)
    Bu[:, :3] = np.where(live[:, None], (F + 2) * U * np.abs(gf[v.i] * p1).sum(axis=2), 0.0)
    gu[v.skip[g.i]] = 0.0
    out['g_u'] = (gu, Bu, _all(g.E))
    if has_f:
        t = np.where(live[:, None, None], phi2[g.pid][:, None, :] * gf[v.j], 0.0)
        g_fin = v.done(gf + v.rows(t, (3, F)))
        B = (_n_edges(g)[:, None, None] + 1 + 2) * U * (np.abs(gf) + v.rows(np.abs(t), (3, F)))
        out['g_fin'] = (g_fin, B, _all(g.N))
    else:
        out['g_fin'] = (np.zeros((g.N, 3, F)), np.zeros((g.N, 3, F)), ~_all(g.N))
    return out


def edge_embed_bwd(g, g_x, g_u, pos=None, want_virial=False, view=None):
    """g_d[e] = (gx / cutoff - (gu . u) / r) u + gu / r  with gx = sum_l g_x[l][e], gu = sum_l g_u[l][e][0:3];
    forces[i] = - sum_{e in row i} (g_d[e] - g_d[rev e]);  virial[b] = - sym( sum_{e in b} (pos_i - pos_j) (x) g_d[e] ) for a
    molecule without a cell (cell = 0).  g_d is written only on the path that also forms the virial.
    g_d: with Ma = |gx| / cutoff + (|gu| . |u|) / r (magnitudes summed over the layers) the coefficient a = gx / cutoff - dot / r
    carries L layer additions, 3 + 2 for the dot product, 3 for 1 / r or 1 / cutoff, the product and the subtraction: (L + 9) u
    Ma; the fused a u_k + gu_k / r one more: (L + 10) u (Ma |u_k| + |gu_k| / r).
    forces: n = deg terms, each a rounded difference of two g_d (their own bounds ride along): (deg + 1 + 2) u.
    virial: fp64 sums of products of the kernel's fp32 g_d, rounded once: the g_d bounds weighted by |pos_i - pos_j|, + u."""
    v = view or View(g)
    g_x = _f64(g_x)
    L = g_x.shape[0] if g_x.ndim > 1 else 1
    g_x, g_u = g_x.reshape(L, g.E), _f64(g_u).reshape(L, g.E, 4)
    gx, gu = g_x.sum(axis=0), g_u[:, :, :3].sum(axis=0)
    Mx, Mu = np.abs(g_x).sum(axis=0), np.abs(g_u[:, :, :3]).sum(axis=0)
    u, r, rc = v.u, v.r[:, None], g.cutoff
    a = gx[:, None] / rc - (gu * u).sum(axis=1, keepdims=True) / r
    Ma = Mx[:, None] / rc + (Mu * np.abs(u)).sum(axis=1, keepdims=True) / r
    gd, Bd = np.zeros((g.E, 4)), np.zeros((g.E, 4))
    gd[:, :3] = a * u + gu / r
    Bd[:, :3] = (L + INV_C + 7) * U * (Ma * np.abs(u) + Mu / r)
    out = {'g_d': (gd, Bd, _all(g.E) if want_virial else ~_all(g.E))}
    rev = g.rev
    forces = v.done(-v.rows(gd[:, :3] - gd[rev, :3], (3,)))
    mag = np.abs(gd[:, :3]) + np.abs(gd[rev, :3])
    Bf = (_n_edges(g)[:, None] + 3) * U * v.rows(mag, (3,)) + v.rows(Bd[:, :3] + Bd[rev, :3], (3,))
    out['forces'] = (forces, Bf, _all(g.N))
    if want_virial:
        pos = _f64(pos)
        dp = pos[g.i] - pos[g.j]
        mol = np.searchsorted(g.mol_ptr, g.i, side='right') - 1
        s, Bs = np.zeros((g.B, 3, 3)), np.zeros((g.B, 3, 3))
        np.add.at(s, mol, dp[:, :, None] * gd[:, None, :3])
        np.add.at(Bs, mol, np.abs(dp)[:, :, None] * Bd[:, None, :3])
        vir = -0.5 * (s + s.transpose(0, 2, 1))
        out['virial'] = (vir, 0.5 * (Bs + Bs.transpose(0, 2, 1)) + 2 * U * np.abs(vir), _all(g.B))
    return out


def head_out(e2, w4, b4, scale, shift, z, mol_ptr, activation='silu', want_g=True):
    """atom_energy[i] = (< act(e2_i), w4 > + b4) scale[z_i] + shift[z_i];  g_e2[i] = scale[z_i] w4 act'(e2_i);  energy[b] = the sum
    of the molecule's atom energies (scale / shift NULL: 1 / 0).
    The dot product: n = 128 (the activations carry dense_ref.act_eval_err each).  atom_energy: the sum + b4 and the fused
    multiply-add round once each: 2 u (|scale| (|s| + |b4|) + |shift|).  g_e2: two products and the activation: 3 u.
    energy: the device adds the fp32 atom energies IN FLOAT64 and rounds once: the atoms' bounds + u |E| -- no term in the
    number of atoms."""
    e2, w4 = _f64(e2), _f64(w4)
    b4 = float(np.asarray(b4).reshape(-1)[0])
    z = np.asarray(z)
    n = e2.shape[0]
    sc = np.ones(n) if scale is None else _f64(scale)[z]
    sh = np.zeros(n) if shift is None else _f64(shift)[z]
    a = D.act(activation, e2)
    s = a @ w4
    Bs = (F + 2) * U * (np.abs(a) @ np.abs(w4)) + D.act_eval_err(e2) @ np.abs(w4)
    ae = (s + b4) * sc + sh
    Bae = np.abs(sc) * Bs + 2 * U * (np.abs(sc) * (np.abs(s) + abs(b4)) + np.abs(sh))
    d = D.dact(activation, e2)
    ge = sc[:, None] * w4 * d
    Bge = np.abs(sc[:, None] * w4) * D.act_eval_err(e2) + 3 * U * np.abs(ge)
    B = len(mol_ptr) - 1
    mol = np.searchsorted(mol_ptr, np.arange(n), side='right') - 1
    E, BE = np.zeros(B), np.zeros(B)
    np.add.at(E, mol, ae)
    np.add.at(BE, mol, Bae)
    return {'atom_energy': (ae, Bae, _all(n)), 'g_e2': (ge, Bge, _all(n) if want_g else ~_all(n)),
            'energy': (E, BE + U * np.abs(E), _all(B))}


# ---------------------------------------------------------------------------------------------------------------------------
# tangent stages (csrc/train.hip): one wave per row, every edge reads the Hermite form
# ---------------------------------------------------------------------------------------------------------------------------
def edge_tangent_geom(g, vdir, sign):
    """dd = sign (v_i - v_j);  dr = u . dd;  tgeo[e] = ((dd - u dr) / r, dr / cutoff).
    dd: 2 roundings; dr: 3 + 1 more; dd - u dr: product and difference; 1 / r: 3 -- (2 + 4 + 2 + 3 + 1) = 12 u of
    (|dd| + |u| (|u| . |dd|)) / r;  dx: (6 + 2) u of (|u| . |dd|) / cutoff."""
    vdir = _f64(vdir)
    u, r = g.geo[:, :3].astype(np.float64), g.geo[:, 3:4].astype(np.float64)
    dd = sign * (vdir[g.i] - vdir[g.j])
    Md = abs(sign) * (np.abs(vdir[g.i]) + np.abs(vdir[g.j]))
    dr = (u * dd).sum(axis=1, keepdims=True)
    Mr = (np.abs(u) * Md).sum(axis=1, keepdims=True)
    t = np.concatenate([(dd - u * dr) / r, dr / g.cutoff], axis=1)
    B = np.concatenate([12 * U * (Md + np.abs(u) * Mr) / r, 8 * U * Mr / g.cutoff], axis=1)
    return {'tgeo': (t, B, _all(g.E))}


def message_tan_fwd(g, filt, m, tgeo, dm=None, da_in=None, view=None):
    """dmsg[p] = d eps dx m_i m_j + eps (dm_i m_j + m_i dm_j) (owner's edge);  da_mid[i] = da_in[i] + sum_e dmsg_e  (dm = da_in = NULL:
    the first layer).  A term: 7 (d eps) + 3 products, 10 (eps) + 3 + the fused product: within 14 u of its magnitude; dmsg one
    spare (15 u); da_mid: n = deg + 1, c = 14."""
    v = view or View(g)
    m, dx = _f64(m), _f64(tgeo)[:, 3:4]
    filt = _filter_for(filt, v)
    table = isinstance(filt, TableFilter)
    eps, deps, Be, Bd = filt.hermite(np.arange(g.E))
    Me = Be / (FILTER_VALUE_C * U) if table else np.abs(eps)
    Md = Bd / (FILTER_DERIV_C * U) if table else np.abs(deps)
    mm = m[v.i] * m[v.j]
    t, mag = deps * dx * mm, Md * np.abs(dx * mm)
    a0 = np.zeros((g.N, F))
    if dm is not None:
        dm, a0 = _f64(dm), _f64(da_in)
        t = t + eps * (dm[v.i] * m[v.j] + m[v.i] * dm[v.j])
        mag = mag + Me * (np.abs(dm[v.i] * m[v.j]) + np.abs(m[v.i] * dm[v.j]))
    own = v.owner
    dmsg, Bm = np.zeros((g.P, F)), np.zeros((g.P, F))
    dmsg[g.pid[own]], Bm[g.pid[own]] = t[own], 15 * U * mag[own]
    da = v.done(a0 + v.rows(t, (F,)))
    Ba = (_n_edges(g)[:, None] + 1 + 14 + 2) * U * (np.abs(a0) + v.rows(mag, (F,)))
    return {'dmsg': (dmsg, Bm, _all(g.P)), 'da_mid': (da, Ba, _all(g.N))}


def force_message_tan_fwd(g, phi1, dphi1, phi2, dphi2, tgeo, f_in=None, df_in=None, view=None):
    """df_out[i][k] = df_in[i][k] + sum_e dphi1 u_k + phi1 du_k + dphi2 f_j[k] + phi2 df_j[k]   (masked edges skipped; f_in = df_in =
    NULL: the phi1 terms only).  Fused terms: n = deg (2 or 4) + 1, c = 0."""
    v = view or View(g)
    phi1, phi2 = _f64(phi1), _f64(phi2)
    dphi1, dphi2 = _f64(dphi1), _f64(dphi2)
    du = _f64(tgeo)[:, :3, None]
    live = v.live[:, None, None]
    t1, t2 = dphi1[g.pid][:, None, :] * v.u[:, :, None], phi1[g.pid][:, None, :] * du
    t, mag, per = t1 + t2, np.abs(t1) + np.abs(t2), 2
    d0 = np.zeros((g.N, 3, F))
    if f_in is not None:
        f0, d0 = _f64(f_in), _f64(df_in)
        t3, t4 = dphi2[g.pid][:, None, :] * f0[v.j], phi2[g.pid][:, None, :] * d0[v.j]
        t, mag, per = t + t3 + t4, mag + np.abs(t3) + np.abs(t4), 4
    out = v.done(d0 + v.rows(np.where(live, t, 0.0), (3, F)))
    B = (per * _n_edges(g)[:, None, None] + 1 + 2) * U * (np.abs(d0) + v.rows(np.where(live, mag, 0.0), (3, F)))
    return {'df_out': (out, B, _all(g.N))}


def force_message_tan_bwd(g, gf, dgf, phi2, dphi2, tgeo, f_in=None, df_in=None, view=None):
    """dg_h12[p] = ( sum_k (dgf_i - dgf_j)[k] u_k + (gf_i - gf_j)[k] du_k  |  sum_k dgf_i f_j + gf_i df_j + dgf_j f_i + gf_j df_i ) for
    the owner's edge, zeros for a masked pair, the second half only with f_in;
    dg_fin[i][k] = dgf[i][k] + sum_e dphi2 gf_j[k] + phi2 dgf_j[k]  (only with f_in).
    first half: 6 terms, a subtraction each: (6 + 1 + 2) u;  second: 12 fused terms: (12 + 2) u;  dg_fin: n = 2 deg + 1."""
    v = view or View(g)
    gf, dgf, phi2, dphi2 = _f64(gf), _f64(dgf), _f64(phi2), _f64(dphi2)
    du, u3 = _f64(tgeo)[:, :3, None], v.u[:, :, None]
    own, live = v.owner, v.live
    has_f = f_in is not None
    sel = own & live
    gh, Bh = np.zeros((g.P, 2 * F)), np.zeros((g.P, 2 * F))
    sgn = v.pair_sign
    first = ((dgf[v.i] - sgn * dgf[v.j]) * u3 + (gf[v.i] - sgn * gf[v.j]) * du).sum(axis=1)
    Bfirst = 9 * U * ((np.abs(dgf[v.i]) + np.abs(dgf[v.j])) * np.abs(u3) + (np.abs(gf[v.i]) + np.abs(gf[v.j])) * np.abs(du)).sum(axis=1)
    gh[g.pid[sel], :F], Bh[g.pid[sel], :F] = first[sel], Bfirst[sel]
    out = {}
    if has_f:
        f0, d0 = _f64(f_in), _f64(df_in)
        parts = (dgf[v.i] * f0[v.j], gf[v.i] * d0[v.j], dgf[v.j] * f0[v.i], gf[v.j] * d0[v.i])
        second = sum(parts).sum(axis=1)
        Bsecond = 14 * U * sum(np.abs(q) for q in parts).sum(axis=1)
        gh[g.pid[sel], F:], Bh[g.pid[sel], F:] = second[sel], Bsecond[sel]
        lv = live[:, None, None]
        t1, t2 = dphi2[g.pid][:, None, :] * gf[v.j], phi2[g.pid][:, None, :] * dgf[v.j]
        fin = v.done(dgf + v.rows(np.where(lv, t1 + t2, 0.0), (3, F)))
        Bf = (2 * _n_edges(g)[:, None, None] + 1 + 2) * U * (np.abs(dgf) + v.rows(np.where(lv, np.abs(t1) + np.abs(t2), 0.0), (3, F)))
        out['dg_fin'] = (fin, Bf, _all(g.N))
    else:
        out['dg_fin'] = (np.zeros((g.N, 3, F)), np.zeros((g.N, 3, F)), ~_all(g.N))
    dh = np.ones((g.P, 2 * F), bool)
    dh[:, F:] = has_f
    out['dg_h12'] = (gh, Bh, dh)
    return out


def message_tan_bwd(g, filt, g_msg, dg_msg, ga, dga, m, tgeo, dm=None, view=None):
    """G = g_msg[p] + ga_i + ga_j, dG likewise;  dg_m[i] = sum_e (dG eps + G d eps dx) m_j + G eps dm_j;
    g_eps[p] = G m_i m_j;  dg_eps[p] = dG m_i m_j + G (dm_i m_j + m_i dm_j)   (owner's edge; dm NULL: the first layer).
    dg_m: n = deg (1 or 2) fused terms, c = 2 (G) + 10 or 7 (filter) + 3 products + 1: 16;  g_eps: 2 + 2 + 1 = 5 u;
    dg_eps: 2 + 2 + 3 + 1 = 8 u."""
    v = view or View(g)
    g_msg, dg_msg, ga, dga, m = _f64(g_msg), _f64(dg_msg), _f64(ga), _f64(dga), _f64(m)
    dx = _f64(tgeo)[:, 3:4]
    G, MG = _G(g, v, g_msg, ga)
    dG, MdG = _G(g, v, dg_msg, dga)
    filt = _filter_for(filt, v)
    table = isinstance(filt, TableFilter)
    eps, deps, Be, Bd = filt.hermite(np.arange(g.E))
    Me = Be / (FILTER_VALUE_C * U) if table else np.abs(eps)
    Md = Bd / (FILTER_DERIV_C * U) if table else np.abs(deps)
    mj = m[v.j]
    t = (dG * eps + G * deps * dx) * mj
    mag = (MdG * Me + MG * Md * np.abs(dx)) * np.abs(mj)
    per = 1
    mm = m[v.i] * mj
    de, Mde = dG * mm, MdG * np.abs(mm)
    if dm is not None:
        dm = _f64(dm)
        t, mag, per = t + G * eps * dm[v.j], mag + MG * Me * np.abs(dm[v.j]), 2
        inner = dm[v.i] * mj + m[v.i] * dm[v.j]
        de, Mde = de + G * inner, Mde + MG * (np.abs(dm[v.i] * mj) + np.abs(m[v.i] * dm[v.j]))
    dg_m = v.done(v.rows(t, (F,)))
    Bm = (per * _n_edges(g)[:, None] + 16 + 2) * U * v.rows(mag, (F,))
    own = v.owner
    ge, Bge, dge, Bdge = (np.zeros((g.P, F)) for _ in range(4))
    ge[g.pid[own]], Bge[g.pid[own]] = (G * mm)[own], (5 * U * MG * np.abs(mm))[own]
    dge[g.pid[own]], Bdge[g.pid[own]] = de[own], (8 * U * Mde)[own]
    return {'dg_m': (dg_m, Bm, _all(g.N)), 'g_eps': (ge, Bge, _all(g.P)), 'dg_eps': (dge, Bdge, _all(g.P))}


def pair_rbf(g, rbf, drbf, tgeo, view=None):
    """rb[p][0:nb] = rbf_e, rb[p][32:32 + nb] = drbf_e dx_e for the owner's edge, zero padded to [P][64]: a copy and one product"""
    rbf, drbf, dx = _f64(rbf), _f64(drbf), _f64(tgeo)[:, 3:4]
    nb = rbf.shape[1]
    own = (view or View(g)).owner
    rb, B = np.zeros((g.P, 64)), np.zeros((g.P, 64))
    rb[g.pid[own], :nb] = rbf[own]
    rb[g.pid[own], 32:32 + nb] = (drbf * dx)[own]
    B[:, 32:32 + nb] = U * np.abs(rb[:, 32:32 + nb])
    return {'rb': (rb, B, _all(g.P))}


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' own order of operations in fp32 (numpy on the host): "the bound really bounds"
# ---------------------------------------------------------------------------------------------------------------------------
f32 = np.float32


def fma32(a, b, c):
    """a b + c rounded once (the product of two fp32 numbers is exact in float64; the float64 sum rounds a second time only
    below 2^-29 of an fp32 ulp)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def filter32(table, xg, e):
    """filter_weights / filter_value / filter_value_deriv of csrc/edge_common.h in fp32: (Lagrange eps, Hermite eps, d eps) [F]"""
    tab = np.asarray(table, f32).reshape(3, FT_ROWS, F)
    g0 = int(xg[e, 0])
    u = np.ascontiguousarray(xg[e:e + 1, 1]).view(f32)[0]
    one, two, three, six = f32(1), f32(2), f32(3), f32(6)
    um1, um2, up1 = u - one, u - two, u + one
    w = [-u * um1 * um2 * f32(1.0 / 6.0), up1 * um1 * um2 * f32(0.5), -up1 * u * um2 * f32(0.5), up1 * u * um1 * f32(1.0 / 6.0)]
    lag = tab[0][g0] * w[0]
    for k in range(1, 4):
        lag = fma32(tab[0][g0 + k], w[k], lag)
    h, v, uu = f32(1.0) / f32(FT_G), one - u, u * u
    a, b, c = h * uu * (three - two * u), h * u * v * v, -h * uu * v
    da, db, dc = six * u * v, v * (one - three * u), u * (three * u - two)
    n0 = g0 + 1
    t0, s0, d0, d1 = tab[0][n0], tab[1][n0], tab[2][n0], tab[2][n0 + 1]
    her = fma32(d1, c, fma32(d0, b, fma32(s0, a, t0)))
    der = fma32(d1, dc, fma32(d0, db, s0 * da))
    return lag, her, der


def row_sum32(ranges, wpr, step, width, first=None):
    """The summation order of the split-row kernels (csrc/edge.hip, csrc/edge_common.h "Split rows"): wave `part` of the row's wpr
    waves walks the edge pairs 2 part, 2 part + 2 wpr, ... of each range; the lower half-wave takes the even edge, the upper the
    odd one; the halves are folded once per wave, then the waves' sums are added in wave order.
    step(acc, e) -> acc: what one edge adds to an accumulator [width] in fp32; first: the start of part 0's lower half."""
    parts = []
    for part in range(wpr):
        lo = np.zeros(width, f32) if (first is None or part) else np.asarray(first, f32).copy()
        hi = np.zeros(width, f32)
        for beg, end in ranges:
            for e in range(beg + 2 * part, end, 2 * wpr):
                lo = step(lo, e)
                if e + 1 < end:
                    hi = step(hi, e + 1)
        parts.append(lo + hi)
    acc = parts[0]
    for q in parts[1:]:
        acc = acc + q
    return acc


def tree_sum32(x):
    """a 128-term dot product's additions as a halving tree in fp32 (the lane reduction's order is the compiler's; any order is
    inside the bound)"""
    x = np.asarray(x, f32).copy()
    n = x.shape[-1]
    while n > 1:
        n //= 2
        x = x[..., :n] + x[..., n:2 * n]
    return x[..., 0]


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: independent random fp32 arrays of ordinary size, the same for the CPU tests of the bounds and for the kernel tests
# ---------------------------------------------------------------------------------------------------------------------------
N_LAYERS, N_BASIS = 3, 20
SPECIES = np.array([0, 1, 6, 7, 8, 118])


def stage_inputs(g, seed=0):
    import zlib
    rng = np.random.default_rng(zlib.crc32(repr(('edge stages', g.N, g.E, seed)).encode()))

    def r(*shape, scale=1.0):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    N, E, P = g.N, g.E, g.P
    d = dict(m=r(N, F), a_in=r(N, F), g_msg=r(P, F), g_a=r(N, F), phi1=r(P, F), phi2=r(P, F), f_in=r(N, 3, F), gf=r(N, 3, F),
             g_x=r(N_LAYERS, E), g_u=r(N_LAYERS, E, 4), pos=r(N, 3, scale=2.0), e2=r(N, F, scale=2.0), w4=r(F, scale=0.3), b4=r(1),
             scale=r(119) + np.float32(2.0), shift=r(119), z=SPECIES[rng.integers(0, len(SPECIES), N)].astype(np.int64),
             embedding=r(119, F), v=r(N, 3), dm=r(N, F), da_in=r(N, F), dphi1=r(P, F), dphi2=r(P, F), df_in=r(N, 3, F), dgf=r(N, 3, F),
             dg_msg=r(P, F), dga=r(N, F), tgeo=r(E, 4), rbf=r(E, N_BASIS), drbf=r(E, N_BASIS))
    return d


def filter_weights(seed=7):
    """(message_edgepart weight [F][N_BASIS], frequencies [N_BASIS]) of the table the stage tests read"""
    rng = np.random.default_rng(seed)
    W = ((rng.random((F, N_BASIS)) * 2 - 1) / np.sqrt(N_BASIS)).astype(np.float32)
    return W, (np.arange(1, N_BASIS + 1) * np.pi).astype(np.float32)
