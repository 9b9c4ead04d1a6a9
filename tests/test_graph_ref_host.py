"""The statement of tests/graph_ref.py checked on the CPU: what tests/test_hip_graph_stages.py compares the neighbour-list builders and
the edge geometry kernels with must itself be right, and the inputs of that file must be sharp enough to tell a wrong builder from
a right one.  No GPU.

  * fma32 is the correctly rounded fused multiply-add (against exact rational arithmetic, constructed midpoints included);
  * the statement reproduces tests/golden/case_boundary.npz (edge lists exactly, a_disp bit for bit, b_disp to the fixture's 2e-6)
    and equals oracle.newtonnet_ref.radius_graph on a periodic diagonal batch, a sheared batch and a non-periodic batch;
  * on every case of the GPU file: cut2_of agrees with sqrt_rn(r2) < cutoff on every candidate pair (asserted inside build_list), no
    pair of a general cell depends on the last bit of the inverse, rev / pid / pair_ptr have their invariants;
  * the geometry statements against an independent evaluation (mpmath, 40 digits): inside the fp64 term of their bound alone;
  * thirteen mutations of the statement, each of which must change a compared array on a case of the GPU file;
  * the bin-margin search of the cell list: no admitted pair two bins apart inside the range newtonnet_amd/hip.py sends to the cell
    list, lost pairs beyond it (the reason the range is enforced), the smallest separation found per offset decade printed.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import edge_ref as E
from tests import graph_ref as G

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def _round_fraction_to_f32(q):
    """the fp32 number nearest to the rational q, ties to even (q well inside the normal range)"""
    if q == 0:
        return f32(0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = 0
    while q >= 2 ** 24:
        q, e = q / 2, e + 1
    while q < 2 ** 23:
        q, e = q * 2, e - 1
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return f32(sign * float(n) * 2.0 ** e)


def test_fma32_is_exact():
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(3000) * 3).astype(f32)
    b = (rng.standard_normal(3000) * 3).astype(f32)
    c = (rng.standard_normal(3000) * 9).astype(f32)
    # constructed: a b + c exactly on an fp32 midpoint, and a hair off it (the float64 sum then rounds ONTO the midpoint)
    for k in range(0, 600, 3):
        x = f32(1 + rng.integers(1, 2 ** 23) * 2.0 ** -23)
        mid = f64(x) + 2.0 ** -24                                     # midpoint between x and its successor
        a[k], b[k], c[k] = f32(2.0 ** -12), f32(2.0 ** -12), x        # a b = 2^-24: the sum IS the midpoint
        lo, hi = f32(2.0 ** -12 * (1 - 2.0 ** -23)), f32(2.0 ** -12 * (1 + 2.0 ** -23))   # lo hi = 2^-24 (1 - 2^-46): a hair below
        a[k + 1], b[k + 1], c[k + 1] = lo, hi, x
        a[k + 2], b[k + 2], c[k + 2] = -lo, hi, -x
        assert mid > x
    got = G.fma32(a, b, c)
    want = np.array([_round_fraction_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], f32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    naive = (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
    assert (naive != want).any(), 'the constructed inputs do not double-round: the test of the correction is vacuous'


def test_cut2_of_is_the_threshold():
    for c in (5.0, 1.0, 6.3, 0.9, 6.0):
        t = G.cut2_of(c)
        assert np.sqrt(t) >= f32(c) and np.sqrt(np.nextafter(t, f32(0))) < f32(c)


# ---------------------------------------------------------------------------------------------------------------------------
# goldens and the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def test_reproduces_the_boundary_fixture():
    g = G._golden()
    r = float(g['cutoff'])
    B = int(g['a_batch'].max()) + 1
    la = G.build_list(g['a_pos'], np.zeros((B, 9), f32), g['a_batch'], r)
    assert np.array_equal(la.edge_index, g['a_edge_index'])
    assert np.array_equal(la.disp.view(np.int32), g['a_disp'].view(np.int32))
    lb = G.build_list(g['b_pos'], g['b_cell'], g['b_batch'], r)
    assert np.array_equal(lb.edge_index, g['b_edge_index'])
    assert np.abs(lb.disp.astype(f64) - g['b_disp'].astype(f64)).max() <= 2e-6


def _oracle_batch(kind, seed):
    rng = np.random.default_rng(seed)
    sizes = [5, 0, 9, 17, 1]
    if kind == 'none':
        cells = [np.zeros(9, f32)] * 5
    elif kind == 'diagonal':
        cells = [G.diag_cell(11, 12, 13.5)] * 5
    else:
        cells = [G.SHEARED] * 5
    pos = np.concatenate([rng.random((n, 3)) * 12 + rng.integers(-1, 2, (n, 3)) * (0 if kind == 'none' else 12) for n in sizes])
    return pos.astype(f32), np.array(cells, f32), G._batch_of(sizes)


@pytest.mark.parametrize('kind', ['diagonal', 'sheared', 'none'])
def test_equals_the_oracle(kind):
    from oracle import newtonnet_ref as ref
    pos, cell, batch = _oracle_batch(kind, 5)
    mine = G.build_list(pos, cell, batch, 5.0)
    if kind == 'sheared':
        assert mine.tie_share == 0.0
    ei, d = ref.radius_graph(torch.from_numpy(pos), torch.from_numpy(cell.reshape(-1, 3, 3)), torch.from_numpy(batch), 5.0)
    assert mine.E > 40
    assert np.array_equal(mine.edge_index, ei.numpy())
    if kind == 'none':
        assert np.array_equal(mine.disp, d.numpy())
    else:   # (the image shift goes through the oracle's bmm / LU solve: equal up to their summation order, as the fixture's b_disp)
        assert np.abs(mine.disp - d.numpy()).max() <= 2e-6


# ---------------------------------------------------------------------------------------------------------------------------
# invariants on every case of the GPU file
# ---------------------------------------------------------------------------------------------------------------------------
def test_invariants_on_every_gpu_case():
    for name, c in G.gpu_cases().items():
        lst = c.list                                         # (build_list asserts cut2_of == the sqrt predicate on every candidate)
        assert lst.tie_share == 0.0, f'{name}: a pair of a general cell depends on the last bit of the inverse'
        assert np.array_equal(lst.mol_ptr, np.concatenate([[0], np.cumsum(np.bincount(c.batch, minlength=c.B))]))
        Ecount = lst.E
        assert Ecount % 2 == 0 and lst.row_ptr[-1] == Ecount
        e = np.arange(Ecount)
        assert np.array_equal(lst.rev[lst.rev], e), name
        assert np.array_equal(lst.pid, lst.pid[lst.rev]), name
        upper = lst.edge_index[1] > lst.edge_index[0]
        assert np.array_equal(lst.pid[upper], np.arange(Ecount // 2)), f'{name}: pid is not the CSR order of the upper edges'
        assert lst.pair_ptr[-1] == Ecount // 2 and lst.pair_ptr[0] == 0
        assert np.array_equal(np.diff(lst.pair_ptr), np.bincount(lst.edge_index[0][upper], minlength=c.N)[:c.N] if c.N else [])
        for a in range(0, c.N, max(1, c.N // 50)):
            row = lst.col[lst.row_ptr[a]:lst.row_ptr[a + 1]]
            assert (np.diff(row) > 0).all(), f'{name}: row {a} is not ascending'
        assert np.array_equal(lst.disp, -lst.disp[lst.rev]) or (G.cell_kind(c.cell) != 0).any()
        assert G.status_bits(c.batch, c.B, c.z) in (0, 8)


def test_cases_reach_the_branches_they_are_there_for():
    cs = G.gpu_cases()
    deg = {k: np.diff(c.list.row_ptr) for k, c in cs.items()}
    assert deg['full'].max() == 65 and 64 in deg['full']                       # degree 64 and 65: one and two ballot chunks
    assert cs['full64'].list.E == 4032 <= G.MG_LDS_EDGES < cs['full65'].list.E == 4160
    assert (deg['cells257'] == G.CW_CAP).sum() > 100 and deg['cells257'].max() >= G.CW_CAP   # the rank sort at its full list
    assert (deg['cells258'] > G.CW_CAP).sum() >= 258                            # the serial form
    for n in (257, 258):
        c = cs[f'cells{n}']
        assert 0 in deg[c.name]
        near, b, nb = G.cells_candidates(c, c.box)
        assert list(nb) == [3, 4, 5]
        flat = (b[:, 0] * nb[1] + b[:, 1]) * nb[2] + b[:, 2]
        assert np.bincount(flat).max() > 64
        i, j = c.list.edge_index
        assert near[i, j].all(), 'the real grid loses an edge of the statement'
        assert G.eligible(c.box, c.cutoff, c.pos)
        below = c.box.copy()
        below[0] = np.nextafter(below[0], f32(0))
        assert not G.eligible(below, c.cutoff)
        for axis in range(3):
            L = c.box[axis]
            col = c.pos[:, axis]
            for v in (f32(0.0), L, np.nextafter(L, f32(0))):
                assert (col == v).any()
            assert (np.signbit(col) & (col == 0)).any() and (col < 0).any()
        assert np.abs(c.pos).max() > 0.85 * G.CELL_LIST_MAX_COORD * c.cutoff     # displaced out to the limit
    c0, pos1, cut = G.reuse_inputs()
    d, r2, _ = G.disp_of_edges(pos1, c0.cell, c0.batch, c0.list.edge_index)
    c2 = G.cut2_of(cut)
    assert (r2 == c2).any() and (r2 == np.nextafter(c2, f32(0))).any() and (r2 == np.nextafter(c2, f32(np.inf))).any()
    geo = G.edge_geometry(d, cut)
    x = geo['x'].astype(f64)
    live = ~geo['masked']
    assert (x[live] < 1.1e-3).any() and ((1 - x[live] < 1e-6) & (x[live] < 1)).any() and geo['masked'].any() and live.any()
    assert geo['grid_distance'][live].min() >= 1e-9
    row_masked = np.array([geo['masked'][c0.list.row_ptr[a]:c0.list.row_ptr[a + 1]].all() and c0.list.row_ptr[a + 1] > c0.list.row_ptr[a]
                           for a in range(c0.N)])
    assert row_masked.any()                                                     # a whole row outside
    for c in cs.values():
        if c.name.startswith('reuse'):
            continue
        g = G.edge_geometry(c.list.disp, c.cutoff)
        assert not g['masked'].any(), 'an edge of the exact list is never masked'
        assert g['grid_distance'].min(initial=1.0) >= 1e-9, c.name


def test_eligibility_is_what_the_wrapper_enforces():
    from newtonnet_amd import hip
    assert hip.CELL_LIST_MAX_COORD == G.CELL_LIST_MAX_COORD
    for cutoff in (5.0, 0.9, 1.0, 6.3):
        t = f32(3.0003 * cutoff)
        for k in range(-6, 7):
            L = t
            for _ in range(abs(k)):
                L = np.nextafter(L, f32(np.inf if k > 0 else -np.inf))
            for box in ([L, 4 * L, 5 * L], [4 * L, L, 4 * L], [L, L, f32(2 * G.CELL_LIST_MAX_COORD * cutoff * 1.001)]):
                got = hip._orthorhombic_box(None, cutoff, cell_host=np.diag(np.array(box, f32))) is not None
                assert got == G.eligible(box, cutoff), (cutoff, k, box)
                if got:      # whatever the wrapper accepts, make_grid accepts (else the route would raise instead of falling back)
                    assert G.make_grid32(box, cutoff) is not None
    pos = torch.tensor([[1.0, -639.0, 2.0]])
    assert hip._cell_list_in_range(pos, 5.0) and not hip._cell_list_in_range(pos * 1.01, 5.0)


# ---------------------------------------------------------------------------------------------------------------------------
# geometry against mpmath
# ---------------------------------------------------------------------------------------------------------------------------
def test_geometry_statement_against_an_independent_evaluation():
    mp = pytest.importorskip('mpmath') if False else __import__('mpmath')
    mp.mp.dps = 40
    c0, pos1, cut = G.reuse_inputs()
    d, _, _ = G.disp_of_edges(pos1, c0.cell, c0.batch, c0.list.edge_index)
    pick = np.unique(np.concatenate([np.arange(0, len(d), 7), np.arange(len(d) - 40, len(d))]))
    d = d[pick]
    freq = (np.arange(1, 6) * np.pi).astype(f32)
    freq = np.concatenate([freq, (np.array([20, 32]) * np.pi).astype(f32)])
    for env in (9, 6, G.COSINE):
        out = G.edge_geometry(d, cut, freq, env)
        worst = {'rbf': 0.0, 'drbf': 0.0, 'geo': 0.0, 'frac': 0.0}
        for e in range(len(d)):
            v = [mp.mpf(float(t)) for t in d[e]]
            r = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
            x = r / mp.mpf(float(f32(cut)))
            for k in range(3):
                worst['geo'] = max(worst['geo'], abs(float(mp.mpf(float(out['geo'][0][e, k])) - v[k] / r)) / 2.0 ** -53)
            worst['geo'] = max(worst['geo'], abs(float(mp.mpf(float(out['geo'][0][e, 3])) - r)) / (2.0 ** -53 * float(r)))
            if out['masked'][e]:
                assert not out['rbf'][0][e].any() and not out['drbf'][0][e].any() and not out['rbf'][1][e].any()
                continue
            t = x * G.FT_G
            g0 = min(max(int(mp.floor(t)), 0), G.FT_G - 1)
            assert out['xg_index'][e] == g0
            worst['frac'] = max(worst['frac'], abs(float(mp.mpf(float(out['xg_frac'][0][e])) - (t - g0))) / (G.FT_G * 2.0 ** -52))
            if env == G.COSINE:
                en, den = (1 + mp.cos(mp.pi * x)) / 2, -mp.pi / 2 * mp.sin(mp.pi * x)
            else:
                p = env
                en = 1 - mp.mpf((p + 1) * (p + 2)) / 2 * x ** p + p * (p + 2) * x ** (p + 1) - mp.mpf(p * (p + 1)) / 2 * x ** (p + 2)
                den = -mp.mpf(p * (p + 1) * (p + 2)) / 2 * x ** (p - 1) * (1 - x) ** 2
            for n, w in enumerate(freq):
                w = mp.mpf(float(w))
                bes = mp.sin(w * x) / x
                dbes = (w * mp.cos(w * x) - bes) / x
                for name, val in (('rbf', en * bes), ('drbf', den * bes + en * dbes)):
                    err = abs(float(mp.mpf(float(out[name][0][e, n])) - val))
                    worst[name] = max(worst[name], err / out['fp64_term'][name][e, n])
        print(f'GRAPH-STATEMENT envelope {env}: statement - mpmath, in units of the fp64 term of the bound: {worst}')
        assert worst['rbf'] <= 1 and worst['drbf'] <= 1 and worst['frac'] <= 1 and worst['geo'] <= 1


# ---------------------------------------------------------------------------------------------------------------------------
# mutations of the statement: each must change a compared array on a case of the GPU file
# ---------------------------------------------------------------------------------------------------------------------------
def _rules(**kw):
    return type('Mutated', (G.Rules,), kw)


def _list_differs(a, b):
    return (a.E != b.E or not np.array_equal(a.col, b.col) or not np.array_equal(a.disp.view(np.int32), b.disp.view(np.int32))
            or not np.array_equal(a.row_ptr, b.row_ptr))


def _mut_rules(case_names, **kw):
    cs = G.gpu_cases()
    return any(_list_differs(G.build_list(cs[n].pos, cs[n].cell, cs[n].batch, cs[n].cutoff, rules=_rules(**kw)), cs[n].list)
               for n in case_names)


def _mut_bin_order():
    c = G.gpu_cases()['cells257']
    _, b, nb = G.cells_candidates(c, c.box)
    flat = (b[:, 0] * nb[1] + b[:, 1]) * nb[2] + b[:, 2]
    m = G.build_list(c.pos, c.cell, c.batch, c.cutoff, order=lambda a, js: np.lexsort((js, flat[js])))
    return not np.array_equal(m.col, c.list.col) and np.array_equal(np.sort(m.col), np.sort(c.list.col))


def _mut_rev():
    lst = G.gpu_cases()['sizes'].list
    rev = lst.rev.copy()
    a = int(np.flatnonzero(np.diff(lst.row_ptr) >= 2)[0])
    s, e = lst.row_ptr[a], lst.row_ptr[a + 1]
    rev[s:e] = np.roll(rev[s:e], 1)
    return not np.array_equal(rev, lst.rev)


def _mut_pid_upper_row():
    lst = G.gpu_cases()['mol sizes'].list
    lower = lst.edge_index[1] < lst.edge_index[0]
    pid = np.zeros(lst.E, np.int32)
    pid[lower] = np.arange(lst.E // 2)                      # numbered where the UPPER endpoint's row meets the pair
    pid[~lower] = pid[lst.rev[~lower]]
    return not np.array_equal(pid, lst.pid)


def _mut_pair_ptr_inclusive():
    lst = G.gpu_cases()['sizes'].list
    return not np.array_equal(np.concatenate([lst.pair_ptr[1:], lst.pair_ptr[-1:]]), lst.pair_ptr)


def _mut_empty_slot():
    c = G.gpu_cases()['sizes']
    sizes = np.bincount(c.batch, minlength=c.B)
    mp = c.list.mol_ptr.copy()
    mp[:-1][sizes == 0] = 0                                  # (what graph_init_kernel left there)
    return not np.array_equal(mp, c.list.mol_ptr)


def _mut_mask_fp64():
    c0, pos1, cut = G.reuse_inputs()
    d, _, _ = G.disp_of_edges(pos1, c0.cell, c0.batch, c0.list.edge_index)
    return not np.array_equal(G.edge_geometry(d, cut)['xg_index'], G.edge_geometry(d, cut, mask_rule='fp64')['xg_index'])


def _mut_geo_fp32_inverse():
    lst = G.gpu_cases()['sizes'].list
    ref, B = G.edge_geometry(lst.disp, 5.0)['geo']
    d = lst.disp
    r = np.sqrt(d.astype(f64) ** 2 @ np.ones(3)).astype(f32)
    wrong = d * (f32(1) / r)[:, None]
    return bool((np.abs(wrong.astype(f64) - ref[:, :3].astype(f64)) > B[:, :3]).any())


def _mut_bins_one_cutoff_wide():
    c = G.gpu_cases()['cells258']
    near, _, nb = G.cells_candidates(c, c.box, factor=f32(1))
    i, j = c.list.edge_index
    return list(nb) == [3, 5, 5] and bool((~near[i, j]).any())


TIES = ('ties5', 'ties1', 'ties6.3')
MUTATIONS = {
    '<= in place of <': lambda: _mut_rules(TIES, strict=False),
    'plain (x^2 + y^2) + z^2': lambda: _mut_rules(('boundary a',), fused=False),
    'product with a rounded 1/L': lambda: _mut_rules(TIES + ('boundary b diagonal',), divide=False),
    'round half away': lambda: _mut_rules(TIES, half_even=False),
    'cut2 = cutoff^2': lambda: _mut_rules(TIES, cut2_exact=False),
    'bin-visit order': _mut_bin_order,
    'rev off by one in a row': _mut_rev,
    'pid from the upper endpoint row': _mut_pid_upper_row,
    'pair_ptr inclusive': _mut_pair_ptr_inclusive,
    'empty slot not propagated': _mut_empty_slot,
    'xg masked by fp64 x >= 1': _mut_mask_fp64,
    'geo from an fp32 1/r': _mut_geo_fp32_inverse,
    'bins exactly one cutoff wide': _mut_bins_one_cutoff_wide,
}


@pytest.mark.parametrize('name', list(MUTATIONS))
def test_mutation_is_detected(name):
    assert MUTATIONS[name](), f'no case of the GPU file tells "{name}" from the statement: an input is missing'


# ---------------------------------------------------------------------------------------------------------------------------
# the cell list's margin
# ---------------------------------------------------------------------------------------------------------------------------
def _threshold_box(nb, cutoff):
    """the smallest float L whose grid has nb bins"""
    L = f32(nb * cutoff * 1.0001)
    while int(G.make_grid32([L, L, L], cutoff)[0][0]) >= nb:
        L = np.nextafter(L, f32(0))
    return np.nextafter(L, f32(np.inf))


def test_bin_margin_search():
    """Boxes at and just above the threshold of 4 .. 100 bins, cutoff 5; offsets out to 10^4 box lengths (MD positions are unwrapped:
    there is no largest offset the front end can feed).  Inside the enforced range (|p| <= 128 cutoffs, L <= 256 cutoffs) every
    offset is searched, same image, neighbouring images and opposite ends of the range; no admitted pair two bins apart may exist."""
    cutoff = 5.0
    P = G.CELL_LIST_MAX_COORD * cutoff
    boxes = [_threshold_box(nb, cutoff) for nb in (4, 5, 10, 20, 50, 100)]
    boxes += [np.nextafter(np.nextafter(b, f32(np.inf)), f32(np.inf)) for b in boxes[:3]] + [f32(v) for v in (50.0052, 100.0102, 250.0252, 500.0502)]
    inside_best, beyond_lost, report = np.inf, 0, {}
    for L in boxes:
        nb = int(G.make_grid32([L, L, L], cutoff)[0][0])
        bd = None if nb <= 10 else [0, 1, nb // 2, nb - 2, nb - 1]
        kmax = int(P / float(L)) - 2
        ks = list(range(-kmax, kmax + 1)) if kmax >= 0 else []
        for other in (ks, [k + 1 for k in ks], [-k for k in ks]):
            if ks:
                best, lost = G.margin_search(L, cutoff, ks, other, boundaries=bd)
                inside_best = min(inside_best, best)
                assert not lost, f'L = {L}: the cell list would lose {lost[:3]} inside the supported range'
        for decade in (2, 3, 4):
            ks = [k for k in (10 ** decade // 4, 10 ** decade // 2, 10 ** decade) if (k - 2) * float(L) > P]
            if not ks:
                continue
            for other in (ks, [k + 1 for k in ks]):
                best, lost = G.margin_search(L, cutoff, ks + [-k for k in ks], other + [-k for k in other], boundaries=bd)
                key = (float(L), decade)
                report[key] = min(report.get(key, np.inf), best)
                beyond_lost += len(lost)
    print(f'GRAPH-MARGIN inside |p| <= {P:g}: smallest |dx| two bins apart = {inside_best!r} (cutoff {cutoff})')
    for (L, decade), best in sorted(report.items()):
        print(f'GRAPH-MARGIN L = {L:.4f}, offsets of 10^{decade} box lengths: smallest |dx| two bins apart = {best!r}'
              + ('  LOST' if best < cutoff else ''))
    assert inside_best > cutoff, 'no margin left inside the supported range'
    assert beyond_lost > 0, 'the search finds no lost pair at any offset: the range limit would be unfounded'


def test_margin_analysis_constants():
    """the inequality next to CELL_LIST_MAX_COORD"""
    P = G.CELL_LIST_MAX_COORD
    margin = float(G.BIN_FACTOR) * (1 - 2.0 ** -22) - 1
    assert 2.0 ** -23 * (4 * P + 2 * P) < margin
