"""The last stage of "tangent over reverse" -- the six kernels of csrc/hessian.hip and the two strain kernels at the head of
csrc/elastic.hip -- each called DIRECTLY through its stage entry point (nnhip_hvp_dgu, nnhip_hvp_dgx, nnhip_hvp_out, nnhip_hess_dirs,
nnhip_hess_scatter, nnhip_strain_tan_geom, nnhip_strain_born) on planted inputs and compared element by element with its float64
statement and componentwise bound (tests/hvp_ref.py).

The harness is that of tests/test_hip_edge_stages.py: every output starts as a sentinel NaN and has 8 guard rows behind it that
must come back bit-identical; every case runs twice and must repeat bit for bit; |got - ref| <= bound element by element (a
bound of 0 -- masked candidates, the other direction of a pair, edges from the cutoff on, fourth components, rows of degree 0 --
wants the exact value); the largest ratio per stage output is printed as a `STAGE-RATIO` line per case and summed up by
test_zz_ratio_summary.  The cases are those of hvp_ref (DGU_CASES, DGX_CASES, OUT_CASES, ...), the ones tests/test_hvp_ref_host.py
holds the fp32 restatements to.

Shapes: hvp_dgu takes 4 rows per block (3, 4, 5, 33 rows; rows of degree 0, 65, 130); hvp_dgx covers 8192 edges in one trip of
its grid (the complete graph of 96 atoms has 9120); hvp_geom / hvp_rows / strain_tan_geom take 256 lanes per block (255, 256, 257);
strain_born strides a system's atoms by 64 lanes (63, 64, 65, 130 atoms)."""
import numpy as np
import pytest
import torch

from tests import edge_ref as R
from tests import hessian_ref
from tests import hvp_ref as H
from tests.test_hip_dense_stages import GUARD, OK, SENT, _stop_after_a_gpu_fault  # noqa: F401  (the fixture is autouse here too)
from tests.test_hip_edge_stages import DevGraph, bits, blank, ptr, run_twice, tin

pytestmark = pytest.mark.gpu

F = R.F
E_INVALID, E_UNSUPPORTED = 1, 2
RATIOS = {}
_CACHE = {}


def _hip():
    from newtonnet_amd import hip
    return hip


def _lib():
    return _hip().lib()


def _stream():
    return _hip()._stream(torch.device('cuda', 0))


def record(stage, what, got, ref):
    """got (a device tensor cut to its rows) against (value, bound, defined): every entry written, finite and within its bound"""
    g = got.detach().cpu().double().numpy().reshape(ref[0].shape)
    assert np.isfinite(g).all(), f'{stage} {what}: {int((~np.isfinite(g)).sum())} elements not written / not finite'
    worst = H.ratio(g, ref)
    RATIOS[stage] = max(RATIOS.get(stage, 0.0), worst)
    print(f'STAGE-RATIO {stage} {what}: {worst:.3f}')
    if worst > 1.0:
        val, B, _ = ref
        err = np.abs(g - val)
        rat = np.where(B > 0, err / np.where(B > 0, B, 1.0), np.where(err > 0, np.inf, 0.0))
        k = np.unravel_index(int(rat.argmax()), rat.shape)
        raise AssertionError(f'{stage} {what}: |got - ref| / bound = {worst:.3g} at {k} (got {g[k]!r}, ref {val[k]!r}, bound {B[k]:.3g}); '
                             f'{int((rat > 1).sum())} of {rat.size} elements outside')
    return g


def dev(g):
    if id(g) not in _CACHE:
        _CACHE[id(g)] = (g, DevGraph(g))          # (the graph is kept alive with its device copy)
    return _CACHE[id(g)][1]


def refused(what, shapes, call, rc_want=E_INVALID):
    """the call is refused with all pointers valid and every buffer keeps the sentinel"""
    bufs = {k: blank(r, w) for k, (r, w) in shapes.items()}
    rc = call(bufs)
    torch.cuda.synchronize()
    assert rc == rc_want, (what, rc, _lib().nnhip_last_error())
    for k, b in bufs.items():
        assert bool((bits(b) == SENT).all()), f'{what}: {k} was written by a refused call'


def nothing(what, shapes, call):
    refused(what, shapes, call, OK)


# ---------------------------------------------------------------------------------------------------------------------------
# hvp_dgu
# ---------------------------------------------------------------------------------------------------------------------------
def _dgu_call(g, t, use_mask, n=None, **null):
    dg = dev(g)
    a = dict(gf=ptr(t['gf']), dgf=ptr(t['dgf']), phi1=ptr(t['phi1']), dphi1=ptr(t['dphi1']), row_ptr=ptr(dg.row_ptr), pid=ptr(dg.pid))
    a.update(null)
    return lambda b: _lib().nnhip_hvp_dgu(a['gf'], a['dgf'], a['phi1'], a['dphi1'], a['row_ptr'], a['pid'],
                                          ptr(dg.xg) if use_mask else None, g.N if n is None else n,
                                          None if null.get('dg_u', 1) is None else ptr(b['dg_u']), _stream())


@pytest.mark.parametrize('name,use_mask', H.DGU_CASES, ids=[f'{n}{"" if m else ", xg NULL"}' for n, m in H.DGU_CASES])
def test_hvp_dgu(name, use_mask):
    g, d = H.dgu_inputs(name)
    t = {k: tin(v) for k, v in d.items()}
    out = run_twice(f'hvp_dgu {name}', {'dg_u': (g.E, 4)}, _dgu_call(g, t, use_mask))
    got = record('hvp_dgu dg_u', f'{name}{"" if use_mask else ", xg NULL"}', out['dg_u'], H.hvp_dgu(g, **d, use_mask=use_mask)['dg_u'])
    assert not got[:, 3].any()
    if use_mask and g.masked.any():
        assert not got[g.masked].any(), 'a masked candidate carries a tangent'
    if name == 'masked' and not use_mask:
        assert got[g.masked][:, :3].all(), 'xg NULL: nothing is masked'


def test_hvp_dgu_refusals_and_zero_sizes():
    g, d = H.dgu_inputs('chain 5')
    t = {k: tin(v) for k, v in d.items()}
    shapes = {'dg_u': (g.E, 4)}
    refused('hvp_dgu n < 0', shapes, _dgu_call(g, t, True, n=-1))
    for k in ('gf', 'dgf', 'phi1', 'dphi1', 'row_ptr', 'pid', 'dg_u'):
        refused(f'hvp_dgu {k} NULL', shapes, _dgu_call(g, t, True, **{k: None}))
    nothing('hvp_dgu n = 0', shapes, _dgu_call(g, t, True, n=0))
    nothing('hvp_dgu n = 0, NULL', shapes, _dgu_call(g, t, True, n=0, gf=None, row_ptr=None))


# ---------------------------------------------------------------------------------------------------------------------------
# hvp_dgx
# ---------------------------------------------------------------------------------------------------------------------------
def _dgx_call(g, t, nb, env, use_mask, n=None, cutoff=None, **null):
    dg = dev(g)
    pid = t['pid'] if 'pid' in t else dg.pid
    a = dict(edge_index=ptr(dg.edge_index), pid=ptr(pid), geo=ptr(t['geo']), tgeo=ptr(t['tgeo']), g_eps=ptr(t['g_eps']),
             dg_eps=ptr(t['dg_eps']), W=ptr(t['W']), freq=ptr(t['freq']))
    a.update(null)
    return lambda b: _lib().nnhip_hvp_dgx(a['edge_index'], a['pid'], a['geo'], a['tgeo'], ptr(dg.xg) if use_mask else None, a['g_eps'],
                                          a['dg_eps'], a['W'], a['freq'], nb, env, g.cutoff if cutoff is None else cutoff,
                                          g.E if n is None else n, None if null.get('dg_x', 1) is None else ptr(b['dg_x']), _stream())


def _dgx_tensors(g, d):
    t = {k: tin(v) for k, v in d.items()}
    t['geo'] = tin(g.geo)
    t['pid'] = tin(g.pid, torch.int32)
    return t


def _dgx_id(c):
    name, nb, env, use_mask, own_rows = c
    return f'{name}, nb {nb}, env {env}' + ('' if use_mask else ', xg NULL') + (', own rows' if own_rows else '')


@pytest.mark.parametrize('case', H.DGX_CASES, ids=[_dgx_id(c) for c in H.DGX_CASES])
def test_hvp_dgx(case):
    name, nb, env, use_mask, own_rows = case
    g, d = H.dgx_inputs(name, nb, own_rows)
    t = _dgx_tensors(g, d)
    out = run_twice(f'hvp_dgx {_dgx_id(case)}', {'dg_x': (g.E, 1)}, _dgx_call(g, t, nb, env, use_mask))
    ref = H.hvp_dgx(g, d['tgeo'], d['g_eps'], d['dg_eps'], d['W'], d['freq'], env, use_mask=use_mask)['dg_x']
    got = record('hvp_dgx dg_x', _dgx_id(case), out['dg_x'], ref)
    assert not got[~(g.i < g.j)].any(), 'the other direction of a pair carries dg_x'
    if name == 'edges':                         # the planted distances: x = 0.02, the last r inside, the first outside
        x, own = H.x_of(g), np.flatnonzero(g.i < g.j)
        inside = own[(x[own] < 1.0) & (x[own] > 1.0 - 1e-6)]
        outside = own[x[own] >= 1.0]
        assert inside.size == 2 and outside.size == 2 and (np.abs(x[own] - 0.02) < 1e-6).sum() == 2
        assert not got[outside].any() and got[inside].all(), 'the cutoff predicate x < 1 is taken on another side'
    if env == 0:                                # envelope 0 means PolynomialCutoff(9): bit for bit
        nine = run_twice('hvp_dgx env 9', {'dg_x': (g.E, 1)}, _dgx_call(g, t, nb, 9, use_mask))
        assert torch.equal(bits(out['dg_x']), bits(nine['dg_x']))


def test_hvp_dgx_refusals_and_zero_sizes():
    g, d = H.dgx_inputs('degrees', 20, False)
    t = _dgx_tensors(g, d)
    shapes = {'dg_x': (g.E, 1)}
    for nb in (0, H.MAX_NB + 1, -1):
        refused(f'hvp_dgx n_basis {nb}', shapes, _dgx_call(g, t, nb, 9, True), E_UNSUPPORTED)
    refused('hvp_dgx n < 0', shapes, _dgx_call(g, t, 20, 9, True, n=-1))
    refused('hvp_dgx cutoff 0', shapes, _dgx_call(g, t, 20, 9, True, cutoff=0.0))
    refused('hvp_dgx cutoff < 0', shapes, _dgx_call(g, t, 20, 9, True, cutoff=-5.0))
    refused('hvp_dgx envelope -2', shapes, _dgx_call(g, t, 20, -2, True))
    for k in ('edge_index', 'pid', 'geo', 'tgeo', 'g_eps', 'dg_eps', 'W', 'freq', 'dg_x'):
        refused(f'hvp_dgx {k} NULL', shapes, _dgx_call(g, t, 20, 9, True, **{k: None}))
    nothing('hvp_dgx n = 0', shapes, _dgx_call(g, t, 20, 9, True, n=0))


# ---------------------------------------------------------------------------------------------------------------------------
# hvp_out
# ---------------------------------------------------------------------------------------------------------------------------
def _out_call(g, t, L, n=None, e=None, cutoff=None, **null):
    a = {k: ptr(v) for k, v in t.items()}
    a.update(null)
    return lambda b: _lib().nnhip_hvp_out(a['g_x'], a['g_u'], a['dg_x'], a['dg_u'], a['geo'], a['tgeo'], a['row_ptr'], a['rev'],
                                          g.N if n is None else n, g.E if e is None else e, L, g.cutoff if cutoff is None else cutoff,
                                          None if null.get('dg_d', 1) is None else ptr(b['dg_d']),
                                          None if null.get('hv', 1) is None else ptr(b['hv']), _stream())


def _out_tensors(g, d):
    t = {k: tin(v) for k, v in d.items()}
    t.update(geo=tin(g.geo), row_ptr=tin(g.row_ptr, torch.int32), rev=tin(g.rev, torch.int32))
    return t


@pytest.mark.parametrize('name,L', H.OUT_CASES, ids=[f'{n}, {L} layers' for n, L in H.OUT_CASES])
def test_hvp_out(name, L):
    g, d = H.out_inputs(name, L)
    t = _out_tensors(g, d)
    out = run_twice(f'hvp_out {name}', {'dg_d': (g.E, 4), 'hv': (g.N, 3)}, _out_call(g, t, L))
    ref = H.hvp_out(g, **d)
    gd = record('hvp_out dg_d', f'{name}, {L} layers', out['dg_d'], ref['dg_d'])
    hv = record('hvp_out hv', f'{name}, {L} layers', out['hv'], ref['hv'])
    assert not gd[:, 3].any()
    empty = np.diff(g.row_ptr) == 0
    assert empty.any() or name in ('wide row', 'short edge'), 'the case has a row of degree 0'
    assert not hv[empty].any()
    if name == 'short edge':                    # the short edge's bound is its own: 1/r^2 = 400 against 0.04
        B = ref['dg_d'][1][:, :3].max(axis=1)
        assert B[5] > 100 * np.delete(B, 5).max()


def test_hvp_out_refusals_and_zero_sizes():
    g, d = H.out_inputs('short edge', 3)
    t = _out_tensors(g, d)
    shapes = {'dg_d': (g.E, 4), 'hv': (g.N, 3)}
    for L in (0, H.MAX_LAYERS + 1, -1):
        refused(f'hvp_out n_layers {L}', shapes, _out_call(g, t, L))
    refused('hvp_out n_atoms < 0', shapes, _out_call(g, t, 3, n=-1))
    refused('hvp_out n_edges < 0', shapes, _out_call(g, t, 3, e=-1))
    refused('hvp_out edges without atoms', shapes, _out_call(g, t, 3, n=0))
    refused('hvp_out cutoff 0', shapes, _out_call(g, t, 3, cutoff=0.0))
    for k in ('g_x', 'g_u', 'dg_x', 'dg_u', 'geo', 'tgeo', 'row_ptr', 'rev', 'dg_d', 'hv'):
        refused(f'hvp_out {k} NULL', shapes, _out_call(g, t, 3, **{k: None}))
    nothing('hvp_out 0 atoms, 0 edges', shapes, _out_call(g, t, 3, n=0, e=0))
    # atoms without edges: every hv row is written as 0, dg_d is left alone
    g0 = R.graph_trivial(5)
    t0 = dict(t, row_ptr=tin(g0.row_ptr, torch.int32))
    out = run_twice('hvp_out 5 atoms, 0 edges', {'dg_d': (0, 4), 'hv': (5, 3)}, _out_call(g0, t0, 3))
    assert not out['hv'].any()


# ---------------------------------------------------------------------------------------------------------------------------
# hess_dirs / hess_scatter
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_rep', H.HESS_REPS)
def test_hess_dirs_and_scatter(n_rep):
    L = _lib()
    batch, mol_ptr, blk_ptr, n_mol0, n_blk = H.hess_inputs(n_rep)
    n = batch.size
    tb, tm, tp = tin(batch, torch.int64), tin(mol_ptr, torch.int32), tin(blk_ptr, torch.int64)
    n_dirs = 3 * max(H.HESS_SIZES)
    passes, live_last = hessian_ref.pass_count(n_dirs, n_rep)
    assert (passes - 1) * n_rep + live_last == n_dirs
    written = np.zeros(n_blk, np.int64)
    for k in range(passes + 1):                 # one pass more than needed: every dir >= 3 n_b, nothing is written
        out = run_twice(f'hess_dirs pass {k}', {'v': (n, 3)}, lambda b: L.nnhip_hess_dirs(ptr(tb), ptr(tm), n, k, n_rep, n_mol0, ptr(b['v']),
                                                                                          _stream()))
        v = H.hess_dirs(batch, mol_ptr, k, n_rep, n_mol0)
        assert np.array_equal(out['v'].cpu().numpy(), v), f'hess_dirs pass {k}'
        hv = H.hess_hv(n, k)
        thv = tin(hv)
        out = run_twice(f'hess_scatter pass {k}', {'blocks': (n_blk, 1)},
                        lambda b: L.nnhip_hess_scatter(ptr(thv), ptr(tb), ptr(tm), ptr(tp), n, k, n_rep, n_mol0, ptr(b['blocks']), _stream()))
        idx, val = H.hess_scatter(hv, batch, mol_ptr, blk_ptr, k, n_rep, n_mol0)
        want = np.full(n_blk, SENT, np.int32)
        want[idx] = val.view(np.int32)
        assert np.array_equal(bits(out['blocks']).cpu().numpy().reshape(-1), want), f'hess_scatter pass {k}'
        assert idx.size == 3 * int(((k * n_rep + batch // n_mol0) < 3 * np.diff(mol_ptr)[batch]).sum())     # every live atom's column
        np.add.at(written, idx, 1)
        if k == passes:
            assert idx.size == 0 and not v.any(), 'a pass beyond 3 n_b of every molecule writes'
    assert (written == 1).all(), 'after all passes every block element is written exactly once'
    RATIOS['hess_dirs / hess_scatter (exact)'] = 0.0


def test_hess_refusals_and_zero_sizes():
    L = _lib()
    batch, mol_ptr, blk_ptr, n_mol0, n_blk = H.hess_inputs(2)
    n = batch.size
    tb, tm, tp, thv = tin(batch, torch.int64), tin(mol_ptr, torch.int32), tin(blk_ptr, torch.int64), tin(H.hess_hv(n, 0))
    dirs = lambda n_=n, k=0, rep=2, mol0=n_mol0, batch_=tb, mol=tm, v=1: lambda b: L.nnhip_hess_dirs(  # noqa: E731
        ptr(batch_), ptr(mol), n_, k, rep, mol0, ptr(b['v']) if v else None, _stream())
    scat = lambda n_=n, k=0, rep=2, mol0=n_mol0, hv=thv, batch_=tb, mol=tm, blk=tp, out=1: lambda b: L.nnhip_hess_scatter(  # noqa: E731
        ptr(hv), ptr(batch_), ptr(mol), ptr(blk), n_, k, rep, mol0, ptr(b['blocks']) if out else None, _stream())
    sv, sb = {'v': (n, 3)}, {'blocks': (n_blk, 1)}
    for what, kw in (('n < 0', dict(n_=-1)), ('k < 0', dict(k=-1)), ('n_rep 0', dict(rep=0)), ('n_rep < 0', dict(rep=-2)),
                     ('n_mol0 0', dict(mol0=0)), ('n_mol0 < 0', dict(mol0=-1)), ('batch NULL', dict(batch_=None)), ('mol_ptr NULL', dict(mol=None))):
        refused(f'hess_dirs {what}', sv, dirs(**kw))
        refused(f'hess_scatter {what}', sb, scat(**kw))
    refused('hess_dirs v NULL', sv, dirs(v=0))
    refused('hess_scatter hv NULL', sb, scat(hv=None))
    refused('hess_scatter blk_ptr NULL', sb, scat(blk=None))
    refused('hess_scatter blocks NULL', sb, scat(out=0))
    nothing('hess_dirs n = 0', sv, dirs(n_=0))
    nothing('hess_scatter n = 0', sb, scat(n_=0))


# ---------------------------------------------------------------------------------------------------------------------------
# strain_tan_geom / strain_born
# ---------------------------------------------------------------------------------------------------------------------------
def _strain_tensors():
    if 'strain' not in _CACHE:
        g, batch, eta6 = H.strain_inputs()
        _CACHE['strain'] = (g, batch, eta6, dict(edge_index=tin(g.edge_index, torch.int64), batch=tin(batch, torch.int64), geo=tin(g.geo),
                                                 eta6=tin(eta6)))
    return _CACHE['strain']


def _strain_call(g, t, n, cutoff=None, **null):
    a = {k: ptr(v) for k, v in t.items()}
    a.update(null)
    return lambda b: _lib().nnhip_strain_tan_geom(a['edge_index'], a['batch'], a['geo'], a['eta6'], n, g.cutoff if cutoff is None else cutoff,
                                                  None if null.get('tgeo', 1) is None else ptr(b['tgeo']), _stream())


@pytest.mark.parametrize('n_edges', H.STRAIN_EDGES, ids=[f'E = {n or "all"}' for n in H.STRAIN_EDGES])
def test_strain_tan_geom(n_edges):
    g, batch, eta6, t = _strain_tensors()
    assert t['batch'].dtype == torch.int64 and not eta6[2].any() and not eta6[1, :3].any() and eta6[1, 3:].all()
    n = g.E if n_edges is None else n_edges
    out = run_twice(f'strain_tan_geom {n}', {'tgeo': (n, 4)}, _strain_call(g, t, n))
    ref = H.strain_tan_geom(g, batch, eta6, n_edges)['tgeo']
    got = record('strain_tan_geom tgeo', f'E = {n}', out['tgeo'], ref)
    sys_of = batch[g.i[:n]]
    assert not got[sys_of == 2].any(), 'no strain, no tangent'
    if n > 1:
        assert set(sys_of) == {0, 1, 2}


def test_strain_tan_geom_refusals_and_zero_sizes():
    g, batch, eta6, t = _strain_tensors()
    shapes = {'tgeo': (g.E, 4)}
    refused('strain_tan_geom n < 0', shapes, _strain_call(g, t, -1))
    refused('strain_tan_geom cutoff 0', shapes, _strain_call(g, t, g.E, cutoff=0.0))
    for k in ('edge_index', 'batch', 'geo', 'eta6', 'tgeo'):
        refused(f'strain_tan_geom {k} NULL', shapes, _strain_call(g, t, g.E, **{k: None}))
    nothing('strain_tan_geom n = 0', shapes, _strain_call(g, t, 0))


def _born_call(t, n_mol, **null):
    a = {k: ptr(v) for k, v in t.items()}
    a.update(null)
    return lambda b: _lib().nnhip_strain_born(a['dg_d'], a['geo'], a['row_ptr'], a['mol_ptr'], n_mol,
                                              None if null.get('d2', 1) is None else ptr(b['d2']), _stream())


def _born(swap):
    g, dg_d, geo = H.born_inputs(swap)
    t = dict(dg_d=tin(dg_d), geo=tin(geo), row_ptr=tin(g.row_ptr, torch.int32), mol_ptr=tin(g.mol_ptr, torch.int32))
    out = run_twice(f'strain_born swap={swap}', {'d2': (g.B, 6)}, _born_call(t, g.B))
    ref = H.strain_born(dg_d, geo, g.row_ptr, g.mol_ptr)['d2']
    record('strain_born d2', 'swapped x, y' if swap else 'systems of 0, 1, 63, 64, 65, 130 atoms', out['d2'], ref)
    return g, t, out['d2'].cpu()


def test_strain_born():
    g, t, d2 = _born(False)
    assert tuple(np.diff(g.mol_ptr)) == H.BORN_SIZES and (np.diff(g.row_ptr) == 0).sum() > 20
    assert not d2[:2].any(), 'a system without atoms or without edges has no strain derivative'
    # x <-> y in dg_d and u exchanges S_01 with S_10, S_00 with S_11 and S_02, S_20 with S_12, S_21: xy is the same number, bit for bit
    _, _, sw = _born(True)
    assert torch.equal(bits(sw[:, 5]), bits(d2[:, 5])), 'the xy component is not symmetric in its two sums'
    assert torch.equal(bits(sw[:, [1, 0, 2, 4, 3]]), bits(d2[:, [0, 1, 2, 3, 4]]))
    shapes = {'d2': (g.B, 6)}
    refused('strain_born n_mol < 0', shapes, _born_call(t, -1))
    for k in ('dg_d', 'geo', 'row_ptr', 'mol_ptr', 'd2'):
        refused(f'strain_born {k} NULL', shapes, _born_call(t, g.B, **{k: None}))
    nothing('strain_born n_mol = 0', shapes, _born_call(t, 0))


def test_zz_ratio_summary():
    """the worst |got - ref| / bound per stage output over every case above"""
    assert RATIOS, 'run after the stage tests'
    for stage, worst in sorted(RATIOS.items()):
        print(f'STAGE-RATIO {stage}: worst {worst:.3f}')
    assert max(RATIOS.values()) <= 1.0
