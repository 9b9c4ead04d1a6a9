"""The neighbour-list builders and the edge geometry kernels of csrc/graph.hip, every route called DIRECTLY through hip.lib() and
compared array by array with the statement of tests/graph_ref.py: the synchronous all-pairs route (nnhip_graph_count_pairs /
_pairs_z + nnhip_graph_pair_scan + nnhip_graph_finish), the early fill and its guard (nnhip_graph_finish_early / _finish_dev), the
single launch (nnhip_graph_small_dev), the per-molecule launches (nnhip_graph_mol_dev), the cell list
(nnhip_graph_count_cells_pairs + nnhip_graph_finish_cells, nnhip_graph_fill_cells), the reused list (nnhip_edge_disp +
nnhip_edge_embed, nnhip_edge_refresh), nnhip_edge_index_from_csr and nnhip_graph_pairs.

Integer arrays (mol_ptr, row_ptr, pair_ptr, col, rev, pid, edge_index, status / tail words) are compared exactly, disp bit for
bit, geo / xg / rbf / drbf element by element with the derived bounds of tests/graph_ref.py (one `GRAPH-RATIO` line per output and
route with the worst |got - ref| / bound).  Every output buffer starts as a sentinel and is over-allocated: entries past E (or past
the capacity) and the guard entries behind every array must still hold the sentinel.  Every case runs twice and must repeat bit
for bit, and every other route must equal the synchronous all-pairs route's arrays bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import graph_ref as G
from tests.test_hip_dense_stages import OK, SENT, _stop_after_a_gpu_fault  # noqa: F401  (the fixture is autouse here too)

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64                       # sentinel entries behind every array
E_INVALID, E_UNSUPPORTED = 1, 2
RATIOS = {}
_CACHE = {}
FREQ20 = (np.arange(1, 21) * np.pi).astype(f32)


def _hip():
    from newtonnet_amd import hip
    return hip


def _st():
    return _hip()._stream(torch.device('cuda', 0))


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def sent(n, dtype=torch.int32, pinned=False):
    """n elements + GUARD of the sentinel"""
    t = torch.empty(int(n) + GUARD, dtype=dtype, device='cuda')
    t.view(torch.int32).fill_(SENT)
    return t


def is_sent(t):
    return bool((t.view(torch.int32) == SENT).all())


def dev(a, dtype):
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(8, dtype=dtype, device='cuda')
    return torch.from_numpy(a).to(dtype).cuda()


class Inputs:
    def __init__(self, case, batch=None, z=None, pos=None):
        self.case = case
        self.pos = dev(case.pos if pos is None else pos, torch.float32)
        self.cell = dev(case.cell, torch.float32)
        self.batch = dev(case.batch if batch is None else batch, torch.int64)
        self.z = dev(case.z if z is None else z, torch.int64)
        self.N, self.B, self.cutoff = case.N, case.B, case.cutoff


class Out:
    """the output arrays of one build: meta arrays sized by N / B, edge arrays sized by `cap`"""

    def __init__(self, N, B, cap, nb=20, rbf=True, ei=True):
        self.N, self.B, self.cap, self.nb = N, B, cap, nb
        n_scan = N // 1024 + 2
        self.mol_ptr, self.row_ptr, self.pair_ptr = sent(B + 1), sent(N + 1), sent(N + 1)
        self.status, self.pair_scan = sent(1 + n_scan), sent(n_scan)
        self.col, self.rev, self.pid, self.xg = sent(cap), sent(cap), sent(cap), sent(2 * cap)
        self.disp, self.geo = sent(3 * cap, torch.float32), sent(4 * cap, torch.float32)
        self.rbf = sent(nb * cap, torch.float32) if rbf else None
        self.drbf = sent(nb * cap, torch.float32) if rbf else None
        self.ei = sent(2 * cap, torch.int64) if ei else None

    EDGE = (('col', 1), ('rev', 1), ('pid', 1), ('xg', 2), ('disp', 3), ('geo', 4))

    def edge_fields(self):
        f = list(self.EDGE)
        if self.rbf is not None:
            f += [('rbf', self.nb), ('drbf', self.nb)]
        return f

    def check_sentinels(self, E, what, meta=True):
        """entries past E of every edge array, and the guards of every array"""
        for name, w in self.edge_fields():
            assert is_sent(getattr(self, name)[w * E:]), f'{what}: {name} was written past its {E} edges'
        if self.ei is not None:
            assert is_sent(self.ei[2 * E:]), f'{what}: edge_index was written past 2 E'
        if meta:
            for name, n in (('mol_ptr', self.B + 1), ('row_ptr', self.N + 1), ('pair_ptr', self.N + 1)):
                assert is_sent(getattr(self, name)[n:]), f'{what}: a guard entry of {name} was written'

    def untouched(self, what):
        self.check_sentinels(0, what, meta=False)

    def host(self, E):
        h = {k: getattr(self, k)[:n].cpu().numpy() for k, n in (('mol_ptr', self.B + 1), ('row_ptr', self.N + 1), ('pair_ptr', self.N + 1))}
        for name, w in self.edge_fields():
            a = getattr(self, name)[:w * E].cpu().numpy()
            h[name] = a.reshape(E, w) if w > 1 else a
        if self.ei is not None:
            h['edge_index'] = self.ei[:2 * E].cpu().numpy().reshape(2, E)
        h['status'] = int(self.status[0].item())
        return h


def same_bits(a, b, what):
    for k in a:
        if k in b and not isinstance(a[k], int):
            x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
            assert x.shape == y.shape and np.array_equal(x.view(np.int32) if x.dtype == f32 else x, y.view(np.int32) if y.dtype == f32 else y), \
                f'{what}: {k} differs'
        elif k in b:
            assert a[k] == b[k], f'{what}: {k} differs'


def twice(build, what):
    a, b = build(), build()
    same_bits(a, b, f'{what} (second run)')
    return a


# ---------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------
def check_list(h, lst, what, ei=True, status=None):
    for k in ('mol_ptr', 'row_ptr', 'pair_ptr', 'col', 'rev', 'pid'):
        assert np.array_equal(h[k], getattr(lst, k)), f'{what}: {k}'
    if ei and 'edge_index' in h:
        assert np.array_equal(h['edge_index'], lst.edge_index), f'{what}: edge_index'
    assert np.array_equal(h['disp'].view(np.int32), lst.disp.view(np.int32)), f'{what}: disp is not bit-equal'
    if status is not None:
        assert h['status'] == status, f'{what}: status {h["status"]} != {status}'


def ratio(route, name, got, ref, bound, what):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref).astype(np.float64), np.asarray(bound, np.float64)
    if got.size == 0:
        return
    assert np.isfinite(got).all(), f'{route} {name} {what}: not finite / not written'
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(r.max())
    RATIOS[(name, route)] = max(RATIOS.get((name, route), 0.0), worst)
    print(f'GRAPH-RATIO {name} [{route}] {what}: {worst:.3f}')
    assert worst <= 1.0, f'{route} {name} {what}: |got - ref| / bound = {worst:.3g} at {np.unravel_index(r.argmax(), r.shape)}'


def reference_geometry(key, disp, cutoff, freq, env):
    k = ('geo', key, None if freq is None else len(freq), env)
    if k not in _CACHE:
        _CACHE[k] = G.edge_geometry(disp, cutoff, freq, env)
    return _CACHE[k]


def _diff(got, ref):
    """got (fp32 array) - ref (longdouble), as float64 error and float64 reference for `ratio`"""
    d = (np.asarray(got, np.float64).astype(np.longdouble) - ref).astype(np.float64)
    return d


def check_geometry(route, h, key, disp, cutoff, freq=None, env=9, what=''):
    ref = reference_geometry(key, disp, cutoff, freq, env)
    zero = np.zeros_like
    g, Bg = ref['geo']
    ratio(route, 'geo', _diff(h['geo'], g), zero(Bg), Bg, what)
    assert np.array_equal(h['xg'][:, 0], ref['xg_index']), f'{route} {what}: xg interval index'
    frac = np.ascontiguousarray(h['xg'][:, 1]).view(f32)
    fr, Bf = ref['xg_frac']
    m = ref['masked']
    assert not h['xg'][m, 1].any(), f'{route} {what}: a masked candidate has a fraction'
    ratio(route, 'xg', _diff(frac, fr)[~m], zero(Bf[~m]), Bf[~m], what)
    if freq is not None and 'rbf' in h:
        for name in ('rbf', 'drbf'):
            v, B = ref[name]
            assert not h[name][m].any(), f'{route} {what}: a masked row of {name} is not zero'
            ratio(route, name, _diff(h[name], v), zero(B), B, what)


# ---------------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------------
def count_pairs(inp, o, dual):
    L = _hip().lib()
    if dual:
        rc = L.nnhip_graph_count_pairs_z(p(inp.pos), p(inp.cell), p(inp.batch), p(inp.z), inp.N, inp.B, inp.cutoff, p(o.mol_ptr),
                                         p(o.row_ptr), p(o.status), p(o.pair_ptr), p(o.pair_scan), _st())
        assert rc == OK, L.nnhip_last_error()
    else:
        rc = L.nnhip_graph_count_pairs(p(inp.pos), p(inp.cell), p(inp.batch), inp.N, inp.B, inp.cutoff, p(o.mol_ptr), p(o.row_ptr),
                                       p(o.status), p(o.pair_ptr), _st())
        assert rc == OK, L.nnhip_last_error()
        rc = L.nnhip_graph_pair_scan(p(o.pair_ptr), inp.N, p(o.pair_scan), _st())
        assert rc == OK, L.nnhip_last_error()


def finish_args(inp, o, n_edges, freq, env):
    return (p(inp.pos), p(inp.cell), p(inp.batch), p(o.mol_ptr), p(o.row_ptr), p(o.pair_ptr), inp.N, inp.B, n_edges, inp.cutoff,
            p(o.col), p(o.rev), p(o.pid), p(o.disp), p(o.ei), p(freq), o.nb, p(o.geo), p(o.rbf), p(o.drbf), p(o.xg), env)


def all_pairs(case, dual=False, nb=20, env=9, rbf=True, ei=True):
    """the synchronous route; returns the host arrays"""
    L = _hip().lib()
    inp = Inputs(case)
    freq = dev(FREQ20[:nb], torch.float32)
    E = case.list.E

    def build():
        o = Out(case.N, case.B, E + 6, nb, rbf, ei)
        count_pairs(inp, o, dual)
        got_E = int(o.row_ptr[case.N].item())
        assert got_E == E, f'{case.name}: {got_E} edges, the statement has {E}'
        # (edge_index rows are written at stride n_edges: the [2][E] block)
        rc = L.nnhip_graph_finish(*finish_args(inp, o, E, freq, env), _st())
        torch.cuda.synchronize()
        assert rc == OK, L.nnhip_last_error()
        o.check_sentinels(E, case.name)
        return o.host(E)
    return twice(build, f'all-pairs {case.name}')


def sync_arrays(case):
    """the synchronous all-pairs route's arrays of a case, built once (what every other route must equal bit for bit)"""
    k = ('sync', case.name)
    if k not in _CACHE:
        _CACHE[k] = all_pairs(case)
    return _CACHE[k]


ALL_PAIRS = ('sizes', 'full', 'chain1023', 'chain1024', 'chain1025', 'chain2049', 'ties5', 'ties1', 'ties6.3', 'boundary a',
             'boundary b diagonal')


@pytest.mark.parametrize('name', ALL_PAIRS)
def test_all_pairs(name):
    case = G.gpu_cases()[name]
    h = sync_arrays(case)
    st = G.status_bits(case.batch, case.B, case.z)
    check_list(h, case.list, f'all-pairs {name}', status=st)
    check_geometry('all-pairs', h, name, case.list.disp, case.cutoff, FREQ20, 9, name)
    dual = all_pairs(case, dual=True)
    same_bits(dual, h, f'count_pairs_z (dual scan) {name}')


def test_all_pairs_no_atoms():
    L = _hip().lib()
    o = Out(0, 3, 4)
    inp = Inputs(G.Case('empty', np.zeros((0, 3)), np.zeros((3, 9)), np.zeros(0, np.int64), 5.0))
    count_pairs(inp, o, False)
    torch.cuda.synchronize()
    assert o.mol_ptr[:4].tolist() == [0, 0, 0, 0] and o.row_ptr[0].item() == 0 and o.pair_ptr[0].item() == 0 and o.status[0].item() == 0
    rc = L.nnhip_graph_finish(*finish_args(inp, o, 0, dev(FREQ20, torch.float32), 9), _st())
    torch.cuda.synchronize()
    assert rc == OK
    o.check_sentinels(0, 'N = 0')
    assert is_sent(o.row_ptr[1:]) and is_sent(o.pair_ptr[1:])


# ---------------------------------------------------------------------------------------------------------------------------
# the early fill and its guard
# ---------------------------------------------------------------------------------------------------------------------------
def early(case, capacity, guard, batch=None, z=None, seq=7):
    L = _hip().lib()
    inp = Inputs(case, batch=batch, z=z)
    freq = dev(FREQ20, torch.float32)

    def build():
        o = Out(case.N, case.B, capacity)
        count_pairs(inp, o, True)
        tail = torch.full((4,), -1, dtype=torch.int32).pin_memory()
        changes = dev(np.array([41], np.int32), torch.int32)
        if guard:
            rc = L.nnhip_graph_finish_dev(*finish_args(inp, o, capacity, freq, 9), p(o.status), C.c_void_p(tail.data_ptr()), p(changes), seq, _st())
        else:
            rc = L.nnhip_graph_finish_early(*finish_args(inp, o, capacity, freq, 9), _st())
        torch.cuda.synchronize()
        assert rc == OK, L.nnhip_last_error()
        return o, tail.tolist()
    (o1, t1), (o2, t2) = build(), build()
    assert t1 == t2
    return o1, o2, t1


@pytest.mark.parametrize('guard', [False, True])
def test_finish_early_and_dev(guard):
    case = G.gpu_cases()['sizes']
    lst, E = case.list, case.list.E
    st = G.status_bits(case.batch, case.B, case.z)
    ref = sync_arrays(case)
    route = 'finish_dev' if guard else 'finish_early'
    for cap in (E, E + 2, 4 * E):
        o1, o2, tail = early(case, cap, guard)
        o1.check_sentinels(E, f'{route} capacity {cap}')
        h = o1.host(E)                                      # (edge_index row 1 starts at the TRUE E: host() reads the [2][E] block)
        same_bits(h, o2.host(E), f'{route} capacity {cap} (second run)')
        check_list(h, lst, f'{route} capacity {cap}', status=st)
        same_bits(h, ref, f'{route} capacity {cap} against the synchronous route')
        if guard:
            assert tail == [E, st, 41, 7], tail
    o1, o2, tail = early(case, E - 2, guard)
    o1.untouched(f'{route} capacity E - 2')
    if guard:
        rp, pp = G.emptied_guard(lst.row_ptr)
        assert np.array_equal(o1.row_ptr[:case.N + 1].cpu().numpy(), rp) and np.array_equal(o1.pair_ptr[:case.N + 1].cpu().numpy(), pp)
        assert tail == [E, st, 41, 7], tail
    else:
        assert np.array_equal(o1.row_ptr[:case.N + 1].cpu().numpy(), lst.row_ptr)
    if guard:     # status bits 1 and 2 empty the graph
        bad_batch = case.batch.copy()
        bad_batch[-1] = 0                                   # (unsorted; no two atoms then race for one mol_ptr entry: the count repeats)
        bad_z = case.z.copy()
        bad_z[3] = G.N_ELEMENTS
        for kw, bit in ((dict(batch=bad_batch), 1), (dict(z=bad_z), 2)):
            o1, o2, tail = early(case, 4 * E, True, **kw)
            assert tail[1] & bit and tail[3] == 7, tail
            rp = o1.row_ptr[:case.N + 1].cpu().numpy()
            assert (rp == rp[-1]).all() and not o1.pair_ptr[:case.N + 1].any().item(), f'status bit {bit}: the graph is not emptied'
            assert tail[0] == rp[-1]
            o1.check_sentinels(4 * E, f'status bit {bit}')
            assert tail[1] == G.status_bits(kw.get('batch', case.batch), case.B, kw.get('z', case.z)) | (st if bit == 2 else tail[1] & 8)


# ---------------------------------------------------------------------------------------------------------------------------
# the single launch
# ---------------------------------------------------------------------------------------------------------------------------
def small(case, capacity, ei=True, batch=None, z=None, want_rc=OK, seq=9):
    L = _hip().lib()
    inp = Inputs(case, batch=batch, z=z)
    freq = dev(FREQ20, torch.float32)

    def build():
        o = Out(max(case.N, 1), case.B, capacity, rbf=False, ei=ei)
        o.N = case.N
        tail = sent(4)
        rc = L.nnhip_graph_small_dev(p(inp.pos), p(inp.cell), p(inp.batch), p(inp.z), case.N, case.B, capacity, case.cutoff, p(o.mol_ptr),
                                     p(o.row_ptr), p(o.pair_ptr), p(tail), None, seq, p(o.col), p(o.rev), p(o.pid), p(o.disp), p(o.ei),
                                     p(freq), 20, p(o.geo), p(o.xg), 9, _st())
        torch.cuda.synchronize()
        assert rc == want_rc, (rc, L.nnhip_last_error())
        assert is_sent(tail[4:])
        return o, tail[:4].tolist()
    (o1, t1), (o2, t2) = build(), build()
    assert t1 == t2
    return o1, o2, t1


@pytest.mark.parametrize('n', G.SMALL_N)
def test_small_launch(n):
    case = G.gpu_cases()[f'small{n}']
    lst, E = case.list, case.list.E
    st = G.status_bits(case.batch, case.B, case.z)
    cap = max(E + 4, 2)
    for ei in (True, False):
        o1, o2, tail = small(case, cap, ei=ei)
        assert tail == [E, st, 0, 9], tail
        o1.check_sentinels(E, f'small {n}')
        h = o1.host(E)
        same_bits(h, o2.host(E), f'small {n} (second run)')
        h['status'] = tail[1]
        check_list(h, lst, f'small {n}', status=st)
        if E:
            ref = sync_arrays(case)
            same_bits({k: v for k, v in h.items() if k not in ('rbf', 'drbf')}, ref, f'small {n} against the synchronous route')
            check_geometry('small', h, case.name, lst.disp, case.cutoff, None, 9, case.name)
    if n >= 1023:
        assert st & 8                                               # a molecule above NNHIP_MOL_STAGE_MAX
    if E >= 4:
        o1, o2, tail = small(case, E - 2)
        assert tail == [E, st, 0, 9], tail                          # tail[0] is still the true count
        rp, pp = G.emptied_small(case.N)
        assert np.array_equal(o1.row_ptr[:n + 1].cpu().numpy(), rp) and np.array_equal(o1.pair_ptr[:n + 1].cpu().numpy(), pp)
        o1.untouched(f'small {n} capacity E - 2')
        assert is_sent(o1.row_ptr[n + 1:]) and is_sent(o1.pair_ptr[n + 1:])
    if n == 17:
        bad_batch = case.batch.copy()
        bad_batch[-1] = 0                                           # unsorted
        bad_z = case.z.copy()
        bad_z[0] = -1
        for kw, bit in ((dict(batch=bad_batch), 1), (dict(z=bad_z), 2)):
            o1, o2, tail = small(case, cap, **kw)
            assert tail[1] & bit and tail[3] == 9
            assert not o1.row_ptr[:n + 1].any().item() and not o1.pair_ptr[:n + 1].any().item()
            o1.untouched(f'small {n} status bit {bit}')


def test_small_launch_refusals():
    for n in (0, 1025):
        case = G.Case(f'refused{n}', np.zeros((n, 3)), np.zeros((1, 9)), np.zeros(n, np.int64), 1.0)
        o1, o2, tail = small(case, 16, want_rc=E_INVALID)
        o1.untouched(f'small {n}')
        assert is_sent(o1.row_ptr) and is_sent(o1.pair_ptr) and is_sent(o1.mol_ptr) and tail == [SENT] * 4


# ---------------------------------------------------------------------------------------------------------------------------
# a workgroup per molecule
# ---------------------------------------------------------------------------------------------------------------------------
def mol(case, capacity, initialised=0, seq=11):
    L = _hip().lib()
    inp = Inputs(case)

    def build():
        o = Out(case.N, case.B, capacity, rbf=False, ei=False)
        scratch = sent(2 * case.B + case.B // 1024 + 4)
        status = sent(1)
        if initialised:                                             # (what graph_init_kernel would have done)
            status[:1].zero_()
            o.mol_ptr[:case.B + 1].zero_()
            o.row_ptr[:case.N + 1].zero_()
        tail = torch.full((4,), -1, dtype=torch.int32).pin_memory()
        rc = L.nnhip_graph_mol_dev(p(inp.pos), p(inp.cell), p(inp.batch), p(inp.z), case.N, case.B, capacity, case.cutoff, p(o.mol_ptr),
                                   p(o.row_ptr), p(o.pair_ptr), p(status), p(scratch), initialised, C.c_void_p(tail.data_ptr()), None, seq,
                                   p(o.col), p(o.rev), p(o.pid), p(o.disp), p(o.geo), p(o.xg), _st())
        torch.cuda.synchronize()
        assert rc == OK, L.nnhip_last_error()
        assert is_sent(scratch[2 * case.B + case.B // 1024 + 4:]) and is_sent(status[1:])
        o.status = status
        return o, tail.tolist()
    (o1, t1), (o2, t2) = build(), build()
    assert t1 == t2
    return o1, o2, t1


MOL_CASES = ('mol sizes', 'full64', 'full65', 'full64+65', 'chain1024') + tuple(f'mols{b}' for b in G.MOL_B)


@pytest.mark.parametrize('name', MOL_CASES)
def test_per_molecule(name):
    case = G.gpu_cases()[name]
    lst, E = case.list, case.list.E
    st = G.status_bits(case.batch, case.B, case.z, route='mol')
    for initialised in (0, 1):
        o1, o2, tail = mol(case, E + 2, initialised)
        assert tail == [E, st, 0, 11], tail
        o1.check_sentinels(E, f'mol {name}')
        h = o1.host(E)
        same_bits(h, o2.host(E), f'mol {name} (second run)')
        check_list(h, lst, f'mol {name} initialised {initialised}', status=st)
    ref = sync_arrays(case)
    same_bits({k: v for k, v in h.items() if k not in ('status',)}, {k: v for k, v in ref.items() if k not in ('rbf', 'drbf', 'edge_index')},
              f'mol {name} against the synchronous route')
    check_geometry('mol', h, case.name, lst.disp, case.cutoff, None, 9, case.name)
    if name in ('mol sizes', 'full64+65'):                          # the capacity does not hold the list: the guard's emptied graph
        o1, o2, tail = mol(case, E - 2)
        assert tail == [E, st, 0, 11], tail
        rp, pp = G.emptied_guard(lst.row_ptr)
        assert np.array_equal(o1.row_ptr[:case.N + 1].cpu().numpy(), rp) and np.array_equal(o1.pair_ptr[:case.N + 1].cpu().numpy(), pp)
        for nm, w in o1.edge_fields():
            assert is_sent(getattr(o1, nm)[w * (E - 2):]), f'mol {name} capacity E - 2: {nm} written past the capacity'


def test_per_molecule_too_large():
    """a 1025-atom chain: bits 8 | 16, an emptied graph, nothing written"""
    case = G.gpu_cases()['chain1025']
    o1, o2, tail = mol(case, case.list.E + 2)
    assert tail == [0, 8 | 16, 0, 11], tail
    assert G.status_bits(case.batch, case.B, case.z, route='mol') == 8 | 16
    assert not o1.row_ptr[:case.N + 1].any().item() and not o1.pair_ptr[:case.N + 1].any().item()
    o1.untouched('mol 1025')
    assert o1.status[0].item() == 8 | 16


# ---------------------------------------------------------------------------------------------------------------------------
# the cell list
# ---------------------------------------------------------------------------------------------------------------------------
def cells(case, finish=True):
    L = _hip().lib()
    inp = Inputs(case)
    box = (C.c_float * 3)(*[float(v) for v in case.box])
    freq = dev(FREQ20, torch.float32)
    E = case.list.E
    n_bytes = L.nnhip_graph_cells_scratch_bytes(case.N, box, case.cutoff)
    assert n_bytes > 0

    def build():
        o = Out(case.N, 1, E + 6, rbf=False)
        scratch = sent(n_bytes // 4)
        rc = L.nnhip_graph_count_cells_pairs(p(inp.pos), p(inp.cell), case.N, case.cutoff, box, p(scratch), p(o.mol_ptr), p(o.row_ptr),
                                             p(o.pair_ptr), _st())
        assert rc == OK, L.nnhip_last_error()
        rc = L.nnhip_graph_pair_scan(p(o.pair_ptr), case.N, p(o.pair_scan), _st())
        assert rc == OK, L.nnhip_last_error()
        assert int(o.row_ptr[case.N].item()) == E
        if finish:
            rc = L.nnhip_graph_finish_cells(p(inp.pos), p(inp.cell), case.N, E, case.cutoff, box, p(scratch), p(o.row_ptr), p(o.pair_ptr),
                                            p(o.col), p(o.rev), p(o.pid), p(o.disp), p(o.ei), p(freq), 20, p(o.geo), None, None, p(o.xg), 9, _st())
        else:
            rc = L.nnhip_graph_fill_cells(p(inp.pos), p(inp.cell), case.N, E, case.cutoff, box, p(scratch), p(o.row_ptr), p(o.col), p(o.rev),
                                          p(o.disp), p(o.ei), _st())
        torch.cuda.synchronize()
        assert rc == OK, L.nnhip_last_error()
        assert is_sent(scratch[n_bytes // 4:])
        if finish:
            o.check_sentinels(E, case.name)
        else:
            for nm, w in (('col', 1), ('rev', 1), ('disp', 3)):
                assert is_sent(getattr(o, nm)[w * E:])
            assert is_sent(o.pid) and is_sent(o.geo) and is_sent(o.xg) and is_sent(o.ei[2 * E:])
        h = o.host(E)
        h['status'] = 0
        return h
    return twice(build, f'cells {case.name}')


@pytest.mark.parametrize('n_ball', [257, 258])
def test_cell_list(n_ball):
    case = G.gpu_cases()[f'cells{n_ball}']
    lst = case.list
    h = cells(case)
    check_list(h, lst, case.name)
    ref = sync_arrays(case)
    same_bits({k: v for k, v in h.items() if k != 'status'}, {k: v for k, v in ref.items() if k not in ('rbf', 'drbf', 'status')},
              f'{case.name} against the all-pairs route')
    check_list(ref, lst, f'all-pairs {case.name}')
    check_geometry('cells', h, case.name, lst.disp, case.cutoff, None, 9, case.name)
    f = cells(case, finish=False)
    for k in ('row_ptr', 'col', 'rev', 'edge_index'):
        assert np.array_equal(f[k], getattr(lst, k)), f'fill_cells {case.name}: {k}'
    assert np.array_equal(f['disp'].view(np.int32), lst.disp.view(np.int32))


def test_cell_list_refuses_a_box_one_float_below_the_threshold():
    L = _hip().lib()
    hip = _hip()
    case = G.gpu_cases()['cells257']
    below = case.box.copy()
    below[0] = np.nextafter(below[0], f32(0))
    box = (C.c_float * 3)(*[float(v) for v in below])
    assert L.nnhip_graph_cells_scratch_bytes(case.N, box, case.cutoff) == 0
    assert hip._orthorhombic_box(None, case.cutoff, cell_host=np.diag(below)) is None
    assert hip._orthorhombic_box(None, case.cutoff, cell_host=np.diag(case.box)) is not None
    inp = Inputs(case)
    o = Out(case.N, 1, 8)
    scratch = sent(4 * case.N + 4096)
    rc = L.nnhip_graph_count_cells_pairs(p(inp.pos), p(inp.cell), case.N, case.cutoff, box, p(scratch), p(o.mol_ptr), p(o.row_ptr),
                                         p(o.pair_ptr), _st())
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED
    assert is_sent(scratch) and is_sent(o.row_ptr) and is_sent(o.mol_ptr) and is_sent(o.pair_ptr)
    pos = torch.from_numpy(case.pos).cuda()
    assert hip._cell_list_in_range(pos, case.cutoff) and not hip._cell_list_in_range(pos * 1.2, case.cutoff)


def test_build_graph_leaves_the_cell_list_beyond_its_range():
    """hip.build_graph sends one big orthorhombic box to the cell list only while every |coordinate| <= CELL_LIST_MAX_COORD cutoffs;
    with one atom beyond, the all-pairs builder serves the same system.  Either way the list is the statement's."""
    hip = _hip()
    L = hip.lib()
    rng = np.random.default_rng(12)
    cutoff = G.CELLS_CUTOFF
    box = (G.cells_box(cutoff) * f32(2)).astype(f32)
    n = hip.CELL_LIST_MIN_ATOMS + 9
    base = rng.random((n, 3)) * box.astype(np.float64)
    kmax = np.floor(G.CELL_LIST_MAX_COORD * cutoff / box.astype(np.float64)).astype(int) - 1
    inside = base + rng.integers(-kmax, kmax + 1, (n, 3)) * box.astype(np.float64)
    beyond = inside.copy()
    beyond[17, 1] = np.sign(beyond[17, 1]) * max(abs(beyond[17, 1]), 1.3 * G.CELL_LIST_MAX_COORD * cutoff)
    calls = []
    real = L.nnhip_graph_count_cells_pairs

    def spy(*a):
        calls.append(1)
        return real(*a)
    L.nnhip_graph_count_cells_pairs = spy
    try:
        for name, pos, want_cells in (('inside', inside, True), ('beyond', beyond, False)):
            case = G.Case(f'range {name}', pos, G.diag_cell(*box)[None], np.zeros(n, np.int64), cutoff)
            assert G.eligible(box, cutoff, case.pos) == want_cells
            del calls[:]
            g = hip.build_graph(torch.from_numpy(case.pos).cuda(), torch.from_numpy(case.cell.reshape(1, 3, 3)).cuda(),
                                torch.from_numpy(case.batch).cuda(), cutoff, torch.from_numpy(FREQ20).cuda())
            assert bool(calls) == want_cells, f'{name}: the cell list was {"not " if want_cells else ""}used'
            lst = case.list
            assert lst.tie_share == 0.0
            assert g.n_edges == lst.E and np.array_equal(g.edge_index.cpu().numpy(), lst.edge_index)
            assert np.array_equal(g.disp.cpu().numpy().view(np.int32), lst.disp.view(np.int32))
            assert np.array_equal(g.rev.cpu().numpy(), lst.rev) and np.array_equal(g.pid.cpu().numpy(), lst.pid)
    finally:
        L.nnhip_graph_count_cells_pairs = real


# ---------------------------------------------------------------------------------------------------------------------------
# reused lists
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb,env', [(20, 9), (1, 9), (G.MAX_NB, 9), (20, 6), (20, G.COSINE)])
def test_reused_list(nb, env):
    L = _hip().lib()
    c0, pos1, cutoff = G.reuse_inputs()
    lst = c0.list
    E = lst.E
    d_ref, r2, tie = G.disp_of_edges(pos1, c0.cell, c0.batch, lst.edge_index)
    assert not tie.any()
    inp = Inputs(c0, pos=pos1)
    ei = dev(lst.edge_index, torch.int64)
    fr = (np.arange(1, nb + 1) * np.pi).astype(f32)
    freq = dev(fr, torch.float32)
    key = f'reuse {nb} {env}'

    def two_calls(given):
        def build():
            o = Out(c0.N, c0.B, E + 5, nb, rbf=given, ei=False)
            rc = L.nnhip_edge_disp(p(inp.pos), p(inp.cell), p(inp.batch), p(ei), E, p(o.disp), _st())
            assert rc == OK, L.nnhip_last_error()
            rc = L.nnhip_edge_embed(p(o.disp), E, cutoff, p(freq), nb, p(o.geo), p(o.rbf), p(o.drbf), p(o.xg) if given else None, env, _st())
            torch.cuda.synchronize()
            assert rc == OK, L.nnhip_last_error()
            return o
        return build

    def one_call(given):
        def build():
            o = Out(c0.N, c0.B, E + 5, nb, rbf=given, ei=False)
            rc = L.nnhip_edge_refresh(p(inp.pos), p(inp.cell), p(inp.batch), p(ei), E, cutoff, p(freq), nb, p(o.disp), p(o.geo), p(o.rbf),
                                      p(o.drbf), p(o.xg) if given else None, env, _st())
            torch.cuda.synchronize()
            assert rc == OK, L.nnhip_last_error()
            return o
        return build
    results = {}
    for route, maker in (('edge_disp + edge_embed', two_calls), ('edge_refresh', one_call)):
        for given in (True, False):
            runs = []
            for _ in range(2):
                o = maker(given)()
                for nm, w in (('disp', 3), ('geo', 4)) + ((('xg', 2), ('rbf', nb), ('drbf', nb)) if given else ()):
                    assert is_sent(getattr(o, nm)[w * E:]), f'{route}: {nm} written past E'
                if not given:
                    assert is_sent(o.xg)
                assert is_sent(o.col) and is_sent(o.rev) and is_sent(o.pid)
                h = {nm: getattr(o, nm)[:w * E].cpu().numpy().reshape(E, w) for nm, w in (('disp', 3), ('geo', 4))}
                if given:
                    h.update({nm: getattr(o, nm)[:w * E].cpu().numpy().reshape(E, w) for nm, w in (('xg', 2), ('rbf', nb), ('drbf', nb))})
                runs.append(h)
            same_bits(runs[0], runs[1], f'{route} (second run)')
            h = runs[0]
            assert np.array_equal(h['disp'].view(np.int32), d_ref.view(np.int32)), f'{route}: disp is not bit-equal to the statement'
            if given:
                check_geometry(route, h, key, d_ref, cutoff, fr, env, f'nb {nb} envelope {env}')
                results[route] = h
            else:
                same_bits({k: h[k] for k in ('disp', 'geo')}, results[route], f'{route}: xg / rbf / drbf NULL changes disp or geo')
    same_bits(results['edge_refresh'], results['edge_disp + edge_embed'], 'edge_refresh against edge_disp + edge_embed')
    if (nb, env) == (20, 9):    # the surviving edges are what a fresh build with the real cutoff gives at the new positions
        fresh = G.Case('reuse (fresh)', pos1, c0.cell, c0.batch, cutoff)
        live = ~reference_geometry(key, d_ref, cutoff, fr, env)['masked']
        assert np.array_equal(lst.edge_index[:, live], fresh.list.edge_index)
        assert np.array_equal(d_ref[live].view(np.int32), fresh.list.disp.view(np.int32))
        g = sync_arrays(fresh)
        check_list(g, fresh.list, 'fresh build at the moved positions')
        assert np.array_equal(g['disp'].view(np.int32), h['disp'][live].view(np.int32))
        assert np.array_equal(g['geo'].view(np.int32), results['edge_refresh']['geo'][live].view(np.int32))
        assert np.array_equal(g['xg'], results['edge_refresh']['xg'][live])
        assert np.array_equal(g['rbf'].view(np.int32), results['edge_refresh']['rbf'][live].view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# edge_index from the CSR list, pair ids from the list
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['sizes', 'full', 'chain1025', 'mols8193', 'cells258', 'ties5'])
def test_edge_index_from_csr_and_pairs(name):
    L = _hip().lib()
    case = G.gpu_cases()[name]
    lst, E, N = case.list, case.list.E, case.N
    if name == 'full':
        assert np.diff(lst.row_ptr)[[0, -1]].tolist() == [0, 0]    # rows of degree 0 at both ends
    row_ptr, col, rev = dev(lst.row_ptr, torch.int32), dev(lst.col, torch.int32), dev(lst.rev, torch.int32)
    for cap, on_device in ((E, False), (E + 10, True), (3 * E, True)):
        outs = []
        for _ in range(2):
            ei = sent(2 * cap, torch.int64)
            rc = L.nnhip_edge_index_from_csr(p(row_ptr), p(col), N, cap, p(ei), C.c_void_p(row_ptr.data_ptr() + 4 * N) if on_device else None, _st())
            torch.cuda.synchronize()
            assert rc == OK, L.nnhip_last_error()
            assert is_sent(ei[2 * E:])
            outs.append(ei[:2 * E].cpu().numpy().reshape(2, E))
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], lst.edge_index), f'edge_index_from_csr {name} capacity {cap}'
    ei = sent(2 * (E - 2), torch.int64)                         # a capacity below the count: nothing is written
    rc = L.nnhip_edge_index_from_csr(p(row_ptr), p(col), N, E - 2, p(ei), C.c_void_p(row_ptr.data_ptr() + 4 * N), _st())
    torch.cuda.synchronize()
    assert rc == OK and is_sent(ei)
    outs = []
    for _ in range(2):
        pair_ptr, pid, scratch = sent(N + 1), sent(E), sent(N // 1024 + 2)
        rc = L.nnhip_graph_pairs(p(row_ptr), p(col), p(rev), N, E, p(pair_ptr), p(pid), p(scratch), _st())
        torch.cuda.synchronize()
        assert rc == OK, L.nnhip_last_error()
        assert is_sent(pair_ptr[N + 1:]) and is_sent(pid[E:]) and is_sent(scratch[N // 1024 + 2:])
        outs.append((pair_ptr[:N + 1].cpu().numpy(), pid[:E].cpu().numpy()))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    assert np.array_equal(outs[0][0], lst.pair_ptr) and np.array_equal(outs[0][1], lst.pid), f'graph_pairs {name}'


def test_zz_ratio_summary():
    """(runs last in this file: the worst ratio per output and route of the session)"""
    for (name, route), worst in sorted(RATIOS.items()):
        print(f'GRAPH-SUMMARY {name} [{route}]: {worst:.3f}')
    assert all(v <= 1.0 for v in RATIOS.values())
