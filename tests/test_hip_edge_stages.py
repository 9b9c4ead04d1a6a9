"""The edge and pair stages the C interface exports one by one (csrc/edge.hip and the tangent kernels at the head of
csrc/train.hip), each called DIRECTLY on independent random inputs and compared element by element with its float64 statement and
componentwise bound (tests/edge_ref.py): nnhip_embed, nnhip_message_fwd / _bwd, nnhip_force_message_fwd / _bwd,
nnhip_edge_embed_bwd, nnhip_head_out, nnhip_edge_tangent_geom, nnhip_message_tan_fwd / _bwd, nnhip_force_message_tan_fwd / _bwd,
nnhip_pair_rbf, and the *_ex entry points that pass what the pipeline passes (pair counts, reverse edges, molecule offsets, the
force tail of layer 0's message adjoint).

The harness is that of tests/test_hip_dense_stages.py: every output starts as a sentinel NaN and has 8 guard rows behind it that
must come back bit-identical; entries the interface leaves unwritten must still hold the sentinel; every case runs twice and must
repeat bit for bit; |got - ref| <= bound element by element; the largest ratio per (stage, form) is printed as a `STAGE-RATIO`
line and summed up in `STAGE-SUMMARY` lines.  The radial filter is read from the table nnhip_filter_tables builds on the device.

The graphs (tests/edge_ref.py: GRAPHS) are tiny and chosen by row degree, not by geometry; one more comes from hip.build_graph
and must equal the synthetic builder's arrays.  The `test_group_*` tests run again in child processes, once per switch set
(the switches are read once per process); every case names the kernel form that serves it from nnhip_config and the launchers'
predicates (csrc/edge.hip: EDGE_LAUNCH, mol_kernels_pay, launch_*).  That name is a LABEL the test computes: it says which form
the launcher should take under this process's switches, and test_group_forms_of_this_process asserts that the labels the child was
started for came up.  It is no proof that the kernel of that name ran: a launcher whose predicate drifted from the copy here would
pass while another form served the call (each form is still held to its bound).  The library itself reports one choice only, the
force tail (`tail_done`), and that one is compared.  Telling more would take a look into the compiled kernels or a profiler."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from newtonnet_amd import abi
from tests import dense_ref as D
from tests import edge_ref as R
from tests.test_hip_dense_stages import (ABNORMAL_RC, FAULT_MARKS, GUARD, OK, SENT,  # noqa: F401  (the fixture is autouse here too)
                                         _stop_after_a_gpu_fault)

pytestmark = pytest.mark.gpu

F = R.F
CHILD = os.environ.get('NNHIP_EDGE_CHILD', '')          # set by test_forms_in_child_processes
RATIOS = {}
GRAPH_NAMES = tuple(R.GRAPHS)
StageOpts = abi.STRUCTS['nnhip_stage_opts']


def _hip():
    from newtonnet_amd import hip
    return hip


def _stream():
    return _hip()._stream(torch.device('cuda', 0))


# ---------------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------------
def blank(rows, width):
    """[rows + GUARD][width] of the sentinel"""
    t = torch.empty(rows + GUARD, width, dtype=torch.float32, device='cuda')
    t.view(torch.int32).fill_(SENT)
    return t


def tin(a, dtype=None):
    """an input array on the device (one element at least: every pointer is valid)"""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(4, dtype=dtype or torch.float32, device='cuda')
    t = torch.from_numpy(a)
    return (t.to(dtype) if dtype is not None else t).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return t.view(torch.int32)


def record(stage, form, got, ref, what=''):
    """got against (value, bound, defined): the defined entries within the bound, the others still the sentinel"""
    val, B, defined = ref
    got32 = got.detach().cpu()
    g = got32.double().numpy().reshape(val.shape)
    raw = got32.view(torch.int32).numpy().reshape(val.shape)
    defined = np.broadcast_to(np.asarray(defined).reshape(np.asarray(defined).shape + (1,) * (val.ndim - np.asarray(defined).ndim)), val.shape)
    assert (raw[~defined] == SENT).all(), f'{stage} [{form}] {what}: an entry the interface leaves unwritten was written'
    if not defined.any():
        return 0.0
    gd, vd, Bd = g[defined], val[defined], B[defined]
    assert np.isfinite(gd).all(), f'{stage} [{form}] {what}: {int((~np.isfinite(gd)).sum())} elements not written / not finite'
    err = np.abs(gd - vd)
    ratio = np.where(Bd > 0, err / np.where(Bd > 0, Bd, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    RATIOS[(stage, form)] = max(RATIOS.get((stage, form), 0.0), worst)
    print(f'STAGE-RATIO {stage} [{form}] {what}: {worst:.3f}')
    if worst > 1.0:
        k = int(ratio.argmax())
        raise AssertionError(f'{stage} [{form}] {what}: |got - ref| / bound = {worst:.3g} (got {gd[k]!r}, ref {vd[k]!r}, bound {Bd[k]:.3g}); '
                             f'{int((ratio > 1).sum())} of {ratio.size} elements outside')
    return worst


def run_twice(what, shapes, call):
    """call(buffers) -> return code, twice on fresh sentinel buffers {name: [rows + GUARD][width]}: NNHIP_OK, guards intact, the two
    runs equal bit for bit.  Returns the first run's buffers cut to their rows."""
    L = _hip().lib()
    runs = []
    for _ in range(2):
        bufs = {k: blank(r, w) for k, (r, w) in shapes.items()}
        rc = call(bufs)
        torch.cuda.synchronize()
        assert rc == OK, (what, rc, L.nnhip_last_error())
        for k, (r, w) in shapes.items():
            assert bool((bits(bufs[k])[r:] == SENT).all()), f'{what}: a guard row of {k} was written'
        runs.append(bufs)
    for k in shapes:
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), f'{what}: {k} differs between two runs'
    return {k: runs[0][k][:shapes[k][0]] for k in shapes}


# ---------------------------------------------------------------------------------------------------------------------------
# the table, the graphs on the device, the forms
# ---------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def device_table():
    """(device tensor, host copy [3][FT_ROWS][F]) of the table nnhip_filter_tables builds for edge_ref.filter_weights()"""
    if 'table' not in _CACHE:
        hip = _hip()
        L = hip.lib()
        W, freq = R.filter_weights()
        Wd, fd = tin(W), tin(freq)
        n = L.nnhip_filter_table_bytes() // 4
        assert n == 3 * R.FT_ROWS * F
        t = torch.empty(n, dtype=torch.float32, device='cuda')
        vp = C.c_void_p
        rc = L.nnhip_filter_tables((vp * 1)(Wd.data_ptr()), (vp * 1)(t.data_ptr()), 1, fd.data_ptr(), R.N_BASIS, 9, _stream())
        torch.cuda.synchronize()
        assert rc == OK, L.nnhip_last_error()
        host = t.cpu().numpy().reshape(3, R.FT_ROWS, F)
        assert not host[:, R.FT_ZERO_ROW:].any()                   # the rows a masked candidate reads
        # the host statement of the same table (the CPU tests' table) agrees to the fp32 rounding of its entries
        mine = R.host_filter_table(W, freq)
        for k in range(3):
            assert np.abs(host[k, 3:] - mine[k, 3:]).max() <= 1e-5 * np.abs(mine[k]).max(), f'plane {k} of the device table'
        _CACHE['table'] = (t, host)
    return _CACHE['table']


class DevGraph:
    def __init__(self, g):
        self.g = g
        i32 = torch.int32
        self.row_ptr, self.col, self.rev, self.pid = (tin(a, i32) for a in (g.row_ptr, g.col, g.rev, g.pid))
        self.pair_ptr, self.mol_ptr = tin(g.pair_ptr, i32), tin(g.mol_ptr, i32)
        self.xg, self.geo = tin(g.xg.reshape(-1), i32), tin(g.geo)
        self.edge_index = tin(g.edge_index, torch.int64)


def graph(name):
    if name not in _CACHE:
        g = R.GRAPHS[name]()
        _CACHE[name] = (g, DevGraph(g), {k: v for k, v in R.stage_inputs(g).items()})
    return _CACHE[name]


def cfg():
    if 'cfg' not in _CACHE:
        _CACHE['cfg'] = _hip().config()
    return _CACHE['cfg']


def wpr(kernel, n_atoms):
    """EDGE_LAUNCH (csrc/edge.hip:934): the forced split, else four waves up to the small-system limit, else the kernel's own"""
    c = cfg()
    forced = int(c['env'].get('NNHIP_EDGE_WPR', '0'))
    forced = forced if forced in (1, 2, 4) else 0
    return forced or (4 if n_atoms <= c['edge_rows']['four_waves_per_row_up_to_atoms'] else c['edge_rows']['waves_per_row'][kernel])


def flag_on(name):
    """a flag switch (csrc/switches.h): on unless set to something atoi reads as 0"""
    v = cfg()['env'].get(name)
    if v is None:
        return True
    digits = ''
    for ch in v.strip():
        if ch.isdigit() or (ch in '+-' and not digits):
            digits += ch
        else:
            break
    return digits not in ('', '+', '-') and int(digits) != 0


def mol_pay(g):
    """mol_kernels_pay (csrc/edge.hip:963)"""
    mf = cfg()['molecule_forms']
    return g.B >= mf['edge_kernels_from_molecules'] and g.N <= g.B * mf['max_atoms'] and g.N >= 8 * g.B


def mol_small(g):
    return g.B > 0 and g.N <= g.B * cfg()['molecule_forms']['max_atoms']


def opts_of(dg, pair_ptr=True, rev=True, mol=True, small=True):
    o = StageOpts()
    o.pair_ptr = ptr(dg.pair_ptr) if pair_ptr else None
    o.rev = ptr(dg.rev) if rev else None
    o.mol_ptr = ptr(dg.mol_ptr) if mol else None
    o.n_mol = dg.g.B if mol else 0
    o.small_molecules = 1 if small else 0
    return o


def rows_form(kernel, g, extra=''):
    return f'{wpr(kernel, g.N)} waves per row{extra}'


# ---------------------------------------------------------------------------------------------------------------------------
# the stages
# ---------------------------------------------------------------------------------------------------------------------------
def message_fwd_case(name):
    g, dg, d = graph(name)
    L, (tab, tab_h) = _hip().lib(), device_table()
    m, a_in = tin(d['m']), tin(d['a_in'])
    ref = R.message_fwd(g, R.TableFilter(tab_h, g.xg), d['m'], d['a_in'])
    out = run_twice(f'message_fwd {name}', {'msg': (g.P, F), 'a_mid': (g.N, F)},
                    lambda b: L.nnhip_message_fwd(ptr(m), ptr(dg.xg), ptr(tab), ptr(dg.row_ptr), ptr(dg.col), ptr(dg.pid), ptr(a_in),
                                                  ptr(b['msg']), ptr(b['a_mid']), g.N, _stream()))
    form = rows_form('msg_fwd', g)
    for k in ('msg', 'a_mid'):
        record(f'message_fwd {k}', form, out[k], ref[k], name)
    if g.masked.any():
        assert not out['msg'][torch.as_tensor(np.unique(g.pid[g.masked])).cuda()].any(), 'a masked pair row of msg is not zero'


def _pair_sum(g, gx):
    """g_x[e] + g_x[rev e] per pair: the only combination the interface defines"""
    gx = gx.reshape(-1)
    own = torch.as_tensor(np.flatnonzero(g.own)).cuda()
    p = torch.as_tensor(g.pid[g.own].astype(np.int64)).cuda()
    out = torch.empty(g.P, dtype=torch.float32, device='cuda')
    out[p] = gx[own] + gx[torch.as_tensor(g.rev[g.own].astype(np.int64)).cuda()]
    return out


def message_bwd_case(name, need_gm):
    g, dg, d = graph(name)
    L, (tab, tab_h) = _hip().lib(), device_table()
    g_msg, g_a, m = tin(d['g_msg']), tin(d['g_a']), tin(d['m'])
    ref = R.message_bwd(g, R.TableFilter(tab_h, g.xg), d['g_msg'], d['g_a'], d['m'], need_gm)
    shapes = {'g_m': (g.N, F), 'g_x': (g.E, 1)}
    head = (ptr(g_msg), ptr(g_a), ptr(m), ptr(dg.xg), ptr(tab), ptr(dg.row_ptr), ptr(dg.col), ptr(dg.pid))
    mf = cfg()['molecule_forms']
    calls = [('plain', rows_form('msg_bwd', g), lambda b: L.nnhip_message_bwd(*head, ptr(b['g_m']), ptr(b['g_x']), g.N, need_gm, _stream()))]
    for tag, o in (('ex, pair counts', opts_of(dg, mol=False)), ('ex, pair counts + molecules', opts_of(dg))):
        molecule = o.mol_ptr is not None and mol_pay(g) and mf['msg_bwd']
        form = 'molecule-resident' if molecule else rows_form('msg_bwd', g, ', pair counts')
        calls.append((tag, form, lambda b, o=o: L.nnhip_message_bwd_ex(*head, ptr(b['g_m']), ptr(b['g_x']), g.N, need_gm, C.byref(o),
                                                                         None, _stream())))
    first = None
    for tag, form, call in calls:
        out = run_twice(f'message_bwd {name} {tag}', shapes, call)
        what = f'{name} need_gm={need_gm} {tag}'
        record('message_bwd g_m', form, out['g_m'], ref['g_m'], what)
        assert bool(torch.isfinite(out['g_x']).all()), f'{what}: an entry of g_x was not written'
        record('message_bwd g_x pair sum', form, _pair_sum(g, out['g_x']), ref['g_x_pair'], what)
        if first is not None and form.split(',')[0] == first[0].split(',')[0]:
            # the split from the pair counts is the split from the ballot: the same bits
            assert torch.equal(bits(out['g_x']), bits(first[1]['g_x'])) and torch.equal(bits(out['g_m']), bits(first[1]['g_m'])), what
        first = first or (form, out)


def message_bwd_force_tail_case(name):
    """layer 0's message adjoint going on with the forces (msg_bwd_mol_kernel<false, true>) where the launcher takes it, against
    the float64 forces of edge_embed_bwd from the g_x row the same launch wrote"""
    g, dg, d = graph(name)
    L, (tab, tab_h) = _hip().lib(), device_table()
    g_msg, g_a, m, g_u = tin(d['g_msg']), tin(d['g_a']), tin(d['m']), tin(d['g_u'])
    mf = cfg()['molecule_forms']
    expect = bool(mol_pay(g) and mf['msg_bwd'] and mf['msg_bwd_with_forces'] and mol_small(g))
    ref = R.message_bwd(g, R.TableFilter(tab_h, g.xg), d['g_msg'], d['g_a'], d['m'], 0)
    n_l = d['g_x'].shape[0]
    o = opts_of(dg)
    o.tail_g_u, o.tail_geo, o.tail_n_edges, o.tail_n_layers, o.tail_cutoff = ptr(g_u), ptr(dg.geo), g.E, n_l, g.cutoff
    done = C.c_int32(-1)

    def call(b):
        gx = b['g_x'].view(-1)                                    # g_x is [L][E]: row 0 is written, the others are inputs
        gx[g.E:n_l * g.E] = torch.from_numpy(d['g_x'][1:].reshape(-1)).cuda()
        o.tail_forces = ptr(b['forces'])
        return L.nnhip_message_bwd_ex(ptr(g_msg), ptr(g_a), ptr(m), ptr(dg.xg), ptr(tab), ptr(dg.row_ptr), ptr(dg.col), ptr(dg.pid),
                                      ptr(b['g_m']), ptr(gx), g.N, 0, C.byref(o), C.byref(done), _stream())
    shapes = {'g_m': (g.N, F), 'g_x': (n_l * g.E, 1), 'forces': (g.N, 3)}
    if not mol_small(g):          # more than NNHIP_MOL_STAGE_MAX atoms per molecule on average: the pipeline never asks, the wrapper refuses
        b = {k: blank(r, w) for k, (r, w) in shapes.items()}
        assert call(b) == 1 and done.value == -1, f'{name}: a force tail without small molecules must be refused'
        torch.cuda.synchronize()
        assert bool((bits(b['g_m']) == SENT).all()) and bool((bits(b['forces']) == SENT).all()) and bool((bits(b['g_x'])[:g.E] == SENT).all())
        return
    out = run_twice(f'message_bwd_ex force tail {name}', shapes, call)
    assert done.value == (1 if expect else 0), f'{name}: tail_done = {done.value}, the launcher\'s predicate says {int(expect)}'
    form = 'molecule-resident, with forces' if expect else ('molecule-resident' if mol_pay(g) and mf['msg_bwd'] else
                                                            rows_form('msg_bwd', g, ', pair counts'))
    gx = out['g_x'].view(n_l, g.E)
    assert torch.equal(bits(gx[1:]).cpu(), torch.from_numpy(d['g_x'][1:]).view(torch.int32)), 'an input row of g_x was written'
    record('message_bwd g_m', form, out['g_m'], ref['g_m'], f'{name} force tail')
    record('message_bwd g_x pair sum', form, _pair_sum(g, gx[0]), ref['g_x_pair'], f'{name} force tail')
    fref = R.edge_embed_bwd(g, gx.cpu().numpy(), d['g_u'])['forces']
    if expect:
        record('message_bwd_ex forces', form, out['forces'], fref, name)
    else:
        assert bool((bits(out['forces']) == SENT).all()), 'forces written without tail_done'


def force_message_fwd_case(name, has_f, masked_xg):
    g, dg, d = graph(name)
    L = _hip().lib()
    phi1, phi2, f_in = tin(d['phi1']), tin(d['phi2']), tin(d['f_in'])
    xg = ptr(dg.xg) if masked_xg else None
    fin = ptr(f_in) if has_f else None
    ref = R.force_message_fwd(g, d['phi1'], d['phi2'], d['f_in'] if has_f else None, use_mask=masked_xg)
    head = (ptr(phi1), ptr(phi2), ptr(dg.geo), xg, ptr(dg.row_ptr), ptr(dg.col), ptr(dg.pid), fin)
    mf = cfg()['molecule_forms']
    calls = [('plain', rows_form('force_fwd', g), lambda b: L.nnhip_force_message_fwd(*head, ptr(b['f_out']), g.N, _stream()))]
    for tag, o in (('ex, pair counts', opts_of(dg, mol=False)), ('ex, pair counts + molecules', opts_of(dg))):
        molecule = has_f and o.mol_ptr is not None and mol_pay(g) and mf['force_fwd']
        form = 'molecule-resident' if molecule else rows_form('force_fwd', g, ', pair counts')
        calls.append((tag, form, lambda b, o=o: L.nnhip_force_message_fwd_ex(*head, ptr(b['f_out']), g.N, C.byref(o), _stream())))
    first = None
    for tag, form, call in calls:
        what = f'{name} f_in={int(has_f)} xg={int(masked_xg)} {tag}'
        out = run_twice('force_message_fwd ' + what, {'f_out': (g.N, 3 * F)}, call)
        record('force_message_fwd f_out', form, out['f_out'], ref['f_out'], what)
        if first is not None and form.split(',')[0] == first[0].split(',')[0]:
            assert torch.equal(bits(out['f_out']), bits(first[1]['f_out'])), what
        first = first or (form, out)


def force_message_bwd_case(name, has_f, masked_xg):
    g, dg, d = graph(name)
    L = _hip().lib()
    gf, phi1, phi2, f_in = tin(d['gf']), tin(d['phi1']), tin(d['phi2']), tin(d['f_in'])
    xg = ptr(dg.xg) if masked_xg else None
    fin = ptr(f_in) if has_f else None
    ref = R.force_message_bwd(g, d['gf'], d['phi1'], d['phi2'], d['f_in'] if has_f else None, use_mask=masked_xg)
    head = (ptr(gf), ptr(phi1), ptr(phi2), ptr(dg.geo), xg, ptr(dg.row_ptr), ptr(dg.col), ptr(dg.pid), fin)
    shapes = {'g_h12': (g.P, 2 * F), 'g_u': (g.E, 4), 'g_fin': (g.N, 3 * F)}
    owner = flag_on('NNHIP_FORCE_BWD_OWNER_GU')                      # launch_force_bwd (csrc/edge.hip:1020)
    calls = [('plain', rows_form('force_bwd', g, ', every row its own g_u'),
              lambda b: L.nnhip_force_message_bwd(*head, ptr(b['g_h12']), ptr(b['g_u']), ptr(b['g_fin']), g.N, _stream()))]
    for tag, o in (('ex, pair counts', opts_of(dg, rev=False)), ('ex, pair counts + rev', opts_of(dg))):
        by_owner = o.rev is not None and owner
        form = rows_form('force_bwd', g, ', the owner writes g_u' if by_owner else ', every row its own g_u')
        calls.append((tag, form, lambda b, o=o: L.nnhip_force_message_bwd_ex(*head, ptr(b['g_h12']), ptr(b['g_u']), ptr(b['g_fin']), g.N,
                                                                               C.byref(o), _stream())))
    first = None
    for tag, form, call in calls:
        what = f'{name} f_in={int(has_f)} xg={int(masked_xg)} {tag}'
        out = run_twice('force_message_bwd ' + what, shapes, call)
        for k in shapes:
            record(f'force_message_bwd {k}', form, out[k], ref[k], what)
        if first is not None:       # "same operands, same lane layout, same reduction: the bits of g_u do not change"
            for k in shapes:
                assert torch.equal(bits(out[k]), bits(first[k])), f'{what}: {k} differs from the plain entry point'
        first = first or out


def edge_embed_bwd_case(name, want_virial):
    g, dg, d = graph(name)
    L = _hip().lib()
    n_l = d['g_x'].shape[0]
    g_x, g_u, pos = tin(d['g_x']), tin(d['g_u']), tin(d['pos'])
    disp = tin(d['pos'][g.i] - d['pos'][g.j]) if g.E else tin(np.zeros((0, 3), np.float32))
    cell = torch.zeros(max(g.B, 1), 9, dtype=torch.float32, device='cuda')          # no cell: the molecules are not periodic
    ref = R.edge_embed_bwd(g, d['g_x'], d['g_u'], d['pos'], want_virial)
    shapes = {'g_d': (g.E, 4), 'forces': (g.N, 3)}
    if want_virial:
        shapes['virial'] = (g.B, 9)
    head = (ptr(g_x), ptr(g_u), ptr(dg.geo), ptr(disp), ptr(pos), ptr(cell), ptr(dg.row_ptr), ptr(dg.col), ptr(dg.rev), ptr(dg.mol_ptr),
            g.N, g.E, g.B, n_l, g.cutoff)
    mf = cfg()['molecule_forms']

    def form_of(small):
        if not want_virial and small and mol_small(g) and mf['force_direct']:      # launch_geometry_bwd (csrc/edge.hip:1113)
            return 'molecule-resident'
        return 'one launch' if not want_virial and g.E <= (1 << 20) else 'g_d, forces, virial'
    tail = lambda b: (ptr(b['g_d']), ptr(b['forces']), ptr(b['virial']) if want_virial else None)  # noqa: E731
    calls = [('plain', form_of(False), lambda b: L.nnhip_edge_embed_bwd(*head, *tail(b), _stream()))]
    for small in (False, True):
        o = opts_of(dg, small=small)
        calls.append((f'ex small_molecules={int(small)}', form_of(small),
                      lambda b, o=o: L.nnhip_edge_embed_bwd_ex(*head, *tail(b), C.byref(o), _stream())))
    first = None
    for tag, form, call in calls:
        what = f'{name} virial={int(want_virial)} {tag}'
        out = run_twice('edge_embed_bwd ' + what, shapes, call)
        for k in shapes:
            record(f'edge_embed_bwd {k}', form, out[k], ref[k], what)
        if first is not None:       # force_direct_mol_kernel: "bit for bit the row form's forces"
            assert torch.equal(bits(out['forces']), bits(first['forces'])), f'{what}: forces differ from the plain entry point'
        first = first or out


def head_out_case(name, act, tables, want_g=True):
    g, dg, d = graph(name)
    hip = _hip()
    L = hip.lib()
    e2, w4, b4, z = tin(d['e2']), tin(d['w4']), tin(d['b4']), tin(d['z'], torch.int64)
    scale, shift = (tin(d['scale']), tin(d['shift'])) if tables else (None, None)
    ref = R.head_out(d['e2'], d['w4'], d['b4'], d['scale'] if tables else None, d['shift'] if tables else None, d['z'], g.mol_ptr, act,
                     want_g)
    shapes = {'atom_energy': (g.N, 1), 'g_e2': (g.N, F), 'energy': (g.B, 1)}
    head = (ptr(e2), ptr(w4), ptr(b4), ptr(scale), ptr(shift), ptr(z), ptr(dg.mol_ptr), g.N, g.B, hip.ACTIVATION_IDS[act])
    tail = lambda b: (ptr(b['atom_energy']), ptr(b['g_e2']) if want_g else None, ptr(b['energy']))  # noqa: E731
    mf = cfg()['molecule_forms']
    calls = [('plain', 'rows, then molecule sums', lambda b: L.nnhip_head_out(*head, *tail(b), _stream()))]
    for small in (False, True):
        o = opts_of(dg, small=small)
        form = 'molecule-resident' if small and mol_small(g) and mf['head_out'] else 'rows, then molecule sums'   # csrc/edge.hip:1178
        calls.append((f'ex small_molecules={int(small)}', form, lambda b, o=o: L.nnhip_head_out_ex(*head, *tail(b), C.byref(o), _stream())))
    first = None
    for tag, form, call in calls:
        what = f'{name} act={act} tables={int(tables)} g_e2={int(want_g)} {tag}'
        out = run_twice('head_out ' + what, shapes, call)
        for k in shapes:
            record(f'head_out {k}', form, out[k], ref[k], what)
        if first is not None:       # head_out_mol_kernel: "the same arithmetic per atom ... bit for bit the same energies"
            for k in shapes:
                assert torch.equal(bits(out[k]), bits(first[k])), f'{what}: {k} differs from the plain entry point'
        first = first or out


# ---------------------------------------------------------------------------------------------------------------------------
# the group that the child processes repeat
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_group_message_stages(name):
    message_fwd_case(name)
    for need_gm in (1, 0):
        message_bwd_case(name, need_gm)
    message_bwd_force_tail_case(name)


@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_group_force_message_stages(name):
    for has_f in (True, False):
        for masked_xg in (True, False):
            force_message_fwd_case(name, has_f, masked_xg)
            force_message_bwd_case(name, has_f, masked_xg)


@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_group_edge_embed_bwd(name):
    for want_virial in (False, True):
        edge_embed_bwd_case(name, want_virial)


@pytest.mark.parametrize('name', ('degrees', 'molecules'))
def test_group_head_out(name):
    for act in D.ACTIVATIONS:
        for tables in (True, False):
            head_out_case(name, act, tables)
    head_out_case(name, 'silu', True, want_g=False)


def test_group_trivial_sizes():
    """one atom without edges: every row output is its start value and nothing else is touched; no atoms: NNHIP_OK, nothing
    touched"""
    for n in (1, 0):
        g = R.graph_trivial(n)
        _CACHE[f'trivial {n}'] = (g, DevGraph(g), R.stage_inputs(g))
        name = f'trivial {n}'
        message_fwd_case(name)
        for need_gm in (1, 0):
            message_bwd_case(name, need_gm)
        if n:                                    # (the force tail is refused without a molecule: tests/test_abi_host.py)
            message_bwd_force_tail_case(name)
        for has_f in (True, False):
            force_message_fwd_case(name, has_f, True)
            force_message_bwd_case(name, has_f, True)
        for want_virial in (False, True):
            edge_embed_bwd_case(name, want_virial)
        head_out_case(name, 'silu', True)


def built_graph():
    """a 12-atom geometry through hip.build_graph: its arrays must be the synthetic builder's for the same adjacency"""
    if 'built' in _CACHE:
        return
    hip = _hip()
    pos = R.geometry_positions()
    _, freq = R.filter_weights()
    gr = hip.build_graph(torch.from_numpy(pos).cuda(), torch.zeros(1, 3, 3, device='cuda'), torch.zeros(12, dtype=torch.int64, device='cuda'),
                         5.0, torch.from_numpy(freq).cuda())
    ei = gr.edge_index.cpu().numpy()
    g = R.stage_graph([(int(a), int(b)) for a, b in ei.T], [12], pos=pos)
    assert 0 < g.E < 12 * 11, 'the geometry should give an incomplete graph'
    twin = R.graph_geometry()                  # the graph the CPU tests of the bounds use: the same list, the same geometry
    assert np.array_equal(ei, twin.edge_index) and np.allclose(gr.geo.cpu().numpy(), twin.geo, rtol=0, atol=1e-6)
    for k in ('row_ptr', 'col', 'rev', 'pid', 'pair_ptr', 'mol_ptr'):
        assert np.array_equal(getattr(gr, k).cpu().numpy().reshape(-1), getattr(g, k)), f'build_graph and stage_graph differ in {k}'
    assert np.array_equal(ei, g.edge_index)
    g.geo, g.xg = gr.geo.cpu().numpy(), gr.xg.cpu().numpy().astype(np.int32)
    g.xg_live, g.masked = g.xg.copy(), g.xg[:, 0] == R.FT_ZERO_ROW
    assert not g.masked.any() and np.array_equal(g.geo[:, :3], -g.geo[g.rev, :3]) and np.array_equal(g.xg, g.xg[g.rev])
    d = R.stage_inputs(g)
    d['pos'] = pos
    _CACHE['built'] = (g, DevGraph(g), d)


def test_group_built_list():
    built_graph()
    name = 'built'
    message_fwd_case(name)
    for need_gm in (1, 0):
        message_bwd_case(name, need_gm)
    message_bwd_force_tail_case(name)
    for has_f in (True, False):
        force_message_fwd_case(name, has_f, True)
        force_message_bwd_case(name, has_f, True)
    for want_virial in (False, True):
        edge_embed_bwd_case(name, want_virial)
    head_out_case(name, 'silu', True)


# the forms each switch set is started for: (stage, form label) pairs that must have come up in the group above
EXPECTED_FORMS = {
    '': [('message_fwd a_mid', '4 waves per row'), ('message_bwd g_m', '4 waves per row, pair counts'),
         ('force_message_fwd f_out', '4 waves per row'), ('force_message_bwd g_fin', '4 waves per row, the owner writes g_u'),
         ('edge_embed_bwd forces', 'molecule-resident'), ('head_out energy', 'molecule-resident')],
    'NNHIP_EDGE_SMALL_ATOMS=0': [('message_fwd a_mid', '2 waves per row'), ('force_message_fwd f_out', '2 waves per row'),
                                 ('force_message_bwd g_fin', '1 waves per row, the owner writes g_u'),
                                 ('message_bwd g_m', '2 waves per row, pair counts')],
    'NNHIP_EDGE_WPR=1': [(s, '1 waves per row' + x) for s, x in (('message_fwd a_mid', ''), ('force_message_fwd f_out', ''),
                                                                   ('message_bwd g_m', ', pair counts'),
                                                                   ('force_message_bwd g_fin', ', the owner writes g_u'))],
    'NNHIP_EDGE_WPR=2': [(s, '2 waves per row' + x) for s, x in (('message_fwd a_mid', ''), ('force_message_fwd f_out', ''),
                                                                   ('message_bwd g_m', ', pair counts'),
                                                                   ('force_message_bwd g_fin', ', the owner writes g_u'))],
    'NNHIP_FORCE_BWD_OWNER_GU=0': [('force_message_bwd g_u', '4 waves per row, every row its own g_u')],
    'NNHIP_MOL_KERNELS_MIN=1': [('message_bwd g_m', 'molecule-resident'), ('message_bwd g_x pair sum', 'molecule-resident'),
                                ('message_bwd g_x pair sum', 'molecule-resident, with forces'),
                                ('message_bwd_ex forces', 'molecule-resident, with forces'),
                                ('force_message_fwd f_out', 'molecule-resident')],
    'NNHIP_MOL_KERNELS_MIN=1 NNHIP_MSG_BWD_FORCE=0': [('message_bwd g_m', 'molecule-resident'),
                                                      ('message_bwd g_x pair sum', 'molecule-resident'),
                                                      ('force_message_fwd f_out', 'molecule-resident')],
}
NEVER_FORMS = {
    '': ['molecule-resident, with forces'],
    'NNHIP_FORCE_BWD_OWNER_GU=0': ['4 waves per row, the owner writes g_u'],
    'NNHIP_MOL_KERNELS_MIN=1 NNHIP_MSG_BWD_FORCE=0': ['molecule-resident, with forces'],
}


def test_group_forms_of_this_process():
    """what nnhip_config says agrees with the switches the process was started with, and the labels of the forms this switch set
    is for came up in the cases above.  A label is the test's own restatement of the launcher's predicate on nnhip_config (module
    docstring): this checks that the switches lead where the table of the children says, not that a kernel of that name ran;
    only the force tail is reported by the library (tail_done) and compared in its case."""
    c = cfg()
    for tok in CHILD.split():
        k, v = tok.split('=')
        assert c['env'].get(k) == v, (k, c['env'])
    g = graph('molecules')[0]
    assert mol_pay(g) == ('NNHIP_MOL_KERNELS_MIN=1' in CHILD) and mol_small(g)
    if not RATIOS:                               # run on its own: the cases whose forms are looked at
        for name in ('degrees', 'molecules'):
            test_group_message_stages(name)
            test_group_force_message_stages(name)
            test_group_edge_embed_bwd(name)
            head_out_case(name, 'silu', True)
    reached = set(RATIOS)
    for pair in EXPECTED_FORMS[CHILD]:
        assert pair in reached, f'[{CHILD or "defaults"}] {pair} was not reached; reached: {sorted(reached)}'
    for form in NEVER_FORMS.get(CHILD, ()):
        assert not any(f == form for _, f in reached), f'[{CHILD or "defaults"}] {form} must not be reached'
    print('\nSTAGE-FORMS', CHILD or 'default switches', 'edge_rows', c['edge_rows'], 'molecule_forms', c['molecule_forms'])


def test_group_zz_ratio_summary():
    """the largest |got - ref| / bound per stage output and form of this process (every one was asserted <= 1 where it was taken)"""
    for (stage, form), v in sorted(RATIOS.items()):
        print(f'STAGE-SUMMARY {CHILD or "default"} | {stage} | {form} | {v:.3f}')


CHILDREN = (
    ('the shipped splits 2/2/1/2', {'NNHIP_EDGE_SMALL_ATOMS': '0'}),
    ('one wave per row', {'NNHIP_EDGE_WPR': '1'}),
    ('two waves per row', {'NNHIP_EDGE_WPR': '2'}),
    ('every force_bwd row its own g_u', {'NNHIP_FORCE_BWD_OWNER_GU': '0'}),
    ('molecule-resident forms', {'NNHIP_MOL_KERNELS_MIN': '1'}),
    ('molecule-resident forms without the force tail', {'NNHIP_MOL_KERNELS_MIN': '1', 'NNHIP_MSG_BWD_FORCE': '0'}),
)


@pytest.mark.skipif(bool(CHILD), reason='a child process does not start children')
@pytest.mark.parametrize('tag,env', CHILDREN)
def test_forms_in_child_processes(tag, env):
    """The group above once per switch set (read once per process: a child pytest each, under a timeout).  The child's cases name
    the form that serves each call and use that name in their STAGE-SUMMARY lines; test_group_forms_of_this_process asserts it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child_env = dict(os.environ, **env)
    child_env['NNHIP_EDGE_CHILD'] = ' '.join(f'{k}={v}' for k, v in env.items())
    try:
        r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-s', '-k', 'test_group'],
                           cwd=root, env=child_env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit(f'[{tag}] the child process hung (300 s): no further GPU work is started', returncode=3)
    out = (r.stdout or '') + (r.stderr or '')
    if r.returncode < 0 or r.returncode in ABNORMAL_RC or any(m in out for m in FAULT_MARKS):
        # a signal, an abort, a time limit or a kernel fault -- not a plain test failure: the other children launch the same
        # kernels and the rest of this file uses the same device, so the whole session ends here
        pytest.exit(f'[{tag}] the child process ended abnormally (return code {r.returncode}): no further GPU work is started\n'
                    + out[-3000:], returncode=3)
    for line in (r.stdout or '').splitlines():
        if 'STAGE-SUMMARY' in line or 'STAGE-FORMS' in line:
            print(line)
    tail = (r.stdout or '')[-3000:] + (r.stderr or '')[-1500:]
    assert r.returncode == 0, f'[{tag}] {tail}'          # (a plain test failure of the child: the `-x` child stopped at it)
    assert ' passed' in r.stdout and 'failed' not in r.stdout.splitlines()[-1], f'[{tag}] {tail}'


# ---------------------------------------------------------------------------------------------------------------------------
# stages without switches: embed, the tangent kernels, pair_rbf (one wave per row, csrc/train.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def tangent_cases(name):
    g, dg, d = graph(name) if name in R.GRAPHS else _CACHE[name]
    L, (tab, tab_h) = _hip().lib(), device_table()
    filt = R.TableFilter(tab_h, g.xg)
    form = 'one wave per row'
    t = {k: tin(v) for k, v in d.items() if v.dtype == np.float32}
    z = tin(d['z'], torch.int64)
    # embed
    out = run_twice(f'embed {name}', {'out': (g.N, F)}, lambda b: L.nnhip_embed(ptr(z), ptr(t['embedding']), g.N, ptr(b['out']), _stream()))
    record('embed out', 'copy', out['out'], R.embed(d['z'], d['embedding'])['out'], name)
    # edge_tangent_geom
    for sign in (-1.0, 0.75):
        out = run_twice(f'edge_tangent_geom {name}', {'tgeo': (g.E, 4)},
                        lambda b: L.nnhip_edge_tangent_geom(ptr(t['v']), sign, ptr(dg.edge_index), ptr(dg.geo), g.E, g.cutoff, ptr(b['tgeo']),
                                                            _stream()))
        record('edge_tangent_geom tgeo', 'one thread per edge', out['tgeo'], R.edge_tangent_geom(g, d['v'], sign)['tgeo'], f'{name} sign={sign}')
    csr = (ptr(dg.row_ptr), ptr(dg.col), ptr(dg.pid))
    for first_layer in (False, True):
        what = f'{name} first layer={int(first_layer)}'
        dm, da_in = (None, None) if first_layer else ('dm', 'da_in')
        P = lambda k: None if k is None else ptr(t[k])  # noqa: E731
        H = lambda k: None if k is None else d[k]  # noqa: E731
        out = run_twice('message_tan_fwd ' + what, {'dmsg': (g.P, F), 'da_mid': (g.N, F)},
                        lambda b: L.nnhip_message_tan_fwd(ptr(t['m']), P(dm), ptr(dg.xg), ptr(t['tgeo']), ptr(tab), *csr, P(da_in),
                                                          ptr(b['dmsg']), ptr(b['da_mid']), g.N, _stream()))
        ref = R.message_tan_fwd(g, filt, d['m'], d['tgeo'], H(dm), H(da_in))
        for k in ref:
            record(f'message_tan_fwd {k}', form, out[k], ref[k], what)
        out = run_twice('message_tan_bwd ' + what, {'dg_m': (g.N, F), 'g_eps': (g.P, F), 'dg_eps': (g.P, F)},
                        lambda b: L.nnhip_message_tan_bwd(ptr(t['g_msg']), ptr(t['dg_msg']), ptr(t['g_a']), ptr(t['dga']), ptr(t['m']), P(dm),
                                                          ptr(dg.xg), ptr(t['tgeo']), ptr(tab), *csr, ptr(b['dg_m']), ptr(b['g_eps']),
                                                          ptr(b['dg_eps']), g.N, _stream()))
        ref = R.message_tan_bwd(g, filt, d['g_msg'], d['dg_msg'], d['g_a'], d['dga'], d['m'], d['tgeo'], H(dm))
        for k in ref:
            record(f'message_tan_bwd {k}', form, out[k], ref[k], what)
        f_in, df_in = (None, None) if first_layer else ('f_in', 'df_in')
        out = run_twice('force_message_tan_fwd ' + what, {'df_out': (g.N, 3 * F)},
                        lambda b: L.nnhip_force_message_tan_fwd(ptr(t['phi1']), ptr(t['dphi1']), ptr(t['phi2']), ptr(t['dphi2']), ptr(dg.geo),
                                                                ptr(t['tgeo']), ptr(dg.xg), *csr, P(f_in), P(df_in), ptr(b['df_out']), g.N,
                                                                _stream()))
        ref = R.force_message_tan_fwd(g, d['phi1'], d['dphi1'], d['phi2'], d['dphi2'], d['tgeo'], H(f_in), H(df_in))
        record('force_message_tan_fwd df_out', form, out['df_out'], ref['df_out'], what)
        out = run_twice('force_message_tan_bwd ' + what, {'dg_h12': (g.P, 2 * F), 'dg_fin': (g.N, 3 * F)},
                        lambda b: L.nnhip_force_message_tan_bwd(ptr(t['gf']), ptr(t['dgf']), ptr(t['phi2']), ptr(t['dphi2']), ptr(dg.geo),
                                                                ptr(t['tgeo']), ptr(dg.xg), *csr, P(f_in), P(df_in), ptr(b['dg_h12']),
                                                                ptr(b['dg_fin']), g.N, _stream()))
        ref = R.force_message_tan_bwd(g, d['gf'], d['dgf'], d['phi2'], d['dphi2'], d['tgeo'], H(f_in), H(df_in))
        for k in ref:
            record(f'force_message_tan_bwd {k}', form, out[k], ref[k], what)
    out = run_twice(f'pair_rbf {name}', {'rb': (g.P, 64)},
                    lambda b: L.nnhip_pair_rbf(ptr(t['rbf']), ptr(t['drbf']), ptr(t['tgeo']), ptr(dg.edge_index), ptr(dg.pid), g.E, R.N_BASIS,
                                               ptr(b['rb']), _stream()))
    record('pair_rbf rb', 'one thread per entry', out['rb'], R.pair_rbf(g, d['rbf'], d['drbf'], d['tgeo'])['rb'], name)


@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_tangent_stages_embed_and_pair_rbf(name):
    tangent_cases(name)


def test_tangent_stages_on_the_built_list_and_trivial_sizes():
    built_graph()
    tangent_cases('built')
    for n in (1, 0):
        g = R.graph_trivial(n)
        _CACHE[f'trivial {n}'] = (g, DevGraph(g), R.stage_inputs(g))
        tangent_cases(f'trivial {n}')


def test_zz_ratio_summary():
    """the largest |got - ref| / bound per stage output and form over the whole file (printed; each was asserted where it was taken)"""
    for (stage, form), v in sorted(RATIOS.items()):
        print(f'STAGE-SUMMARY all | {stage} | {form} | {v:.3f}')
