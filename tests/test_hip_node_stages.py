"""The row-local node stages (csrc/node128.hip, csrc/node128s.hip), the four LayerNorm kernels (csrc/edge.hip, csrc/train.hip) and the
elementwise update tangents, each called DIRECTLY on independent random inputs and compared element by element with its float64
statement and componentwise bound (tests/node_ref.py): nnhip_node_fwd_ex / nnhip_node_bwd_ex (images: the split-f16 kernels; no
images: the fp32 ones), nnhip_node_turn, nnhip_node_tan_fwd / _bwd, nnhip_layer_norm_fwd / _bwd / _tan_fwd / _tan_bwd,
nnhip_update_tan_fwd / _bwd, nnhip_head_seed_tan, nnhip_direct_force / _bwd.

The harness is that of tests/test_hip_dense_stages.py: every output starts as a sentinel NaN and has 8 guard rows behind it that
must come back bit-identical; entries a variant leaves unwritten must still hold the sentinel; every case runs twice and must
repeat bit for bit; |got - ref| <= bound element by element.  Every output is held to two statements (node_ref.judge): the chained
one, and the one that takes the stored intermediate in front of it as an exact operand, so that every product is also judged
alone; the larger ratio counts.  The largest ratio per (stage, form) is printed as a `STAGE-RATIO` line per case and summed up in
`STAGE-SUMMARY` lines.  The cases are node_ref.node_cases(): the ones tests/test_node_ref_host.py holds the fp32 restatements to.

Rows: the node kernels tile 32 rows (1, 5, 31, 32, 33, 63, 97), the LayerNorm / update kernels take 4 rows per block
(1, 3, 4, 5, 33).  Rows whose largest magnitude lies below 2^-87 (an exponent field below 40) are not scaled by the split and are
flushed by design (csrc/mlp128s.hip: pow2_scale): the data edges keep their row maxima above it."""
import ctypes as C

import numpy as np
import pytest
import torch

from newtonnet_amd import abi
from tests import dense_ref as D
from tests import node_ref as R
from tests.test_hip_dense_stages import GUARD, OK, SENT, _stop_after_a_gpu_fault, mlp_kernel, weight_images  # noqa: F401  (the fixture is autouse here too)
from tests.test_hip_edge_stages import bits, blank, ptr, run_twice, tin

pytestmark = pytest.mark.gpu

F = R.F
E_INVALID = 1
RATIOS = {}
Images = abi.STRUCTS['nnhip_node_images']
_CACHE = {}
W3 = 3 * F


def _hip():
    from newtonnet_amd import hip
    return hip


def _stream():
    return _hip()._stream(torch.device('cuda', 0))


def act_id(name):
    return _hip().ACTIVATION_IDS[name]


def inputs(n, edge='plain'):
    """(host arrays, device tensors, the six images) of node_ref.node_inputs(n, edge)"""
    key = ('node', n, edge)
    if key not in _CACHE:
        t = R.node_inputs(n, edge)
        d = {k: tin(v) for k, v in t.items()}
        img = dict(zip(('Wu', 'W0', 'W2', 'W2T', 'W0T', 'WuT'), weight_images([d[k] for k in ('Wu', 'W0', 'W2', 'W2T', 'W0T', 'WuT')])))
        _CACHE[key] = (t, d, img)
    return _CACHE[key]


def images(img, **drop):
    """nnhip_node_images of the image tensors; name=None leaves a member out"""
    return Images(**{k: (None if k in drop else v.data_ptr()) for k, v in img.items()})


def host(bufs):
    return {k: v.detach().cpu() for k, v in bufs.items()}


def judge(stage, form, act, t, v, bufs, what, stored=None):
    """the outputs against node_ref.judge's two statements; entries left unwritten still the sentinel"""
    hb = host(bufs)
    refs = R.node_ref(stage, form, act, t, v)
    got = {}
    for k, b in hb.items():
        val, _, defined = refs[k]
        raw = b.view(torch.int32).numpy().reshape(val.shape)
        dd = np.broadcast_to(np.asarray(defined).reshape((-1,) + (1,) * (val.ndim - 1)), val.shape)
        assert (raw[~dd] == SENT).all(), f'{stage} [{form}] {what}: {k} was written where the variant leaves it alone'
        if dd.any():
            got[k] = b.double().numpy().reshape(val.shape)
            assert np.isfinite(got[k]).all(), f'{stage} [{form}] {what}: {k} not written / not finite'
    ratios = R.judge(stage, form, act, t, v, got, stored)
    worst = max(ratios.values()) if ratios else 0.0
    RATIOS[(stage, form)] = max(RATIOS.get((stage, form), 0.0), worst)
    print(f'STAGE-RATIO {stage} [{form}] {what}: {worst:.3f} ' + ' '.join(f'{k}={r:.3f}' for k, r in ratios.items()))
    assert worst <= 1.0, f'{stage} [{form}] {what}: |got - ref| / bound = {ratios}'
    return got


# ---------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------
def call_fwd(n, d, img, form, act, b, store_q=True, mlp=True, n_arg=None, act_arg=None, im=None):
    L = _hip().lib()
    im = im if im is not None else (images(img) if form == R.SPLIT else None)
    return L.nnhip_node_fwd_ex(ptr(d['f']), ptr(d['a_mid']), ptr(d['Wu']), ptr(b['q']) if store_q else None, ptr(b['a_out']),
                               ptr(d['W0']) if mlp else None, ptr(d['b0']), ptr(d['W2']) if mlp else None, ptr(d['b2']), ptr(b['hn']),
                               ptr(b['m']), n if n_arg is None else n_arg, act_id(act) if act_arg is None else act_arg,
                               C.byref(im) if im is not None else None, _stream())


def call_bwd(n, d, img, form, act, b, mlp=True, upd=True, acc=0, G_f=False, T=False, g_a_in=None, recompute=False, q=None,
             n_arg=None, act_arg=None, im=None, g_top=None, h_top=None, fill=True):
    L = _hip().lib()
    im = im if im is not None else (images(img) if form == R.SPLIT else None)
    if fill and n > 0:
        b['g_a'][:n] = d['g_a']                                   # in place: the running g_a
    gin = None if g_a_in is None else (b['g_a'] if g_a_in == 'same' else d['g_a_in'])
    return L.nnhip_node_bwd_ex(ptr(d['g_top'] if g_top is None else g_top), ptr(d['h_top'] if h_top is None else h_top),
                               ptr(d['W2T']) if mlp else None, ptr(d['W0T']) if mlp else None, ptr(b['g_a']), acc, ptr(d['f']),
                               None if recompute else ptr(d['q'] if q is None else q), ptr(d['G_f']) if G_f else None,
                               ptr(d['WuT']) if upd else None, ptr(b['gf']), ptr(b['T']) if T else None, ptr(gin),
                               n if n_arg is None else n_arg, act_id(act) if act_arg is None else act_arg,
                               C.byref(im) if im is not None else None, _stream())


def call_turn(n, d, img, b, scale=True, shift=True, n_arg=None, im=None):
    im = im if im is not None else images(img)
    return _hip().lib().nnhip_node_turn(ptr(d['f']), ptr(d['a_mid']), ptr(b['a_out']), ptr(d['b0']), ptr(d['b2']), ptr(d['w4']), ptr(d['b4']),
                                        ptr(d['scale']) if scale else None, ptr(d['shift']) if shift else None, ptr(d['z']),
                                        ptr(b['atom_energy']), ptr(b['g_a']), ptr(b['gf']), n if n_arg is None else n_arg, C.byref(im),
                                        _stream())


def call_tan_fwd(n, d, img, b, n_arg=None, im=None):
    im = im if im is not None else images(img)
    return _hip().lib().nnhip_node_tan_fwd(ptr(d['df']), ptr(d['f']), ptr(d['q']), ptr(d['da_mid']), ptr(d['hn']), ptr(b['dq']),
                                           ptr(b['da_out']), ptr(b['T']), ptr(b['Y']), n if n_arg is None else n_arg, C.byref(im), _stream())


def call_tan_bwd(n, d, img, b, A=True, B=True, t2=True, acc=0, dgf_in=False, n_arg=None, im=None):
    im = im if im is not None else images(img)
    if n > 0:
        b['dga'][:n] = d['dga']
    return _hip().lib().nnhip_node_tan_bwd(ptr(d['g_top']) if A else None, ptr(d['h_top']), ptr(d['t2_top']) if t2 else None,
                                           ptr(d['hd_top']) if t2 else None, ptr(b['G']), ptr(b['dga']), acc, ptr(d['ga']),
                                           ptr(d['f']) if B else None, ptr(d['df']), ptr(d['q']), ptr(d['dq']),
                                           ptr(d['dgf_in']) if dgf_in else None, ptr(b['gq']), ptr(b['dgq']), ptr(b['dgf']),
                                           n if n_arg is None else n_arg, C.byref(im), _stream())


SHAPES = {
    'node_fwd': lambda n: {'q': (n, W3), 'a_out': (n, F), 'hn': (n, F), 'm': (n, F)},
    'node_bwd': lambda n: {'g_a': (n, F), 'gf': (n, W3), 'T': (n, F)},
    'node_turn': lambda n: {'a_out': (n, F), 'atom_energy': (n, 1), 'g_a': (n, F), 'gf': (n, W3)},
    'node_tan_fwd': lambda n: {'dq': (n, W3), 'da_out': (n, F), 'T': (n, F), 'Y': (n, F)},
    'node_tan_bwd': lambda n: {'G': (n, F), 'dga': (n, F), 'gq': (n, W3), 'dgq': (n, W3), 'dgf': (n, W3)},
}


def composition(n, t, d, img, v):
    """nnhip_node_fwd_ex -> nnhip_head_out -> nnhip_node_bwd_ex on the inputs of node_turn: (outputs, what it stores in between)"""
    L = _hip().lib()
    fw = run_twice('turn: node_fwd', SHAPES['node_fwd'](n), lambda b: call_fwd(n, d, img, R.SPLIT, 'silu', b))
    mol_ptr = tin(np.array([0, n], np.int32))
    ho = run_twice('turn: head_out', {'atom_energy': (n, 1), 'g_e2': (n, F), 'energy': (1, 1)}, lambda b: L.nnhip_head_out(
        ptr(fw['m']), ptr(d['w4']), ptr(d['b4']), ptr(d['scale']) if v['scale'] else None, ptr(d['shift']) if v['shift'] else None,
        ptr(d['z']), ptr(mol_ptr), n, 1, act_id('silu'), ptr(b['atom_energy']), ptr(b['g_e2']), ptr(b['energy']), _stream()))
    bw = run_twice('turn: node_bwd', SHAPES['node_bwd'](n), lambda b: call_bwd(
        n, d, img, R.SPLIT, 'silu', b, g_top=ho['g_e2'], h_top=fw['hn'], q=fw['q'], fill=False))
    out = {'a_out': fw['a_out'], 'atom_energy': ho['atom_energy'], 'g_a': bw['g_a'], 'gf': bw['gf']}
    stored = {'a_out': fw['a_out'], 'e1': fw['hn'], 'e2': fw['m'], 'g_e2': ho['g_e2'], 'g_a': bw['g_a']}
    return out, {k: x.cpu().double().numpy() for k, x in stored.items()}


def run_case(stage, form, act, n, edge, name, v):
    t, d, img = inputs(n, edge)
    what = f'N={n} {act} {edge} {name}'
    if stage == 'node_fwd':
        bufs = run_twice(what, SHAPES[stage](n), lambda b: call_fwd(n, d, img, form, act, b, **v))
        if not v['store_q']:
            del bufs['q']                                      # (NULL was passed: nothing to look at)
        judge(stage, form, act, t, v, bufs, what)
    elif stage == 'node_bwd':
        bufs = run_twice(what, SHAPES[stage](n), lambda b: call_bwd(n, d, img, form, act, b, **v))
        if not v.get('T'):
            del bufs['T']
        if not v['mlp']:                                       # g_a is an input only: it must come back as it went in
            assert torch.equal(bits(bufs['g_a']), bits(d['g_a'])), what
        judge(stage, form, act, t, v, bufs, what)
        if v.get('recompute'):
            # q formed again from the f tile and the image of W_u = the bits node_fwd stores: both forms within their bound and equal
            fw = run_twice(what + ' (q)', SHAPES['node_fwd'](n), lambda b: call_fwd(n, d, img, form, act, b, mlp=False))
            vs = dict(v, recompute=False)
            stored_q = run_twice(what + ' (stored q)', SHAPES[stage](n), lambda b: call_bwd(n, d, img, form, act, b, q=fw['q'], **vs))
            del stored_q['T']
            tq = dict(t, q=fw['q'].cpu().numpy().reshape(n, 3, F))
            judge(stage, form, act, tq, vs, stored_q, what + ' (stored q)')
            for k in ('g_a', 'gf'):
                assert torch.equal(bits(stored_q[k]), bits(bufs[k])), f'{what}: {k} differs between the stored and the recomputed q'
    elif stage == 'node_turn':
        bufs = run_twice(what, SHAPES[stage](n), lambda b: call_turn(n, d, img, b, **v))
        comp, stored = composition(n, t, d, img, v)
        judge(stage, form, act, t, v, bufs, what, stored=stored)
        for k in bufs:
            assert torch.equal(bits(bufs[k]), bits(comp[k])), f'{what}: {k} differs from node_fwd -> head_out -> node_bwd'
    elif stage == 'node_tan_fwd':
        judge(stage, form, act, t, v, run_twice(what, SHAPES[stage](n), lambda b: call_tan_fwd(n, d, img, b)), what)
    else:
        bufs = run_twice(what, SHAPES[stage](n), lambda b: call_tan_bwd(n, d, img, b, **v))
        if not v['A']:
            assert torch.equal(bits(bufs['dga']), bits(d['dga'])), what
        judge(stage, form, act, t, v, bufs, what)


CASES = R.node_cases()


def _run(pred):
    todo = [c for c in CASES if pred(*c)]
    assert todo
    for c in todo:
        run_case(*c)


@pytest.mark.parametrize('n', R.NODE_ROWS)
@pytest.mark.parametrize('stage', tuple(SHAPES))
def test_node_stage_rows_and_variants(stage, n):
    _run(lambda s, form, act, nn, edge, name, v: s == stage and nn == n and edge == 'plain' and act == 'silu')


@pytest.mark.parametrize('act', D.ACTIVATIONS[1:])
def test_node_stages_fp32_every_activation(act):
    _run(lambda s, form, a, nn, edge, name, v: a == act)
    # the split form is SiLU only: refused, nothing written
    n = 33
    t, d, img = inputs(n)
    for stage, call in (('node_fwd', lambda b: call_fwd(n, d, img, R.SPLIT, act, b)), ('node_bwd', lambda b: call_bwd(n, d, img, R.SPLIT, act, b, fill=False))):
        refused(stage, n, call, f'{act} with images')


@pytest.mark.parametrize('edge', R.EDGES[1:])
def test_node_stages_data_edges(edge):
    _run(lambda s, form, act, nn, e, name, v: e == edge)


def refused(stage, n, call, what, shapes=None):
    L = _hip().lib()
    bufs = {k: blank(r, w) for k, (r, w) in (shapes or SHAPES[stage](n)).items()}
    rc = call(bufs)
    torch.cuda.synchronize()
    assert rc == E_INVALID, (stage, what, rc, L.nnhip_last_error())
    for k, b in bufs.items():
        assert bool((bits(b) == SENT).all()), f'{stage} {what}: {k} was written by a refused call'


def test_node_stages_refusals_and_zero_rows():
    """every pointer passed is a valid, fully sized device buffer: a missing check could not touch memory it does not own"""
    n = 33
    t, d, img = inputs(n)
    nofill = dict(fill=False)
    for form in (R.SPLIT, R.FP32):
        refused('node_fwd', n, lambda b: call_fwd(n, d, img, form, 'silu', b, n_arg=-1), f'{form} n_atoms < 0')
        refused('node_fwd', n, lambda b: call_fwd(n, d, img, form, 'silu', b, act_arg=9), f'{form} activation 9')
        refused('node_fwd', n, lambda b: call_fwd(n, d, img, form, 'silu', b, act_arg=-1), f'{form} activation -1')
        refused('node_bwd', n, lambda b: call_bwd(n, d, img, form, 'silu', b, n_arg=-1, **nofill), f'{form} n_atoms < 0')
        refused('node_bwd', n, lambda b: call_bwd(n, d, img, form, 'silu', b, act_arg=9, **nofill), f'{form} activation 9')
    refused('node_bwd', n, lambda b: call_bwd(n, d, img, R.FP32, 'silu', b, recompute=True, **nofill), 'fp32, no q')
    refused('node_bwd', n, lambda b: call_bwd(n, d, img, R.FP32, 'silu', b, T=True, **nofill), 'fp32 with T')
    refused('node_bwd', n, lambda b: call_bwd(n, d, img, R.SPLIT, 'silu', b, recompute=True, im=images(img, Wu=None), **nofill),
            'no q and no image of Wu')
    for miss in ('Wu', 'W0', 'W2'):
        refused('node_fwd', n, lambda b: call_fwd(n, d, img, R.SPLIT, 'silu', b, im=images(img, **{miss: None})), f'no image of {miss}')
        refused('node_tan_fwd', n, lambda b: call_tan_fwd(n, d, img, b, im=images(img, **{miss: None})), f'no image of {miss}')
    for miss in ('W2T', 'W0T', 'WuT'):
        refused('node_bwd', n, lambda b: call_bwd(n, d, img, R.SPLIT, 'silu', b, im=images(img, **{miss: None}), **nofill), f'no image of {miss}')
    for miss in img:
        refused('node_turn', n, lambda b: call_turn(n, d, img, b, im=images(img, **{miss: None})), f'no image of {miss}')
    refused('node_turn', n, lambda b: call_turn(n, d, img, b, n_arg=-1), 'n_atoms < 0')
    refused('node_tan_fwd', n, lambda b: call_tan_fwd(n, d, img, b, n_arg=-1), 'n_atoms < 0')
    L = _hip().lib()
    ln = ln_dev(n, 'plain')[1]
    lnb = {'a': (n, F), 'xhat': (n, F), 'rstd': (n, 1), 'w': (n, F), 'b': (n, F)}
    refused('layer_norm_fwd', n, lambda b: L.nnhip_layer_norm_fwd(ptr(b['a']), ptr(ln['gamma']), ptr(ln['beta']), -1, ptr(b['xhat']),
                                                                 ptr(b['rstd']), _stream()), 'n_atoms < 0', lnb)
    refused('layer_norm_bwd', n, lambda b: L.nnhip_layer_norm_bwd(ptr(b['a']), ptr(ln['gamma']), ptr(ln['xhat']), ptr(ln['rstd']), -1,
                                                                 _stream()), 'n_atoms < 0', lnb)
    refused('layer_norm_tan_fwd', n, lambda b: L.nnhip_layer_norm_tan_fwd(ptr(b['a']), ptr(ln['xhat']), ptr(ln['rstd']), ptr(ln['gamma']), -1,
                                                                         ptr(b['xhat']), ptr(b['rstd']), _stream()), 'n_atoms < 0', lnb)
    refused('layer_norm_tan_bwd', n, lambda b: L.nnhip_layer_norm_tan_bwd(
        ptr(ln['gy']), ptr(b['a']), ptr(ln['xhat']), ptr(ln['rstd']), ptr(ln['dxhat']), ptr(ln['drstd']), ptr(ln['gamma']), -1,
        ptr(b['w']), ptr(b['b']), _stream()), 'n_atoms < 0', lnb)

    # N = 0: NNHIP_OK, nothing written (the buffers are those of 33 rows)
    def nothing(stage, call, shapes=None):
        bufs = {k: blank(r, w) for k, (r, w) in (shapes or SHAPES[stage](n)).items()}
        rc = call(bufs)
        torch.cuda.synchronize()
        assert rc == OK, (stage, L.nnhip_last_error())
        for k, b in bufs.items():
            assert bool((bits(b) == SENT).all()), f'{stage} with N = 0 wrote {k}'
    for form in (R.SPLIT, R.FP32):
        nothing('node_fwd', lambda b: call_fwd(n, d, img, form, 'silu', b, n_arg=0))
        nothing('node_bwd', lambda b: call_bwd(n, d, img, form, 'silu', b, n_arg=0, **nofill))
    nothing('node_turn', lambda b: call_turn(n, d, img, b, n_arg=0))
    nothing('node_tan_fwd', lambda b: call_tan_fwd(n, d, img, b, n_arg=0))
    nothing('node_tan_bwd', lambda b: call_tan_bwd(0, d, img, b, n_arg=0))
    nothing('layer_norm_fwd', lambda b: L.nnhip_layer_norm_fwd(ptr(b['a']), ptr(ln['gamma']), ptr(ln['beta']), 0, ptr(b['xhat']), ptr(b['rstd']),
                                                              _stream()), lnb)
    nothing('layer_norm_bwd', lambda b: L.nnhip_layer_norm_bwd(ptr(b['a']), ptr(ln['gamma']), ptr(ln['xhat']), ptr(ln['rstd']), 0, _stream()), lnb)
    nothing('update_tan_fwd', lambda b: L.nnhip_update_tan_fwd(ptr(d['da_mid']), ptr(d['f']), ptr(d['df']), ptr(d['q']), ptr(d['dq']), 0,
                                                              ptr(b['a']), _stream()), lnb)


# ---------------------------------------------------------------------------------------------------------------------------
# one wave per row: LayerNorm and the update tangents
# ---------------------------------------------------------------------------------------------------------------------------
def ln_dev(n, edge):
    key = ('ln', n, edge)
    if key not in _CACHE:
        t = R.ln_inputs(n, edge)
        _CACHE[key] = (t, {k: tin(v) for k, v in t.items()})
    return _CACHE[key]


def wave_record(stage, bufs, ref, what):
    worst = 0.0
    for k, b in bufs.items():
        val = ref[k][0]
        g = (b.cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)).reshape(val.shape)
        assert np.isfinite(g).all(), f'{stage} {what}: {k} not written / not finite'
        worst = max(worst, R.worst_ratio(g, ref[k] if ref[k][2] is not None else (val, ref[k][1], np.ones(val.shape[0], bool))))
    RATIOS[(stage, R.FP32)] = max(RATIOS.get((stage, R.FP32), 0.0), worst)
    print(f'STAGE-RATIO {stage} [{R.FP32}] {what}: {worst:.3f}')
    assert worst <= 1.0, f'{stage} {what}: |got - ref| / bound = {worst:.3g}'


def ln_case(n, edge):
    L = _hip().lib()
    t, d = ln_dev(n, edge)
    what = f'N={n} {edge}'

    def fill(b, k, src):
        b[k][:n] = d[src]
        return b

    fw = run_twice(what, {'y': (n, F), 'xhat': (n, F), 'rstd': (n, 1)}, lambda b: L.nnhip_layer_norm_fwd(
        ptr(fill(b, 'y', 'x')['y']), ptr(d['gamma']), ptr(d['beta']), n, ptr(b['xhat']), ptr(b['rstd']), _stream()))
    wave_record('layer_norm_fwd', fw, R.ref_ln('layer_norm_fwd', t), what)
    bw = run_twice(what, {'g_x': (n, F)}, lambda b: L.nnhip_layer_norm_bwd(
        ptr(fill(b, 'g_x', 'g')['g_x']), ptr(d['gamma']), ptr(d['xhat']), ptr(d['rstd']), n, _stream()))
    wave_record('layer_norm_bwd', bw, R.ref_ln('layer_norm_bwd', t), what)
    tf = run_twice(what, {'dy': (n, F), 'dxhat': (n, F), 'drstd': (n, 1)}, lambda b: L.nnhip_layer_norm_tan_fwd(
        ptr(fill(b, 'dy', 'dx')['dy']), ptr(d['xhat']), ptr(d['rstd']), ptr(d['gamma']), n, ptr(b['dxhat']), ptr(b['drstd']), _stream()))
    wave_record('layer_norm_tan_fwd', tf, R.ref_ln('layer_norm_tan_fwd', t), what)
    tb = run_twice(what, {'dg_x': (n, F), 'row_w': (n, F), 'row_b': (n, F)}, lambda b: L.nnhip_layer_norm_tan_bwd(
        ptr(d['gy']), ptr(fill(b, 'dg_x', 'dgy')['dg_x']), ptr(d['xhat']), ptr(d['rstd']), ptr(d['dxhat']), ptr(d['drstd']), ptr(d['gamma']), n,
        ptr(b['row_w']), ptr(b['row_b']), _stream()))
    wave_record('layer_norm_tan_bwd', tb, R.ref_ln('layer_norm_tan_bwd', t), what)


@pytest.mark.parametrize('n', R.WAVE_ROWS)
def test_layer_norm_and_update_tangents(n):
    L = _hip().lib()
    for edge in (R.LN_EDGES if n == 33 else ('plain',)):
        ln_case(n, edge)
    t, d, _ = inputs(n)
    what = f'N={n}'
    uf = run_twice(what, {'da_out': (n, F)}, lambda b: L.nnhip_update_tan_fwd(
        ptr(d['da_mid']), ptr(d['f']), ptr(d['df']), ptr(d['q']), ptr(d['dq']), n, ptr(b['da_out']), _stream()))
    wave_record('update_tan_fwd', uf, R.update_tan_fwd(t['da_mid'], t['f'], t['df'], t['q'], t['dq']), what)
    for gin in (False, True):
        ub = run_twice(what, {'gq': (n, W3), 'dgq': (n, W3), 'dgf': (n, W3)}, lambda b: L.nnhip_update_tan_bwd(
            ptr(d['ga']), ptr(d['dga']), ptr(d['f']), ptr(d['df']), ptr(d['q']), ptr(d['dq']), ptr(d['dgf_in']) if gin else None, n,
            ptr(b['gq']), ptr(b['dgq']), ptr(b['dgf']), _stream()))
        wave_record('update_tan_bwd', ub, R.update_tan_bwd(t['ga'], t['dga'], t['f'], t['df'], t['q'], t['dq'], t['dgf_in'] if gin else None),
                    f'{what} dgf_in={int(gin)}')


@pytest.mark.parametrize('n', R.WAVE_ROWS)
def test_head_seed_tan(n):
    L = _hip().lib()
    t = R.head_seed_inputs(n)
    d = {k: tin(v) for k, v in t.items()}
    for act in (D.ACTIVATIONS if n == 33 else ('silu',)):
        for sc in (True, False):
            what = f'N={n} {act} scale={int(sc)}'
            bufs = run_twice(what, {'dg_e2': (n, F), 'w4row': (n, F), 'scal': (n, 4)}, lambda b: L.nnhip_head_seed_tan(
                ptr(d['e2']), ptr(d['de2']), ptr(d['w4']), ptr(d['b4']), ptr(d['scale']) if sc else None, ptr(d['z']), ptr(d['batch']),
                ptr(d['g_energy']), n, act_id(act), ptr(b['dg_e2']), ptr(b['w4row']), ptr(b['scal']), _stream()))
            wave_record('head_seed_tan', bufs, R.head_seed_tan(t['e2'], t['de2'], t['w4'], t['b4'], t['scale'] if sc else None, t['z'],
                                                               t['batch'], t['g_energy'], act), what)


def _rec(stage, got, ref, B, what):
    wave_record(stage, {'x': got}, {'x': (np.asarray(ref), np.asarray(B), None)}, what)


@pytest.mark.parametrize('n', R.WAVE_ROWS)
def test_direct_force_and_its_adjoint(n):
    """nnhip_direct_force leaves pre1 | pre2 | d3 in its scratch and nnhip_direct_force_bwd g_d3 | g_pre2 | t1 | g_pre1 in its work
    buffer: every product is judged from the stored operand in front of it (dense_ref.mlp / linear128), the two row kernels by
    node_ref.direct_force_tail / direct_force_adj"""
    hip = _hip()
    L = hip.lib()
    t = R.direct_force_inputs(n)
    d = {k: tin(v) for k, v in t.items()}
    nf = n * F
    for act in (D.ACTIVATIONS if n == 33 else ('silu',)):
        for sc in (True, False):
            what = f'N={n} {act} scale={int(sc)}'
            scale = t['scale'] if sc else None
            fw = run_twice(what, {'scratch': (3 * n, F), 'out': (n, 3)}, lambda b: L.nnhip_direct_force(
                ptr(d['atom_node']), ptr(d['f']), ptr(d['z']), ptr(d['w0']), ptr(d['b0']), ptr(d['w2']), ptr(d['b2']), ptr(d['w4']), ptr(d['b4']),
                ptr(d['scale']) if sc else None, act_id(act), n, ptr(b['scratch']), ptr(b['out']), _stream()))
            pre1, pre2, d3 = (fw['scratch'][k * n:(k + 1) * n].cpu().double().numpy() for k in range(3))
            form = mlp_kernel(n, act, False, True, 0, False)[1]
            m = D.mlp(D.MODE_FWD, t['atom_node'], t['w0'], t['w2'], act, form, b1=t['b0'], b2=t['b2'], H_got=pre1)
            _rec('direct_force', pre1, *m['H'], what + ' pre1')
            _rec('direct_force', pre2, *m['Y'], what + ' pre2')
            _rec('direct_force', d3, *D.linear128(pre2, t['w4'], bias=t['b4'], prologue=1, epilogue=1, activation=act), what + ' d3')
            wave_record('direct_force', {'out': fw['out']}, R.direct_force_tail(d3, t['f'], scale, t['z']), what)

            keep = fw['scratch'].contiguous()
            assert L.nnhip_direct_force_bwd_work_floats(n) == 4 * nf + 3 * F * F
            sp = torch.zeros(max(int(L.nnhip_species_scratch_bytes(4)), 4), dtype=torch.uint8, device='cuda')
            bw = run_twice(what, {'work': (4 * n + 3 * F, F), 'seed_a': (n, F), 'seed_f': (n, 3 * F), 'sc4': (n, 4), 'g_scale': (119, 1)},
                           lambda b: L.nnhip_direct_force_bwd(
                ptr(d['g_out']), ptr(d['f']), ptr(d['z']), ptr(d['w0']), ptr(d['w2']), ptr(d['w4']), ptr(d['scale']) if sc else None,
                act_id(act), n, ptr(keep), ptr(b['work']), ptr(b['seed_a']), ptr(b['seed_f']), ptr(b['sc4']), ptr(sp),
                ptr(b['g_scale']) if sc else None, _stream()))
            g_d3, g_pre2, t1, g_pre1 = (bw['work'][k * n:(k + 1) * n].cpu().double().numpy() for k in range(4))
            adj = R.direct_force_adj(t['g_out'], d3, t['f'], scale, t['z'])
            wave_record('direct_force_bwd', {'g_d3': bw['work'][:n], 'seed_f': bw['seed_f'], 'sc4': bw['sc4']}, adj, what)
            _rec('direct_force_bwd', g_pre2, *D.linear128(g_d3, t['w4'].T, H=pre2, epilogue=2, activation=act), what + ' g_pre2')
            form = mlp_kernel(n, act, False, False, 2, False)[1]
            m = D.mlp(D.MODE_TAN, g_pre2, t['w2'].T, t['w0'].T, act, form, H=pre1, T_got=t1)
            _rec('direct_force_bwd', t1, *m['T'], what + ' t1')
            _rec('direct_force_bwd', bw['seed_a'].cpu().double().numpy(), *m['Y'], what + ' seed_a')
            gp1 = t1 * D.dact(act, pre1)
            _rec('direct_force_bwd', g_pre1, gp1, np.abs(t1) * D.act_eval_err(pre1) + D.U * np.abs(gp1), what + ' g_pre1')
            if sc:
                sc4 = bw['sc4'].cpu().double().numpy()
                _rec('direct_force_bwd', bw['g_scale'].cpu().double().numpy(), *D.species_sum(sc4, t['z'], 0, 1), what + ' g_scale')
            else:
                assert bool((bits(bw['g_scale']) == SENT).all()), what


def test_species_across_the_table():
    """node_turn reads scale / shift by species: the cases cover both ends of the table"""
    z = R.node_inputs(33)['z']
    assert z.min() == 0 and z.max() == 118 and len(set(z.tolist())) >= 8


def test_zz_ratio_summary():
    for (stage, form), v in sorted(RATIOS.items()):
        print(f'STAGE-SUMMARY all | {stage} | {form} | {v:.3f}')
    assert all(v <= 1.0 for v in RATIOS.values())
