"""The dense and reduction stages the C interface exports one by one, each called DIRECTLY and compared element by element with
its float64 statement and componentwise bound (tests/dense_ref.py): nnhip_linear128, nnhip_mlp128_ex, nnhip_mlp128_pair_ex,
nnhip_wgrad_batch, nnhip_colsum_batch, nnhip_species_sum, nnhip_loss_grad / nnhip_mse_loss_grad, nnhip_clip_adam(_dev).

Every output buffer has 8 guard rows behind row M (and guard columns behind column 128 where the pitch is larger) holding a
sentinel NaN pattern that must come back bit-identical; rows the kernel has to write start as the same NaN, scratch / slab buffers
are NaN-filled, every case runs twice and must repeat bit for bit.  The row counts are the smallest at which a tiling decision
changes (1, 31, 32, 33, 95, 129, 1000 and the dispatch edges of csrc/mlp128.hip / csrc/lin128.hip).  The `test_group_*` tests
are run again in child processes with the form switches of the library set (test_forms_in_child_processes): the switches are
read once per process.  Every comparison prints the largest |got - ref| / bound it saw as a `DENSE-RATIO` line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dense_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FC5A5A5            # a quiet NaN with a payload: unwritten output rows fail every comparison, guards are compared as bits
GUARD = 8
OK, E_INVALID, E_UNSUPPORTED = 0, 1, 2
ROWS = (1, 31, 32, 33, 95, 129, 1000)
CHILD = os.environ.get('NNHIP_DENSE_CHILD', '')          # set by test_forms_in_child_processes
RATIOS = {}
ABNORMAL_RC = (124, 134, 137, 139)                       # time limit, abort, kill, segmentation fault
FAULT_MARKS = ('illegal memory', 'Memory access fault', 'hipError', 'HSA_STATUS_ERROR', 'unspecified launch failure')


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A kernel fault poisons the context for every later launch: when the device no longer answers after a test, the session
    ends there and nothing more is started on the GPU."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as exc:  # noqa: BLE001
        pytest.exit(f'the GPU does not answer after this test ({exc}): no further GPU work is started', returncode=3)


def _hip():
    from newtonnet_amd import hip
    return hip


def _seed(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


def _f32(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)).astype(np.float32)


def blank(M, ld=128):
    t = torch.empty(M + GUARD, ld, dtype=torch.float32, device='cuda')
    t.view(torch.int32).fill_(SENT)
    return t


def dev(a, ld=128):
    """host [M][w] -> device [M + GUARD][ld]; everything outside the M x w block is the sentinel"""
    a = np.ascontiguousarray(a, np.float32)
    t = blank(a.shape[0], ld)
    if a.size:
        t[:a.shape[0], :a.shape[1]] = torch.from_numpy(a).cuda()
    return t


def flat(a, dtype=torch.float32):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).to(dtype).cuda() if a.size else torch.zeros(1, dtype=dtype, device='cuda')


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def guards_intact(t, M, w=128):
    i = t.view(torch.int32)
    return bool((i[M:] == SENT).all()) and bool((i[:M, w:] == SENT).all())


def untouched(t):
    return bool((t.view(torch.int32) == SENT).all())


def host(t, M, w=128):
    return t[:M, :w].cpu().double().numpy()


def record(op, form, got, ref, B, what=''):
    """assert |got - ref| <= B element by element; keep and print the largest ratio seen per (operation, form)"""
    got, ref, B = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(B, np.float64)
    assert got.shape == ref.shape, (op, form, what, got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all(), f'{op} [{form}] {what}: {np.argwhere(~np.isfinite(got))[:4].tolist()} not written / not finite'
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(B > 0, err / B, np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    RATIOS[(op, form)] = max(RATIOS.get((op, form), 0.0), worst)
    print(f'DENSE-RATIO {op} [{form}] {what}: {worst:.3f}')
    if worst > 1.0:
        k = np.unravel_index(ratio.argmax(), ratio.shape)
        raise AssertionError(f'{op} [{form}] {what}: |got - ref| / bound = {worst:.3g} at {tuple(int(v) for v in k)} '
                             f'(got {got[k]!r}, ref {ref[k]!r}, bound {B[k]:.3g}); {int((ratio > 1).sum())} elements outside')
    return worst


def rows_ok(op, form, got, ref, tol, what=''):
    rel, spread = R.row_errors(got, ref)
    assert spread > 1e-3, f'{op} {what}: a reference row norm is {spread:.2e} of the median: pick another seed'
    print(f'DENSE-RATIO {op} rows [{form}] {what}: {rel.max() / tol:.3f}')
    RATIOS[(op + ' rows', form)] = max(RATIOS.get((op + ' rows', form), 0.0), float(rel.max() / tol))
    assert rel.max() <= tol, f'{op} [{form}] {what}: worst row {rel.max():.3e} > {tol} (row {int(rel.argmax())})'


# ---------------------------------------------------------------------------------------------------------------------------
# which kernel form serves a launch (csrc/mlp128.hip: mlp_use_wide, launch_mlp; csrc/mlp128r.hip: mlp_regw_serves)
# ---------------------------------------------------------------------------------------------------------------------------
def _wide_tiles(silu_split):
    env = int(os.environ.get('NNHIP_MLP_WIDE_TILES', '-1'))
    return env if env >= 0 else (832 if silu_split else 1536)


def mlp_kernel(M, act, images, biased, mode, acc, bf16=False, pair=None):
    """(name of the kernel form, product form of dense_ref, takes the one-pass register-weights kernel)"""
    hip = _hip()
    split, silu = hip.split_products(), act == 'silu'
    wide = -(-M // 32) <= _wide_tiles(split and silu) or biased
    if wide:
        s = bool(images) and silu and split
        name, form, onepass = ('row-local split-f16' if s else 'row-local fp32'), (R.SPLIT if s else R.FP32), False
    else:
        s = split and silu
        regw = (s and mode in (2, 3) and bool(images) and hip.mlp_forms()['regw_bwd']
                and os.environ.get('NNHIP_MLP_REGW_TRAIN', '1') != '0')
        onepass = regw and (not acc if pair is None else pair in ('shared_y', 'shared_x'))
        name = 'one-pass register-weights' if onepass else ('persistent split-f16' if s else 'persistent fp32')
        form = R.SPLIT if s else R.FP32
    if bf16:
        name, form = name + ' bf16', R.BF16
    return name, form, onepass


def weight_images(mats, bf16=False):
    hip = _hip()
    L = hip.lib()
    nb = L.nnhip_weight_image_bytes()
    imgs = [torch.zeros(nb, dtype=torch.uint8, device='cuda') for _ in mats]
    vp = C.c_void_p
    fn = L.nnhip_weight_images_bf16 if bf16 else L.nnhip_weight_images
    rc = fn((vp * len(mats))(*[m.data_ptr() for m in mats]), (vp * len(mats))(*[i.data_ptr() for i in imgs]), len(mats),
            hip._stream(mats[0].device))
    assert rc == OK, L.nnhip_last_error()
    return imgs


def mlp_inputs(M, mode, bias, acc, key):
    rng = np.random.default_rng(_seed('mlp', M, mode, bias, acc, key))
    d = dict(X=_f32(rng, M, 128), W1=_f32(rng, 128, 128, scale=1 / 11), W2=_f32(rng, 128, 128, scale=1 / 11))
    if mode != 0:
        d['H'] = _f32(rng, M, 128)
    if mode == 3:
        d['T2'], d['Hd'] = _f32(rng, M, 128), _f32(rng, M, 128)
    if bias:                                   # True: both; 'b1' / 'b2': that one alone
        b1, b2 = _f32(rng, 128), _f32(rng, 128)
        if bias in (True, 'b1'):
            d['b1'] = b1
        if bias in (True, 'b2'):
            d['b2'] = b2
    if acc:
        d['Y0'] = _f32(rng, M, 128)
    return d


class MlpLaunch:
    """device buffers and the descriptor of one nnhip_mlp_desc"""
    OUT = {0: ('H', 'Y'), 1: ('Y',), 2: ('T', 'Y'), 3: ('G', 'Y')}

    def __init__(self, inp, M, mode, act, ld=(128, 128, 128), acc=False, images=None, precision=0, share=None):
        hip = _hip()
        ldx, ldh, ldy = ld
        self.M, self.mode, self.ld, self.keep = M, mode, ld, []
        share = share or {}
        t = {'X': share.get('X') if 'X' in share else dev(inp['X'], ldx)}
        for name in ('W1', 'W2', 'b1', 'b2'):
            t[name] = flat(inp[name]) if name in inp else None
        for name in ('H', 'T2', 'Hd'):
            t[name] = dev(inp[name], ldh) if (name in inp and not (name == 'H' and mode == 0)) else None
        if mode == 0:
            t['H'] = blank(M, ldh)
        t['T'] = blank(M, ldh) if mode == 2 else None
        t['G'] = blank(M, ldh) if mode == 3 else None
        t['Y'] = share['Y'] if 'Y' in share else (dev(inp['Y0'], ldy) if acc and 'Y0' in inp else blank(M, ldy))
        self.t = t
        d = hip.MlpDesc()
        for name in ('X', 'W1', 'W2', 'b1', 'b2', 'H', 'Y', 'T', 'T2', 'Hd', 'G'):
            setattr(d, name, None if t[name] is None else t[name].data_ptr())
        d.ldx, d.ldh, d.ldy, d.M, d.mode, d.accumulate = ldx, ldh, ldy, M, mode, 1 if acc else 0
        d.activation, d.precision = hip.ACTIVATION_IDS[act], precision
        if images:
            d.W1_image, d.W2_image = images[0].data_ptr(), images[1].data_ptr()
            self.keep.append(images)
        self.desc = d

    def outputs(self):
        return {n: self.t[n] for n in self.OUT[self.mode]}

    def check_guards(self, what):
        for n, buf in self.outputs().items():
            assert guards_intact(buf, self.M), f'{what}: a guard row / column of {n} was written'


def run_single(inp, M, mode, act, ld, acc, images=None, precision=0):
    hip = _hip()
    la = MlpLaunch(inp, M, mode, act, ld, acc, images, precision)
    rc = hip.lib().nnhip_mlp128_ex(C.byref(la.desc), hip._stream(torch.device('cuda', 0)))
    torch.cuda.synchronize()
    return rc, la


def mlp_reference(inp, mode, act, form, la=None, Y0=None):
    """the float64 outputs and bounds; `la`: the launch whose stored H / T / G feed the second product (dense_ref.mlp)"""
    got = {n: host(la.t[n], la.M) for n in ('H', 'T', 'G') if la is not None and n in la.outputs()}
    return R.mlp(mode, inp['X'], inp['W1'], inp['W2'], act, form, H=inp.get('H'), b1=inp.get('b1'), b2=inp.get('b2'),
                 T2=inp.get('T2'), Hd=inp.get('Hd'), Y0=Y0, H_got=got.get('H'), T_got=got.get('T'), G_got=got.get('G'))


def check_mlp(op, kname, form, la, ref, what):
    M = la.M
    for n, buf in la.outputs().items():
        record(f'{op} mode {la.mode} {n}', kname, host(buf, M), ref[n][0], ref[n][1], what)
    tol = R.ROW_TOL_BF16 if form == R.BF16 else R.ROW_TOL
    if la.mode == 0 and M:
        rows_ok(f'{op} mode 0 Y', kname, host(la.t['Y'], M), ref['Y'][0], tol, what)
    if la.mode == 3 and M:
        rows_ok(f'{op} mode 3 G', kname, host(la.t['G'], M), ref['G'][0], tol, what)


def onepass_count(fn):
    """run fn() and return how many launches of the 'mlp_onepass' timer class it made"""
    hip = _hip()
    hip.timers_read(reset=True)
    hip.timers_enable(True, classes=('mlp_onepass',))
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        hip.timers_enable(False)
    return hip.timers_read(reset=True)['mlp_onepass'][1], out


def mlp_case(M, mode, act, ld=(128, 128, 128), acc=False, bias=False, images=False, bf16=False, key=0):
    """one nnhip_mlp128_ex case: twice, bit-equal, guards, bound of the form that serves it, the form asserted"""
    hip = _hip()
    inp = mlp_inputs(M, mode, bias, acc, key)
    imgs = None
    if images or bf16:
        w = [flat(inp['W1']), flat(inp['W2'])]
        imgs = weight_images(w, bf16=bf16)
    kname, form, onepass = mlp_kernel(M, act, imgs is not None, bool(bias), mode, acc, bf16)
    what = f'M={M} act={act} ld={ld} acc={int(acc)} bias={bias} images={int(images)}'
    n_bf = hip.bf16_mlp_launches()
    n_one, (rc, la) = onepass_count(lambda: run_single(inp, M, mode, act, ld, acc, imgs, 1 if bf16 else 0))
    assert rc == OK, (what, hip.lib().nnhip_last_error())
    assert n_one == (1 if onepass and M else 0), f'{what}: expected {kname}, the one-pass timer class counted {n_one}'
    assert hip.bf16_mlp_launches() - n_bf == (1 if bf16 and M else 0), what
    la.check_guards(what)
    rc2, lb = run_single(inp, M, mode, act, ld, acc, imgs, 1 if bf16 else 0)
    assert rc2 == OK
    for n in la.outputs():
        assert torch.equal(bits(la.t[n]), bits(lb.t[n])), f'{what}: {n} differs between two runs'
    ref = mlp_reference(inp, mode, act, form, la, inp.get('Y0'))
    check_mlp('mlp128_ex', kname, form, la, ref, what)
    if bf16 and M:
        # the launch counter advances before the dispatch: that operands were really rounded to bf16 shows in the result -- the
        # first output must leave the split-f16 bound somewhere (a launch that quietly ran at full precision stays inside it)
        n = la.OUT[mode][0]
        fine = mlp_reference(inp, mode, act, R.SPLIT, la, inp.get('Y0'))[n]
        over = float((np.abs(host(la.t[n], M) - fine[0]) / fine[1]).max())
        print(f'DENSE-RATIO mlp128_ex mode {mode} {n} [{kname}] against the split-f16 bound: {over:.1f}')
        assert over > 4.0, f'{what}: {n} is within {over:.2f} x the split-f16 bound: the bf16 form did not run'
    return la


def _pitches(k):
    return ((128, 128, 128), (160, 128, 128), (128, 160, 128), (128, 128, 160), (160, 160, 160))[k % 5]


# ---------------------------------------------------------------------------------------------------------------------------
# the group that the child processes repeat: nnhip_linear128, nnhip_mlp128_ex, nnhip_mlp128_pair_ex
# ---------------------------------------------------------------------------------------------------------------------------
LIN_PAIRS = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1))


def lin_case(M, pro, epi, lda=128, ldc=128, ldh=128, alias=False):
    hip = _hip()
    L = hip.lib()
    rng = np.random.default_rng(_seed('lin', M, pro, epi, lda, ldc, ldh, alias))
    A, W = _f32(rng, M, 128), _f32(rng, 128, 128, scale=1 / 11)
    bias, H, C0 = _f32(rng, 128), _f32(rng, M, 128), _f32(rng, M, 128)
    if alias:
        ldc = lda
        C0 = A                                   # (EPI_ACC with C aliasing A: C = A + A W^T)
    kname = 'row-local fp32' if (pro == 0 and epi in (0, 3) and M <= 32 * 1536) else 'persistent fp32'
    what = f'M={M} pro={pro} epi={epi} lda={lda} ldc={ldc} ldh={ldh} alias={int(alias)}'
    ref, B = R.linear128(A, W, bias, H, C0, pro, epi)
    outs = []
    for _ in range(2):
        Ad, Wd, bd, Hd = dev(A, lda), flat(W), flat(bias), dev(H, ldh)
        Cd = Ad if alias else (dev(C0, ldc) if epi == 3 else blank(M, ldc))
        rc = L.nnhip_linear128(Ad.data_ptr(), lda, Wd.data_ptr(), Cd.data_ptr(), ldc, bd.data_ptr(), Hd.data_ptr(), ldh, M, pro, epi,
                               hip._stream(Ad.device))
        torch.cuda.synchronize()
        assert rc == OK, (what, L.nnhip_last_error())
        assert guards_intact(Cd, M), f'{what}: a guard row / column of C was written'
        outs.append(Cd)
    assert torch.equal(bits(outs[0]), bits(outs[1])), f'{what}: two runs differ'
    record(f'linear128 pro {pro} epi {epi}', kname, host(outs[0], M), ref, B, what)


@pytest.mark.parametrize('M', ROWS + (49152, 49153))
def test_group_linear128(M):
    """all six prologue / epilogue pairs launch_lin serves, pitches 128 and 160, C aliasing A exactly, EPI_ACC onto a non-zero C;
    49 152 / 49 153: the row-local form hands over to the persistent one (csrc/lin128.hip:241)"""
    for k, (pro, epi) in enumerate(LIN_PAIRS):
        lin_case(M, pro, epi)
        lin_case(M, pro, epi, lda=160 if k % 2 == 0 else 128, ldc=160 if k % 3 != 1 else 128, ldh=160)
        lin_case(M, pro, epi, lda=160 if k % 2 else 128, alias=True)


def test_group_linear128_more_tiles_than_one_trip():
    """2048 tiles + 5 rows: more than the 512 workgroups x 4 waves of the persistent linear take in one trip, ragged last tile"""
    lin_case(2048 * 32 + 5, 0, 2)
    lin_case(2048 * 32 + 5, 1, 1, lda=160, ldc=160)


def test_group_linear128_refusals_and_zero_rows():
    hip = _hip()
    L = hip.lib()
    rng = np.random.default_rng(3)
    A, W = dev(_f32(rng, 33, 128)), flat(_f32(rng, 128, 128))
    bias, H = flat(_f32(rng, 128)), dev(_f32(rng, 33, 128))
    st = hip._stream(A.device)
    for pro, epi in ((1, 2), (1, 3), (2, 0), (0, 4)):        # the pairs launch_lin does not serve
        Cd = blank(33)
        rc = L.nnhip_linear128(A.data_ptr(), 128, W.data_ptr(), Cd.data_ptr(), 128, bias.data_ptr(), H.data_ptr(), 128, 33, pro, epi, st)
        torch.cuda.synchronize()
        assert rc == E_INVALID, (pro, epi, rc)
        assert untouched(Cd), (pro, epi)
    for pro, epi in LIN_PAIRS:                               # M = 0: NNHIP_OK, nothing touched
        Cd = blank(0)
        rc = L.nnhip_linear128(A.data_ptr(), 128, W.data_ptr(), Cd.data_ptr(), 128, bias.data_ptr(), H.data_ptr(), 128, 0, pro, epi, st)
        torch.cuda.synchronize()
        assert rc == OK and untouched(Cd), (pro, epi, rc)


def _mlp_sweep(M, act, k0=0):
    """modes 0 .. 3, accumulate 0 / 1 in modes 1 .. 3, biases in mode 0, every pitch pattern, with and without images (SiLU)"""
    k = k0
    for images in ((False, True) if act == 'silu' else (False,)):
        for mode in (0, 1, 2, 3):
            for acc in ((False,) if mode == 0 else (False, True)):
                mlp_case(M, mode, act, _pitches(k), acc, bias=False, images=images)
                k += 1
        for bias in (True, 'b1', 'b2'):
            mlp_case(M, 0, act, _pitches(k), bias=bias, images=images)
            k += 1


@pytest.mark.parametrize('act', ('silu', 'tanh', 'softplus', 'relu'))
@pytest.mark.parametrize('M', ROWS)
def test_group_mlp128_ex(M, act):
    _mlp_sweep(M, act, k0=M)


@pytest.mark.parametrize('act', ('elu', 'leaky_relu', 'sigmoid', 'gelu', 'ssp'))
def test_group_mlp128_ex_other_activations(act):
    _mlp_sweep(33, act)


def test_group_mlp128_ex_more_tiles_than_one_trip():
    """32 * 1024 + 5 rows with the persistent forms forced: more tiles than 256 workgroups x 4 waves take in one trip, ragged
    last tile.  (At the default switches this row count is the persistent split form's for SiLU and the row-local one's for tanh.)"""
    M = 32 * 1024 + 5
    for act in ('silu', 'tanh'):
        for images in ((False, True) if act == 'silu' else (False,)):
            for mode in (0, 1, 2, 3):
                mlp_case(M, mode, act, _pitches(mode + 1), acc=(mode == 1), images=images)
            for bias in ('b1', 'b2'):        # one bias alone sends the launch to the row-local form at any M (mlp_use_wide)
                mlp_case(M, 0, act, _pitches(3), bias=bias, images=images)


@pytest.mark.parametrize('M', (26624, 26625))
@pytest.mark.parametrize('images', (False, True))
def test_group_mlp128_ex_split_edge(M, images):
    """832 tiles: with images the row-local split-f16 kernel hands over to the persistent split one, without them the row-local
    fp32 kernel does (csrc/mlp128.hip: MLPS_WIDE_MAX_TILES)"""
    for mode in (0, 1, 2, 3):
        mlp_case(M, mode, 'silu', _pitches(mode), acc=(mode == 2), images=images)


@pytest.mark.parametrize('M', (49152, 49153))
def test_group_mlp128_ex_fp32_edge(M):
    """1536 tiles: the row-local fp32 kernel hands over to the persistent fp32 one for the non-SiLU activations"""
    for mode in (0, 1, 2, 3):
        mlp_case(M, mode, 'tanh', _pitches(mode + 2), acc=(mode == 3))


@pytest.mark.parametrize('M', (33, 1000))
def test_group_mlp128_ex_bf16(M):
    """precision = 1 with nnhip_weight_images_bf16: 2^-9 operands, fp32 accumulation; the launch counter advances by one"""
    hip = _hip()
    if not hip.split_products():
        rc, la = run_single(mlp_inputs(M, 0, False, False, 0), M, 0, 'silu', (128, 128, 128), False,
                            weight_images([torch.zeros(128, 128, device='cuda')] * 2, bf16=True), 1)
        assert rc == E_UNSUPPORTED and all(untouched(b) for b in la.outputs().values())   # (csrc/mlp128.hip:508)
        return
    for mode in (0, 1, 2, 3):
        mlp_case(M, mode, 'silu', _pitches(mode), acc=(mode == 1), bf16=True)


def test_group_mlp128_ex_refusals_and_zero_rows():
    hip = _hip()
    L = hip.lib()
    st = hip._stream(torch.device('cuda', 0))
    M = 33
    img = weight_images([torch.zeros(128, 128, device='cuda')] * 2)
    img_bf = weight_images([torch.zeros(128, 128, device='cuda')] * 2, bf16=True)

    def refused(code, mode=0, act='silu', ld=(128, 128, 128), bias=False, images=None, precision=0, one_image=False):
        la = MlpLaunch(mlp_inputs(M, mode, bias, False, 1), M, mode, act, (128, 128, 128), False, images, precision)
        la.desc.ldx, la.desc.ldh, la.desc.ldy = ld            # (refused before anything is read: the buffers keep pitch 128)
        if one_image:
            la.desc.W2_image = None
        rc = L.nnhip_mlp128_ex(C.byref(la.desc), st)
        torch.cuda.synchronize()
        assert rc == code, (rc, mode, act, ld, bias, precision, one_image)
        assert all(untouched(b) for b in la.outputs().values()), 'a refused launch wrote'
    for mode in (1, 2, 3):
        refused(E_INVALID, mode=mode, bias=True)                        # biases belong to mode 0
    refused(E_INVALID, images=img, one_image=True)                      # one image without the other
    refused(E_UNSUPPORTED, images=img_bf, precision=1, bias=True)       # bf16 mode: bias-free ...
    refused(E_UNSUPPORTED, images=img_bf, precision=1, act='tanh')      # ... SiLU ...
    refused(E_UNSUPPORTED, precision=1)                                 # ... with images
    refused(E_INVALID, precision=2)
    for ld in ((130, 128, 128), (128, 134, 128), (128, 128, 142), (124, 128, 128)):
        refused(E_INVALID, ld=ld)                                       # pitches: multiples of 4, >= 128
    n_bf = hip.bf16_mlp_launches()
    for mode in (0, 1, 2, 3):                                            # M = 0: NNHIP_OK, nothing touched
        for images, prec in ((None, 0), (img, 0), (img_bf, 1)):
            if prec and not hip.split_products():
                continue
            la = MlpLaunch(mlp_inputs(0, mode, False, False, 2), 0, mode, 'silu', (128, 128, 128), False, images, prec)
            rc = L.nnhip_mlp128_ex(C.byref(la.desc), st)
            torch.cuda.synchronize()
            assert rc == OK and all(untouched(b) for b in la.outputs().values()), (mode, prec, rc)
    assert hip.bf16_mlp_launches() == n_bf


PAIR_SHAPES = (('shared_x', 0), ('shared_x', 2), ('shared_y', 1), ('shared_y', 2), ('shared_y', 3), ('independent', 0),
               ('independent', 1))


def pair_case(M, shape, mode, images, ld=(128, 128, 128)):
    """nnhip_mlp128_pair_ex in the three shapes the model produces, against the bound and against the two single launches"""
    hip = _hip()
    L = hip.lib()
    st = hip._stream(torch.device('cuda', 0))
    act = 'silu'
    i0, i1 = mlp_inputs(M, mode, False, False, ('p0', shape)), mlp_inputs(M, mode, False, False, ('p1', shape))
    if shape == 'shared_x':
        i1['X'] = i0['X']
    imgs = [weight_images([flat(i['W1']), flat(i['W2'])]) if images else None for i in (i0, i1)]
    acc1 = shape == 'shared_y'
    what = f'pair {shape} M={M} mode={mode} images={int(images)} ld={ld}'

    def launch(pair):
        a = MlpLaunch(i0, M, mode, act, ld, False, imgs[0])
        share = {'X': a.t['X']} if shape == 'shared_x' else ({'Y': a.t['Y']} if shape == 'shared_y' else {})
        b = MlpLaunch(i1, M, mode, act, ld, acc1, imgs[1], share=share)
        if pair:
            rc = L.nnhip_mlp128_pair_ex(C.byref(a.desc), C.byref(b.desc), st)
        else:
            rc = L.nnhip_mlp128_ex(C.byref(a.desc), st) or L.nnhip_mlp128_ex(C.byref(b.desc), st)
        torch.cuda.synchronize()
        assert rc == OK, (what, pair, L.nnhip_last_error())
        a.check_guards(what)
        b.check_guards(what)
        return a, b
    kname, form, onepass = mlp_kernel(M, act, images, False, mode, acc1, pair=shape)
    n_one, (a, b) = onepass_count(lambda: launch(True))
    assert n_one == (1 if onepass else 0), f'{what}: expected {kname}, the one-pass timer class counted {n_one}'
    a2, b2 = launch(True)
    sa, sb = launch(False)
    s_one = [mlp_kernel(M, act, images, False, mode, acc)[2] for acc in (False, acc1)]
    same_form = not onepass and not any(s_one)
    for x, x2, s, tag in ((a, a2, sa, 'first'), (b, b2, sb, 'second')):
        for n in x.outputs():
            assert torch.equal(bits(x.t[n]), bits(x2.t[n])), f'{what}: {tag} {n} differs between two runs'
            if same_form:
                assert torch.equal(bits(x.t[n]), bits(s.t[n])), f'{what}: {tag} {n} differs from the single launches ({kname})'
    r0 = mlp_reference(i0, mode, act, form, a)
    if shape == 'shared_y':           # Y = the first MLP's result + the second's; the first's bound rides along
        r1 = mlp_reference(i1, mode, act, form, b, Y0=r0['Y'][0])
        r1['Y'] = (r1['Y'][0], r1['Y'][1] + r0['Y'][1])
        for n in a.outputs():
            if n != 'Y':
                record(f'mlp128_pair_ex mode {mode} {n}', kname, host(a.t[n], M), r0[n][0], r0[n][1], what)
    else:
        r1 = mlp_reference(i1, mode, act, form, b)
        check_mlp('mlp128_pair_ex', kname, form, a, r0, what)
    check_mlp('mlp128_pair_ex', kname, form, b, r1, what)
    if not same_form:                 # another form served the singles: they agree within the bound as well
        rs0 = mlp_reference(i0, mode, act, form, sa)
        rs1 = mlp_reference(i1, mode, act, form, sb, Y0=rs0['Y'][0] if shape == 'shared_y' else None)
        if shape == 'shared_y':
            rs1['Y'] = (rs1['Y'][0], rs1['Y'][1] + rs0['Y'][1])
        if shape != 'shared_y':           # (shared Y: the first launch's Y is the shared buffer, judged through the second)
            check_mlp('mlp128_pair_ex (singles)', 'singles next to ' + kname, form, sa, rs0, what)
        check_mlp('mlp128_pair_ex (singles)', 'singles next to ' + kname, form, sb, rs1, what)


@pytest.mark.parametrize('M', ROWS)
def test_group_mlp128_pair_ex(M):
    for k, (shape, mode) in enumerate(PAIR_SHAPES):
        for images in (False, True):
            pair_case(M, shape, mode, images, ld=_pitches(k + M) if shape == 'independent' else (128, 128, 128))


def test_group_mlp128_pair_ex_large():
    """above every row-local limit at the default switches (26 625 rows: the persistent forms) and, in the forced-persistent
    children, more tiles than one trip"""
    M = 32 * 1024 + 5 if 'WIDE_TILES' in CHILD else 26625
    for shape, mode in PAIR_SHAPES:
        pair_case(M, shape, mode, images=True)
    pair_case(M, 'shared_y', 1, images=False)


def test_group_mlp128_pair_ex_refusals():
    hip = _hip()
    L = hip.lib()
    st = hip._stream(torch.device('cuda', 0))

    def refused(ma, mb):
        rc = L.nnhip_mlp128_pair_ex(C.byref(ma.desc), C.byref(mb.desc), st)
        torch.cuda.synchronize()
        assert rc == E_INVALID, rc
        assert all(untouched(t) for m in (ma, mb) for t in m.outputs().values())
    mk = lambda M=33, mode=1, act='silu', acc=False: MlpLaunch(mlp_inputs(M, mode, False, False, 5), M, mode, act, acc=acc)  # noqa: E731
    refused(mk(), mk(M=32))
    refused(mk(), mk(mode=2))
    refused(mk(), mk(act='tanh'))
    refused(mk(acc=True), mk())
    a, b = mk(M=0), mk(M=0)                                   # M = 0: NNHIP_OK, nothing touched
    assert L.nnhip_mlp128_pair_ex(C.byref(a.desc), C.byref(b.desc), st) == OK
    torch.cuda.synchronize()
    assert all(untouched(t) for m in (a, b) for t in m.outputs().values())


def test_group_forms_of_this_process():
    """what the library says about the forms of this process agrees with the switches the process was started with"""
    hip = _hip()
    cfg, forms = hip.config(), hip.mlp_forms()
    split = os.environ.get('NNHIP_MLP_SPLIT', '1') != '0'
    assert hip.split_products() == split and bool(cfg['split_f16_products']) == split and forms['split'] == split
    assert cfg['edge_mlp']['row_local_up_to_tiles'] == _wide_tiles(split)
    for name in ('NNHIP_MLP_WIDE_TILES', 'NNHIP_MLP_SPLIT', 'NNHIP_MLP_REGW_TRAIN'):
        if name in os.environ:
            assert cfg['env'].get(name) == os.environ[name], (name, cfg['env'])
    print('\nDENSE-FORMS', CHILD or 'default switches', 'split', split, 'row_local_up_to_tiles', cfg['edge_mlp']['row_local_up_to_tiles'],
          'one_pass_adjoint', forms['regw_bwd'], 'kernels:', sorted({k[1] for k in RATIOS}))


def test_group_zz_ratio_summary():
    """the largest |got - ref| / bound per operation and form of this process (every one was asserted <= 1 where it was taken)"""
    for (op, form), v in sorted(RATIOS.items()):
        print(f'DENSE-SUMMARY {CHILD or "default"} | {op} | {form} | {v:.3f}')


CHILDREN = (
    ('persistent split-f16, one-pass TAN/TAN2', {'NNHIP_MLP_WIDE_TILES': '0'}),
    ('persistent split-f16, two-phase TAN/TAN2', {'NNHIP_MLP_WIDE_TILES': '0', 'NNHIP_MLP_REGW_TRAIN': '0'}),
    ('persistent fp32', {'NNHIP_MLP_WIDE_TILES': '0', 'NNHIP_MLP_SPLIT': '0'}),
    ('row-local fp32 in place of split', {'NNHIP_MLP_SPLIT': '0'}),
)


@pytest.mark.skipif(bool(CHILD), reason='a child process does not start children')
@pytest.mark.parametrize('tag,env', CHILDREN)
def test_forms_in_child_processes(tag, env):
    """The group above once per switch set (read once per process: a child pytest each, under a timeout).  The child's cases
    assert the form that ran (one-pass timer class, split_products, mlp_forms, config) and use that form's bound."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child_env = dict(os.environ, **env)
    child_env['NNHIP_DENSE_CHILD'] = ' '.join(f'{k}={v}' for k, v in env.items())
    try:
        r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-s', '-k', 'test_group'],
                           cwd=root, env=child_env, capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired:
        pytest.exit(f'[{tag}] the child process hung (900 s): no further GPU work is started', returncode=3)
    out = (r.stdout or '') + (r.stderr or '')
    if r.returncode < 0 or r.returncode in ABNORMAL_RC or any(m in out for m in FAULT_MARKS):
        # a signal, an abort, a time limit or a kernel fault -- not a plain test failure: the other children launch the same
        # kernels and the rest of this file uses the same device, so the whole session ends here
        pytest.exit(f'[{tag}] the child process ended abnormally (return code {r.returncode}): no further GPU work is started\n'
                    + out[-3000:], returncode=3)
    for line in (r.stdout or '').splitlines():
        if 'DENSE-SUMMARY' in line or 'DENSE-FORMS' in line:
            print(line)
    tail = (r.stdout or '')[-3000:] + (r.stderr or '')[-1500:]
    assert r.returncode == 0, f'[{tag}] {tail}'          # (a plain test failure of the child: the `-x` child stopped at it)
    assert ' passed' in r.stdout and 'failed' not in r.stdout.splitlines()[-1], f'[{tag}] {tail}'


# ---------------------------------------------------------------------------------------------------------------------------
# nnhip_wgrad_batch
# ---------------------------------------------------------------------------------------------------------------------------
WG_FORMS = {0: ('fp32 MFMA', R.FP32), 1: ('bf16 operands', R.BF16_RN), 2: ('three bf16 pieces', R.SPLIT3)}


class WgProblem:
    """one row of the device table with its operands, output buffer and float64 reference"""

    def __init__(self, key, M, typ, two, act='silu', ld=0, cols32=None, cap=None, pad=0):
        hip = _hip()
        rng = np.random.default_rng(_seed('wg', key, M, typ, two, act, ld))
        self.M, self.typ, self.two, self.act, self.cols32 = M, typ, two, act, cols32
        rows = cap if cap is not None else M                      # cap: the table is built for a capacity, M comes from pair_rows
        pitch = ld or 128
        h = {}

        def arr(name, w=128):
            a = _f32(rng, rows, w)
            h[name] = a[:M]
            t = dev(a, pitch if w == 128 else w)
            if cap is not None and M < rows:
                t[M:rows] = float('nan')                          # rows beyond this step's count are not read
            return t
        d = {'A1': arr('A1')}
        if cols32:
            rb = arr('rb', 64)                                    # [rows][64]: B1 = columns 0..31, B2 = columns 32..63
            d['B1'] = rb
            h['B1'], h['B2'] = h['rb'][:, :32], h['rb'][:, 32:]
        elif typ == 1:
            d['hB'] = arr('hB')
            if two:
                d['dhB'] = arr('dhB')
        else:
            d['B1'] = arr('B1')
            if two:
                d['B2'] = arr('B2')
        if two:
            d['A2'] = arr('A2')
            if typ == 2 and not cols32:
                d['hA'] = arr('hA')
        self.h, self.d = h, d
        ncols, ldo = cols32 if cols32 else (0, 0)
        self.ncols, self.ldo = (ncols or 128), (ldo or ncols or 128)
        self.out = blank(128, self.ldo)
        q = hip.WgradProblem()
        for name in ('A1', 'B1', 'A2', 'B2', 'hA', 'hB', 'dhB'):
            setattr(q, name, d[name].data_ptr() if name in d else None)
        if cols32 and two:
            q.B2 = d['B1'].data_ptr() + 32 * 4
        q.out = self.out.data_ptr()
        q.M = -1 if cap is not None else M
        q.lda1 = q.lda2 = q.ldh = ld
        q.ldb1 = q.ldb2 = 64 if cols32 else ld
        q.type, q.b_cols32, q.activation = (0 if cols32 else typ), (1 if cols32 else 0), hip.ACTIVATION_IDS[act]
        q.ldo, q.ncols, q.pad_ = (ldo, ncols, pad) if cols32 else (0, 0, pad)
        self.q = q

    def reference(self, form):
        h = self.h
        if self.cols32:
            V, B = R.wgrad(0, h['A1'], h['B1'], h.get('A2') if self.two else None, h['B2'] if self.two else None, form=form)
            return V[:, :self.ncols], B[:, :self.ncols]
        return R.wgrad(self.typ, h['A1'], h.get('B1'), h.get('A2'), h.get('B2'), h.get('hA'), h.get('hB'), h.get('dhB'), self.act, form)


def wgrad_launch(probs, chunks, bf16_operands, pair_rows=0, nan_bits=SENT):
    hip = _hip()
    L = hip.lib()
    table = (hip.WgradProblem * len(probs))(*[p.q for p in probs])
    tab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    slabs = torch.empty(L.nnhip_wgrad_slab_bytes(len(probs), chunks) // 4, dtype=torch.float32, device='cuda')
    slabs.view(torch.int32).fill_(nan_bits)
    for p in probs:
        p.out.view(torch.int32).fill_(SENT)
    rc = L.nnhip_wgrad_batch(tab.data_ptr(), len(probs), chunks, slabs.data_ptr(), bf16_operands, pair_rows, hip._stream(tab.device))
    torch.cuda.synchronize()
    assert rc == OK, L.nnhip_last_error()
    return [p.out.clone() for p in probs]


def wgrad_check(probs, chunks, bf16_operands, pair_rows=0, what=''):
    kname, form = WG_FORMS[bf16_operands]
    first = wgrad_launch(probs, chunks, bf16_operands, pair_rows, SENT)
    second = wgrad_launch(probs, chunks, bf16_operands, pair_rows, 0x7FFFFFFF)       # another NaN pattern in the slabs
    for k, p in enumerate(probs):
        tag = f'{what} chunks={chunks} problem {k}: M={p.M} type={p.typ} two={int(p.two)} act={p.act} cols32={p.cols32}'
        assert torch.equal(bits(first[k]), bits(second[k])), f'{tag}: two runs differ'
        assert guards_intact(first[k], 128, p.ncols), f'{tag}: outside of out[128][{p.ncols}] was written'
        got = host(first[k], 128, p.ncols)
        if p.M == 0:
            assert not got.any(), f'{tag}: M = 0 must give exactly zero'
            continue
        V, B = p.reference(form)
        record(f'wgrad_batch type {p.typ}{" b_cols32" if p.cols32 else ""}', kname, got, V, B, tag)


def _wg_rows(chunks):
    return sorted({0, 1, 15, 16, 17, 31, 32, 33, 16 * chunks - 1, 16 * chunks + 1, 1000})


@pytest.mark.parametrize('chunks', (1, 3, 64))
@pytest.mark.parametrize('bf16_operands', (0, 1, 2))
def test_wgrad_batch_rows_and_types(bf16_operands, chunks):
    """every row count x types 0, 1, 2 x one / two products, all problems of one (form, chunks) in ONE launch"""
    probs = [WgProblem('rows', M, typ, two) for M in _wg_rows(chunks) for typ in (0, 1, 2) for two in (False, True)]
    wgrad_check(probs, chunks, bf16_operands, what='rows')


@pytest.mark.parametrize('chunks', (1, 3, 64))
@pytest.mark.parametrize('bf16_operands', (0, 1, 2))
def test_wgrad_batch_operand_forms(bf16_operands, chunks):
    """32-column B rows (ncols 20 / 32, a non-default ldo), operand pitch 160, activations tanh / ssp, at ragged row counts"""
    probs = []
    for M in (17, 33, 16 * chunks + 1, 1000):
        for two in (False, True):
            probs.append(WgProblem('c32', M, 0, two, cols32=(20, 24)))
            probs.append(WgProblem('c32', M, 0, two, cols32=(32, 0)))
            for typ in (0, 1, 2):
                probs.append(WgProblem('ld', M, typ, two, ld=160))
            for act in ('tanh', 'ssp'):
                for typ in (1, 2):
                    probs.append(WgProblem('act', M, typ, two, act=act))
    wgrad_check(probs, chunks, bf16_operands, what='forms')


@pytest.mark.parametrize('bf16_operands', (0, 1, 2))
def test_wgrad_batch_mixed_table(bf16_operands):
    """one launch of eight problems of different M and type, as the table of train_fused.py: pair-level problems whose M is
    negative and resolved by pair_rows (smaller than the capacity they were built for), node-level ones, the radial-basis
    problem, and pad_ as a floor on the rows per chunk (a 40-row problem next to a 1000-row one)"""
    chunks, cap, pair_rows = 3, 1000, 777
    rpc = -(-cap // chunks)
    probs = [WgProblem('mix', pair_rows, 1, True, cap=cap, pad=rpc, ld=0), WgProblem('mix', pair_rows, 2, True, cap=cap, pad=rpc),
             WgProblem('mix', pair_rows, 0, True, cols32=(20, 20), cap=cap, pad=rpc), WgProblem('mix', 40, 1, True, pad=rpc),
             WgProblem('mix', 40, 2, True, pad=rpc), WgProblem('mix', 129, 1, False, pad=rpc), WgProblem('mix', 129, 0, False, pad=rpc),
             WgProblem('mix', 387, 0, True, pad=rpc)]
    wgrad_check(probs, chunks, bf16_operands, pair_rows=pair_rows, what='mixed, pad_')
    for p in probs:
        p.q.pad_ = 0
    wgrad_check(probs, chunks, bf16_operands, pair_rows=pair_rows, what='mixed')


# ---------------------------------------------------------------------------------------------------------------------------
# nnhip_colsum_batch, nnhip_species_sum
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', ((0, 1, 3, 4, 5), (63, 64, 65, 1000, 4097)))
def test_colsum_batch(rows):
    hip = _hip()
    L = hip.lib()
    rng = np.random.default_rng(_seed('colsum', rows))
    src = [_f32(rng, r, 128) for r in rows]
    outs = []
    for run in range(2):
        sd = [dev(s) for s in src]
        out = [blank(1) for _ in rows]
        table = (hip.ColsumProblem * len(rows))()
        for k, r in enumerate(rows):
            table[k].src, table[k].out, table[k].rows = sd[k].data_ptr(), out[k].data_ptr(), r
        tab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
        scratch = torch.empty(L.nnhip_colsum_scratch_bytes(len(rows)) // 4, dtype=torch.float32, device='cuda')
        scratch.view(torch.int32).fill_(SENT if run == 0 else 0x7FFFFFFF)
        rc = L.nnhip_colsum_batch(tab.data_ptr(), len(rows), scratch.data_ptr(), hip._stream(tab.device))
        torch.cuda.synchronize()
        assert rc == OK, L.nnhip_last_error()
        outs.append(out)
    for k, r in enumerate(rows):
        assert torch.equal(bits(outs[0][k]), bits(outs[1][k])), r
        assert guards_intact(outs[0][k], 1), r
        ref, B = R.colsum(src[k])
        got = host(outs[0][k], 1)[0]
        if r == 0:
            assert not got.any()
        record('colsum_batch', 'two passes', got, ref, B, f'rows={r}')
    assert L.nnhip_colsum_batch(None, 0, None, None) == OK


SPECIES = np.array([0, 1, 6, 7, 8, 118])


def species_case(n, width, which=(0, 1, 2), single_species=False):
    hip = _hip()
    L = hip.lib()
    rng = np.random.default_rng(_seed('species', n, width, which, single_species))
    ldx = width + 3
    x = _f32(rng, n, width)
    z = np.full(n, 8) if single_species else SPECIES[rng.integers(0, len(SPECIES), n)]
    c0, cols0 = 0, max(1, (3 * width) // 4)
    c1, cols1 = (cols0, width - cols0) if width > 1 else (0, 1)
    ct = width - 1
    what = f'n_atoms={n} width={width} outputs={which} ldx={ldx}'
    res = []
    for run in range(2):
        xd = dev(x, ldx)
        zd = flat(z, torch.int64)
        scratch = torch.empty(L.nnhip_species_scratch_bytes(width) // 4, dtype=torch.float32, device='cuda')
        scratch.view(torch.int32).fill_(SENT if run == 0 else 0x7FFFFFFF)
        o0, o1, tot = blank(R.N_ELEMENTS, cols0 + 2), blank(R.N_ELEMENTS, cols1 + 1), blank(1, 4)
        rc = L.nnhip_species_sum(xd.data_ptr(), ldx, width, zd.data_ptr(), n, scratch.data_ptr(),
                                 o0.data_ptr() if 0 in which else None, c0, cols0, cols0 + 2,
                                 o1.data_ptr() if 1 in which else None, c1, cols1, cols1 + 1,
                                 tot.data_ptr() if 2 in which else None, ct, hip._stream(xd.device))
        torch.cuda.synchronize()
        assert rc == OK, (what, L.nnhip_last_error())
        res.append((o0, o1, tot))
    for a, b in zip(*res):
        assert torch.equal(bits(a), bits(b)), f'{what}: two runs differ'
    o0, o1, tot = res[0]
    absent = np.setdiff1d(np.arange(R.N_ELEMENTS), z)
    for k, (o, c, cols) in enumerate(((o0, c0, cols0), (o1, c1, cols1))):
        if k not in which:
            assert untouched(o), f'{what}: output {k} was not asked for'
            continue
        assert guards_intact(o, R.N_ELEMENTS, cols), f'{what}: outside of output {k} was written'
        ref, B = R.species_sum(x, z, c, cols)
        got = host(o, R.N_ELEMENTS, cols)
        assert not got[absent].any(), f'{what}: rows of elements that do not occur must be exactly zero'
        record('species_sum', 'one launch' if n <= 1024 else 'two passes', got, ref, B, what)
    if 2 in which:
        assert guards_intact(tot, 1, 1)
        ref, B = R.species_total(x[:, ct], z)
        record('species_sum total', 'one launch' if n <= 1024 else 'two passes', host(tot, 1, 1), [[ref]], [[B]], what)
    else:
        assert untouched(tot)


@pytest.mark.parametrize('width', (1, 5, 128))
def test_species_sum(width):
    """1024 / 1025: the single launch hands over to the two passes; 16 385: the chunk count is capped at 256"""
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 1024, 1025, 16385):
        species_case(n, width)
    for which in ((0,), (1,), (2,)):
        species_case(129, width, which)
        species_case(1025, width, which)
    species_case(1024, width, single_species=True)        # the longest per-element list the single launch can see


# ---------------------------------------------------------------------------------------------------------------------------
# nnhip_loss_grad / nnhip_mse_loss_grad
# ---------------------------------------------------------------------------------------------------------------------------
LOSS_SIZES = (0, 1, 1023, 1024, 1025, 5000)


def _loss_arrays(rng, n, delta):
    lab = (np.round(_f32(rng, n) * 8) / 8).astype(np.float32)      # (multiples of 1/8: label + residual is exact for the special ones)
    res = _f32(rng, n, scale=2 * delta)
    special = np.array([0.0, delta, -delta, 0.0, delta], np.float32)
    res[:min(n, 5)] = special[:min(n, 5)]
    if n > 1030:
        res[1022:1027] = special                                   # around the 1024-thread stride as well
    return (lab + res).astype(np.float32), lab


@pytest.mark.parametrize('mode_f', (0, 1, 2))
@pytest.mark.parametrize('mode_e', (0, 1, 2))
def test_loss_grad(mode_e, mode_f):
    hip = _hip()
    L = hip.lib()
    de_, df_ = 0.5, 0.25
    st = hip._stream(torch.device('cuda', 0))
    for ne in LOSS_SIZES:
        for nf in LOSS_SIZES:
            rng = np.random.default_rng(_seed('loss', ne, nf))
            e, e_lab = _loss_arrays(rng, ne, de_)
            f, f_lab = _loss_arrays(rng, nf, df_)
            w = np.array([1.0 / max(ne, 1), 50.0 / max(nf, 1)], np.float32)
            wd = flat(w)                                             # the weights live in device memory
            args = [flat(e), flat(e_lab), ne, flat(f), flat(f_lab), nf, wd]
            ptr = lambda a: [t.data_ptr() if torch.is_tensor(t) else t for t in a]  # noqa: E731
            res = []
            for run in range(3 if (mode_e, mode_f) == (0, 0) else 2):
                loss, ge, gf = blank(1, 4), blank(1, max(ne, 4) + 4), blank(1, max(nf, 4) + 4)
                if run == 2:
                    rc = L.nnhip_mse_loss_grad(*ptr(args), loss.data_ptr(), ge.data_ptr(), gf.data_ptr(), st)
                else:
                    rc = L.nnhip_loss_grad(*ptr(args), mode_e, mode_f, de_, df_, loss.data_ptr(), ge.data_ptr(), gf.data_ptr(), st)
                torch.cuda.synchronize()
                assert rc == OK, L.nnhip_last_error()
                res.append((loss, ge, gf))
            for other in res[1:]:
                for a, b in zip(res[0], other):
                    assert torch.equal(bits(a), bits(b)), (ne, nf, 'runs differ (the third is nnhip_mse_loss_grad)')
            loss, ge, gf = res[0]
            assert guards_intact(loss, 1, 1) and guards_intact(ge, 1, ne) and guards_intact(gf, 1, nf), (ne, nf)
            ref, B, rge, rgf = R.loss_grad(e, e_lab, f, f_lab, w.astype(np.float64), mode_e, mode_f, de_, df_)
            what = f'modes {mode_e}/{mode_f} n_energy={ne} n_force={nf}'
            record('loss_grad loss', 'one workgroup', host(loss, 1, 1), [[ref]], [[B]], what)
            for got, want, n in ((ge, rge, ne), (gf, rgf, nf)):
                ulp2 = 2 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                record('loss_grad gradient (2 ulp)', 'one workgroup', host(got, 1, n)[0], want, ulp2, what)


# ---------------------------------------------------------------------------------------------------------------------------
# nnhip_clip_adam / nnhip_clip_adam_dev
# ---------------------------------------------------------------------------------------------------------------------------
def _adam_case(n, max_norm, dev_form=False, mask=None, lr_schedule=None):
    hip = _hip()
    L = hip.lib()
    rng = np.random.default_rng(_seed('adam', n, max_norm, dev_form))
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    lr, b1, b2, eps = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8)
    p = torch.from_numpy(_f32(rng, n)).cuda()
    m, v = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    state = torch.zeros(2, device='cuda')
    scratch = torch.empty(L.nnhip_clip_adam_scratch_bytes() // 4, device='cuda')
    maskd = flat(mask, torch.uint8) if mask is not None else None
    live = np.ones(n, bool) if mask is None else mask != 0
    hyper = torch.tensor([lr, b1, b2, eps, max_norm], dtype=torch.float32, device='cuda')
    st = hip._stream(p.device)
    # max_norm = 0.5 lies below the gradient norm and 1e6 above it at every n (asserted per step; at small n the elements are
    # pushed away from zero so that this holds for every draw)
    what = f'n={n} max_norm={max_norm} dev={int(dev_form)} mask={int(mask is not None)}'
    for t in range(1, 6):
        gh = _f32(rng, n, scale=3.0)
        gh = np.where(np.abs(gh) < 1.0, np.copysign(np.float32(1.0), gh) + gh, gh).astype(np.float32)     # |g_k| >= 1
        g = torch.from_numpy(gh).cuda()
        if lr_schedule:
            lr = f32(lr_schedule[t - 1])
            hyper[0] = lr                                       # changed in DEVICE memory between steps
        p0, m0, v0 = (a.cpu().double().numpy() for a in (p, m, v))
        scratch.view(torch.int32).fill_(SENT)
        if dev_form:
            rc = L.nnhip_clip_adam_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, scratch.data_ptr(), state.data_ptr(),
                                       hyper.data_ptr(), None if maskd is None else maskd.data_ptr(), st)
        else:
            rc = L.nnhip_clip_adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, scratch.data_ptr(), state.data_ptr(),
                                   lr, b1, b2, eps, max_norm, st)
        torch.cuda.synchronize()
        assert rc == OK, L.nnhip_last_error()
        rp, rm, rv, norm = R.clip_adam_step(p0, g.cpu().double().numpy(), m0, v0, t, lr, b1, b2, eps, f32(max_norm), mask)
        s = state.cpu().double().numpy()
        assert s[0] == t, (what, s)
        if live.any() and max_norm > 0:      # which branch of the clipping ran is known
            assert (norm > max_norm) if max_norm < 1 else (norm < max_norm), (what, norm)
        record('clip_adam norm', 'two passes', [s[1]], [norm], [R.grad_norm_rel_bound() * norm], f'{what} step {t}')
        gp = p.cpu().double().numpy()
        frozen = ~live
        assert np.array_equal(gp[frozen], p0[frozen]) and not m.cpu().numpy()[frozen].any() and not v.cpu().numpy()[frozen].any(), \
            f'{what}: frozen elements moved'
        record('clip_adam parameters', 'two passes', gp[live], rp[live], 4 * R.U * np.abs(rp[live]) + 1e-6 * lr, f'{what} step {t}')
        # the moments: the clipped gradient g' carries the norm's error and two roundings (5 u); exp_avg adds one product and one
        # fused multiply-add (7 u on |(1 - b1) g'| <= |m| + |b1 m0|, u on the result: 8 u (|m| + |m0|), since it may cancel against
        # its old value); exp_avg_sq squares g' (10 u), two products and the fused multiply-add: 13 u of non-negative terms, 16 u
        record('clip_adam exp_avg', 'two passes', m.cpu().double().numpy()[live], rm[live],
               8 * R.U * (np.abs(rm[live]) + np.abs(m0[live])), f'{what} step {t}')
        record('clip_adam exp_avg_sq', 'two passes', v.cpu().double().numpy()[live], rv[live],
               16 * R.U * (np.abs(rv[live]) + np.abs(v0[live])), f'{what} step {t}')


@pytest.mark.parametrize('max_norm', (0.5, 1e6, 0.0, -1.0))
@pytest.mark.parametrize('n', (1, 255, 256, 257, 65537, 1000003))
def test_clip_adam(n, max_norm):
    """five consecutive steps, each against one float64 step from the state the device held before it"""
    _adam_case(n, max_norm)


@pytest.mark.parametrize('n', (1, 257, 65537, 1000003))
def test_clip_adam_dev_mask_and_schedule(n):
    mask = (np.arange(n) % 3 != 0).astype(np.uint8)         # a third of the elements frozen
    _adam_case(n, 0.5, dev_form=True, mask=mask)
    _adam_case(n, 0.5, dev_form=True, lr_schedule=(1e-3, 1e-3, 5e-4, 5e-4, 2.5e-4))
    _adam_case(n, 0.0, dev_form=True)


def test_clip_adam_zero_elements():
    hip = _hip()
    L = hip.lib()
    t = blank(1, 4)
    state = blank(1, 2)
    assert L.nnhip_clip_adam(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, t.data_ptr(), state.data_ptr(), 1e-3, 0.9, 0.999,
                             1e-8, 1.0, hip._stream(t.device)) == OK
    torch.cuda.synchronize()
    assert untouched(t) and untouched(state)


def test_zz_ratio_summary():
    """the largest |got - ref| / bound per operation and form over the whole file (printed; each was asserted where it was taken)"""
    for (op, form), v in sorted(RATIOS.items()):
        print(f'DENSE-SUMMARY all | {op} | {form} | {v:.3f}')
