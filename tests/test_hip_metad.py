"""Bias on collective variables on the HIP path (newtonnet_amd/metadynamics.py, csrc/bias.hip).

Kernel alone: nnhip_bias_step on a synthetic batch of groups against the fp64 restatement of the launch (tests/bias_ref.py), every
output within its bound plus half an ulp of the stored value, every bit the launch does not own untouched.  Driver: without a bias
it is Dynamics bit for bit; with one, every recorded step is checked ONE step at a time as in tests/test_hip_md.py, the bias of the
reference on the hills recorded so far added to the model's forces on the recorded geometry."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import bias_ref as br
from tests import md_ref as mr
from tests import util
from tests.test_hip_hessian import cuda, make_model
from tests.test_hip_md import _forces, check_stepwise

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 777.0
SIGMA = {br.DISTANCE: 0.12, br.ANGLE: 0.2, br.TORSION: 0.35}
KIND = {'distance': br.DISTANCE, 'angle': br.ANGLE, 'torsion': br.TORSION}


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _wrapped(d):
    return d - 2.0 * np.pi * np.rint(d / (2.0 * np.pi))


# ---- the synthetic batch ------------------------------------------------------------------------------------------------------------

# (atoms, walkers, variables, restraints, bias factor, torsion 0 within 1e-3 of +pi with hill centres near -pi)
SPECS = [
    (2, 1, [('distance', 0, 1)], True, None, False),
    (3, 3, [('angle', 0, 1, 2)], False, 6.0, False),
    (4, 1, [('torsion', 0, 1, 2, 3)], True, 6.0, True),
    (5, 3, [('torsion', 0, 1, 2, 3), ('distance', 3, 4)], True, None, False),
    (21, 65, [('angle', 0, 5, 7), ('torsion', 3, 5, 9, 20)], True, 6.0, False),
    (255, 1, [('distance', 254, 0), ('angle', 1, 2, 254)], False, None, False),
    (256, 3, [], False, None, False),
    (257, 1, [('torsion', 256, 0, 128, 255)], False, 10.0, False),
    (300, 3, [('distance', 299, 256), ('torsion', 0, 256, 257, 299)], True, None, False),
    (4, 3, [('torsion', 0, 1, 2, 3), ('angle', 0, 1, 2)], True, None, True),
]
HILL_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)        # deposits so far: the hills of a group of one walker


def _cv_table(cvs):
    table = np.zeros((br.MAX_CVS, 5), dtype=np.int32)
    for d, cv in enumerate(cvs):
        table[d, 0] = KIND[cv[0]]
        table[d, 1:len(cv)] = cv[1:]
    return table


def _values(table, x):
    return [br.variable(int(table[d, 0]), table[d, 1:].tolist(), x) for d in range(br.MAX_CVS)]


def _base_geometry(rng, n, table):
    """n atoms in a box, redrawn until no variable is close to a singularity (gradient rows below 20 per unit)"""
    while True:
        x = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
        ok = True
        for s, _, atoms, rows, degenerate in _values(table, x.astype(np.float64)):
            ok = ok and not degenerate and all(abs(float(c.v)) < 20.0 for r in rows for c in r)
        if ok:
            return x


def _near_pi(j):
    """four atoms whose torsion is pi - (j + 1) 2e-4"""
    phi = 1.25 * np.pi - (j + 1) * 2e-4
    x = np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.5], [np.cos(phi), np.sin(phi), 2.5]])
    s = float(br.variable(br.TORSION, [0, 1, 2, 3], x)[0].v)
    if s < 0:
        x[:, 1] = -x[:, 1]
    return x.astype(np.float32)


def make_group(spec, seed, n_hills_max):
    n, W, cvs, restrained, gamma, near_pi = spec
    rng = np.random.default_rng(seed)
    table = _cv_table(cvs)
    if near_pi:
        x = np.stack([_near_pi(j) for j in range(W)])
    else:
        base = _base_geometry(rng, n, table)
        x = (base[None] + rng.normal(size=(W, n, 3)) * 0.02).astype(np.float32)
    s = np.array([[float(v[0].v) for v in _values(table, x[j].astype(np.float64))] for j in range(W)])         # [W, 2]
    if near_pi:
        assert np.all(s[:, 0] > np.pi - 1e-3) and np.all(s[:, 0] < np.pi)
    par = np.zeros(4)
    restraint = np.zeros((W, br.MAX_CVS, 2))
    rows = np.zeros((n_hills_max, 4))
    for d in range(len(cvs)):
        kind = int(table[d, 0])
        par[d] = 1.0 / SIGMA[kind] ** 2
        c = s[:, d].mean() + rng.normal(size=n_hills_max) * 1.2 * SIGMA[kind]
        if kind == br.TORSION:
            c = -np.pi + rng.uniform(0.0, 0.3, n_hills_max) if near_pi and d == 0 else _wrapped(c)
        rows[:, d] = c
        if restrained:
            restraint[:, d, 0] = rng.uniform(0.5, 3.0, W)
            centre = s[:, d] + rng.normal(size=W) * 0.2
            restraint[:, d, 1] = -np.pi + 0.1 if near_pi and d == 0 else (_wrapped(centre) if kind == br.TORSION else centre)
    rows[:, 2] = rng.uniform(0.002, 0.01, n_hills_max)
    par[2] = 0.01
    par[3] = 0.0 if gamma is None else 1.0 / (br.K_BOLTZMANN * (gamma - 1.0) * 300.0)
    return dict(n=n, W=W, x=x, f=rng.normal(size=(W, n, 3)).astype(np.float32), cv_def=np.stack([table] * W),
                restraint=restraint.astype(np.float32), par=par.astype(np.float32), rows=rows.astype(np.float32))


@pytest.fixture(scope='module')
def groups():
    return [make_group(spec, 100 + i, 1000 * spec[1]) for i, spec in enumerate(SPECS)]


def pack(groups, n_deposits, room=1):
    """the launch's arrays; every group's list holds its first n_deposits W rows, sentinels behind them"""
    W_max = max(g['W'] for g in groups)
    capacity = (n_deposits + room) * W_max + 2
    hills = np.full((len(groups), capacity, 4), SENT, dtype=np.float32)
    for i, g in enumerate(groups):
        hills[i, :n_deposits * g['W']] = g['rows'][:n_deposits * g['W']]
    counts = np.concatenate([[g['n']] * g['W'] for g in groups])
    return dict(pos=np.concatenate([g['x'].reshape(-1, 3) for g in groups]), force_in=np.concatenate([g['f'].reshape(-1, 3) for g in groups]),
                mol_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                group_ptr=np.concatenate([[0], np.cumsum([g['W'] for g in groups])]).astype(np.int32),
                cv_def=np.concatenate([g['cv_def'] for g in groups]).astype(np.int32),
                restraint=np.concatenate([g['restraint'] for g in groups]), hill_par=np.stack([g['par'] for g in groups]), hills=hills)


READ = ('pos', 'force_in', 'mol_ptr', 'group_ptr', 'cv_def', 'restraint', 'hill_par')
WRITTEN = ('force_out', 'cv_out', 'bias_out', 'status_out', 'hills')


def tensors(p):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in p.items()}
    t['mol_ptr_host'], t['group_ptr_host'] = torch.from_numpy(p['mol_ptr'].copy()), torch.from_numpy(p['group_ptr'].copy())
    N, B = p['pos'].shape[0], p['mol_ptr'].shape[0] - 1
    t['force_out'] = torch.full((N, 3), SENT, device='cuda')
    t['cv_out'], t['bias_out'] = torch.full((B, 2), SENT, device='cuda'), torch.full((B, 2), SENT, device='cuda')
    t['status_out'] = torch.full((B,), 777, dtype=torch.int32, device='cuda')
    return t


def call(t, n_deposits, flags, **replace):
    from newtonnet_amd import hip
    a = dict(t, **replace)
    hip.bias_step(a['pos'], a['force_in'], a['mol_ptr'], a['mol_ptr_host'], a['group_ptr'], a['group_ptr_host'], a['cv_def'],
                  a['restraint'], a['hill_par'], a['hills'], n_deposits, flags, a['force_out'], a['cv_out'], a['bias_out'],
                  a['status_out'])


def launch(groups, n_deposits, flags):
    """one launch; returns what it left as numpy arrays, and checks that the inputs are intact"""
    p = pack(groups, n_deposits)
    t = tensors(p)
    call(t, n_deposits, flags)
    torch.cuda.synchronize()
    for name in READ:
        assert _same(_np(t[name]), p[name]), name
    return p, {k: _np(t[k]) for k in WRITTEN}


def _within(got, want, bound, worst, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    tol = bound + br.half_ulp32(want)
    ratio = float(np.max(err / tol)) if err.size else 0.0
    worst[what] = max(worst.get(what, 0.0), ratio)
    assert np.all(err <= tol), f'{what}: err / bound {ratio:.3f}'


def check_against_reference(groups, p, out, n_deposits, flags, worst):
    for i, g in enumerate(groups):
        m0, W, n = p['group_ptr'][i], g['W'], g['n']
        H = n_deposits * W
        walkers, new = br.group(g['x'], g['f'], g['cv_def'], g['restraint'], g['par'], p['hills'][i], n_deposits, flags)
        for j, w in enumerate(walkers):
            b = m0 + j
            a0 = p['mol_ptr'][b]
            what = (i, j, n_deposits)
            assert w['ambiguous'] == 0, what
            got_f = out['force_out'][a0:a0 + n]
            assert out['status_out'][b] == w['status'] == 0, what
            # an atom in no variable, and a whole molecule without one, keeps every bit of force_in
            assert _same(got_f[~w['touched']], g['f'][j][~w['touched']]), what
            assert not w['touched'].any() or g['cv_def'][j, :, 0].any(), what
            _within(got_f[w['touched']], w['force'][w['touched']], w['bforce'][w['touched']], worst, 'force')
            _within(out['cv_out'][b], w['cv'], w['bcv'], worst, 'cv')
            _within(out['bias_out'][b], w['bias'], w['bbias'], worst, 'bias')
        rows = out['hills'][i]
        assert _same(rows[:H], p['hills'][i, :H]), i                                   # the hills that existed
        if flags & br.DEPOSIT:
            cv = out['cv_out'][m0:m0 + W]
            assert _same(rows[H:H + W, :2], cv), i                                      # the centres: the walkers' own cv, bit for bit
            assert np.all(rows[H:H + W, 3] == 0.0), i
            _within(rows[H:H + W, 2], new[:, 2], np.array([w['bheight'] for w in walkers]), worst, 'height')
            assert np.all(rows[H + W:] == np.float32(SENT)), i                         # nothing behind them
        else:
            assert np.all(rows[H:] == np.float32(SENT)), i


# ---- 1. the kernel against the restatement --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_deposits', HILL_COUNTS)
def test_kernel_against_the_reference(groups, n_deposits):
    worst = {}
    for flags in (0, br.DEPOSIT):
        p, out = launch(groups, n_deposits, flags)
        check_against_reference(groups, p, out, n_deposits, flags, worst)
    print(f'{n_deposits} deposits ({[n_deposits * g["W"] for g in groups]} hills): worst err / bound '
          + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()))


# ---- 2. properties ----------------------------------------------------------------------------------------------------------------------

def test_launches_repeat_and_a_group_does_not_depend_on_the_batch(groups):
    n_deposits = 65
    p, whole = launch(groups, n_deposits, br.DEPOSIT)
    _, again = launch(groups, n_deposits, br.DEPOSIT)
    _, backwards = launch(groups[::-1], n_deposits, br.DEPOSIT)
    for k in WRITTEN:
        assert _same(whole[k], again[k]), k
    rev_ptr = np.concatenate([[0], np.cumsum([g['W'] for g in groups[::-1]])])
    for i, g in enumerate(groups):
        pa, alone = launch([g], n_deposits, br.DEPOSIT)
        m0, W, n = p['group_ptr'][i], g['W'], g['n']
        a0 = p['mol_ptr'][m0]
        r = len(groups) - 1 - i
        rm0 = rev_ptr[r]
        ra0 = int(sum(h['W'] * h['n'] for h in groups[::-1][:r]))
        assert _same(alone['force_out'], whole['force_out'][a0:a0 + W * n]), i
        assert _same(backwards['force_out'][ra0:ra0 + W * n], whole['force_out'][a0:a0 + W * n]), i
        for k in ('cv_out', 'bias_out', 'status_out'):
            assert _same(alone[k], whole[k][m0:m0 + W]) and _same(backwards[k][rm0:rm0 + W], whole[k][m0:m0 + W]), (i, k)
        rows = (n_deposits + 1) * W
        assert _same(alone['hills'][0, :rows], whole['hills'][i, :rows]) and _same(backwards['hills'][r, :rows], whole['hills'][i, :rows]), i
    # the bias force of a molecule has no net force
    for i, g in enumerate(groups):
        m0, W, n = p['group_ptr'][i], g['W'], g['n']
        walkers, _ = br.group(g['x'], g['f'], g['cv_def'], g['restraint'], g['par'], p['hills'][i], n_deposits)
        for j, w in enumerate(walkers):
            a0 = p['mol_ptr'][m0 + j]
            net = (whole['force_out'][a0:a0 + n].astype(np.float64) - g['f'][j]).sum(0)
            bound = (w['bforce'] + br.half_ulp32(w['force']) * w['touched']).sum(0) + 1e-12 * np.abs(w['force']).max()
            assert np.all(np.abs(net) <= bound), (i, j, net, bound)


def _one_molecule(x, cv_def, restraint=None, n_hills=0):
    n = x.shape[0]
    rng = np.random.default_rng(5)
    rows = np.zeros((max(n_hills, 1), 4), dtype=np.float32)
    rows[:, 2] = 0.01
    return dict(n=n, W=1, x=x[None].astype(np.float32), f=rng.normal(size=(1, n, 3)).astype(np.float32),
                cv_def=np.asarray(cv_def, dtype=np.int32)[None],
                restraint=np.asarray([[[2.0, 1.0], [2.0, 1.0]]] if restraint is None else restraint, dtype=np.float32),
                par=np.array([4.0, 4.0, 0.01, 0.0], dtype=np.float32), rows=rows)


def test_degenerate_and_impossible_variables():
    # three collinear atoms (exactly: the cross products are 0 in any precision): the torsion has no gradient, the distance has
    line = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.5, 0.0, 0.0], [3.0, 1.0, 0.5], [0.5, 0.5, 2.0]])
    deg = _one_molecule(line, [[br.TORSION, 0, 1, 2, 3], [br.DISTANCE, 3, 4, 0, 0]], n_hills=3)
    coincident = _one_molecule(np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 0.0, 1.0]]), [[br.DISTANCE, 0, 1, 0, 0], [br.ANGLE, 0, 1, 2, 0]])
    straight = _one_molecule(line[:3], [[br.ANGLE, 0, 1, 2, 0], [br.ANGLE, 1, 0, 2, 0]])
    batch = [deg, coincident, straight]
    p, out = launch(batch, 3, br.DEPOSIT)
    assert out['status_out'].tolist() == [1, 3, 3]
    assert np.isfinite(out['force_out']).all() and np.isfinite(out['cv_out']).all() and np.isfinite(out['bias_out']).all()
    worst = {}
    for i, g in enumerate(batch):
        w = br.walker(g['x'][0], g['f'][0], g['cv_def'][0], g['restraint'][0], g['par'], p['hills'][i, :3])
        a0 = p['mol_ptr'][i]
        got = out['force_out'][a0:a0 + g['n']]
        assert w['status'] == out['status_out'][i] and w['ambiguous'] == 0
        assert _same(got[~w['touched']], g['f'][0][~w['touched']])
        _within(got[w['touched']], w['force'][w['touched']], w['bforce'][w['touched']], worst, 'force')
        _within(out['cv_out'][i], w['cv'], w['bcv'], worst, 'cv')
        _within(out['bias_out'][i], w['bias'], w['bbias'], worst, 'bias')
    a0 = p['mol_ptr'][0]
    assert _same(out['force_out'][a0:a0 + 3], deg['f'][0][:3]) and not _same(out['force_out'][a0 + 3:a0 + 5], deg['f'][0][3:])
    assert _same(out['force_out'][p['mol_ptr'][1]:], np.concatenate([coincident['f'][0], straight['f'][0]]))      # no gradient at all
    assert abs(float(out['cv_out'][2, 0]) - np.pi) < 1e-6 and out['cv_out'][2, 1] == 0.0 and out['cv_out'][1, 0] == 0.0
    # state words no driver leaves behind: a pure copy and the status bit, no hill, the neighbours as they are
    good = _one_molecule(line[[0, 1, 3, 4]], [[br.TORSION, 0, 1, 2, 3], [br.DISTANCE, 0, 3, 0, 0]])
    bad = [_one_molecule(line, d) for d in ([[br.DISTANCE, 0, 5, 0, 0], [0, 0, 0, 0, 0]], [[br.ANGLE, 0, 1, -1, 0], [0, 0, 0, 0, 0]],
                                           [[br.DISTANCE, 0, 1, 0, 0], [7, 0, 1, 2, 3]], [[-1, 0, 1, 0, 0], [0, 0, 0, 0, 0]],
                                           [[br.TORSION, 0, 1, 2, 2 ** 31 - 1], [0, 0, 0, 0, 0]])]
    batch = [good] + bad + [good]
    p, out = launch(batch, 0, br.DEPOSIT)
    assert out['status_out'].tolist() == [0] + [br.STATUS_INVALID] * len(bad) + [0]
    for i, g in enumerate(batch):
        a0 = p['mol_ptr'][i]
        if 0 < i <= len(bad):
            assert _same(out['force_out'][a0:a0 + g['n']], g['f'][0]) and not out['cv_out'][i].any() and not out['bias_out'][i].any()
            assert np.all(out['hills'][i] == np.float32(SENT))
        else:
            assert not _same(out['force_out'][a0:a0 + g['n']], g['f'][0]) and out['hills'][i, 0, 2] == np.float32(0.01)
    assert _same(out['force_out'][:4], out['force_out'][-4:])


def test_refusals_write_nothing_and_an_empty_batch_succeeds(groups):
    from newtonnet_amd import hip
    small = [groups[0], groups[3], groups[1]]
    n_deposits = 2
    p = pack(small, n_deposits)
    t = tensors(p)
    before = {k: t[k].clone() for k in WRITTEN}
    B, G, N, capacity = p['mol_ptr'].shape[0] - 1, len(small), p['pos'].shape[0], p['hills'].shape[1]

    def host(a):
        return torch.tensor(a, dtype=torch.int32)
    gp, mp = p['group_ptr'], p['mol_ptr']
    short, late, empty, uneven, not_to_n = gp.copy(), gp.copy(), gp.copy(), mp.copy(), mp.copy()
    short[-1] -= 1
    late[0] = 1
    empty[2] = empty[1]                                           # a group without walkers
    uneven[2] += 1                                                # the first two walkers of group 1 differ in size
    not_to_n[-1] -= 1
    room = capacity // 3                                          # the largest group has 3 walkers
    cases = [('run from 0', 0, dict(group_ptr_host=host(short))), ('run from 0', 0, dict(group_ptr_host=host(late))),
             ('walkers', 0, dict(group_ptr_host=host(empty))), ('atoms', 0, dict(mol_ptr_host=host(uneven))),
             ('run from 0', 0, dict(mol_ptr_host=host(not_to_n))), ('overlap', 0, dict(force_out=t['force_in'])),
             ('overlap', 0, dict(force_out=t['pos'])), ('flag', 2, dict()), ('flag', 3, dict())]
    for match, flags, replace in cases:
        with pytest.raises(hip.HipLibraryError, match=match):
            call(t, n_deposits, flags, **replace)
    with pytest.raises(hip.HipLibraryError, match='capacity'):
        call(t, room + 1, 0)
    with pytest.raises(hip.HipLibraryError, match='capacity'):
        call(t, room, br.DEPOSIT)
    call(t, room, 0, force_out=torch.empty_like(t['force_out']), cv_out=torch.empty_like(t['cv_out']),
         bias_out=torch.empty_like(t['bias_out']), status_out=torch.empty_like(t['status_out']))       # the last count that fits
    # straight at the C entry point: NULL pointers one at a time, negative counts, n_deposits < 0
    names = ('pos', 'force_in', 'mol_ptr', 'mol_ptr_host', 'group_ptr', 'group_ptr_host', 'cv_def', 'restraint', 'hill_par', 'hills')
    outs = ('force_out', 'cv_out', 'bias_out', 'status_out')
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(missing=None, capacity=capacity, n_deposits=n_deposits, flags=0, counts=(G, B, N)):
        ptr = {k: None if k == missing else C.c_void_p(t[k].data_ptr()) for k in names + outs}
        return hip.lib().nnhip_bias_step(*[ptr[k] for k in names], capacity, n_deposits, flags, *counts, *[ptr[k] for k in outs], stream)
    for missing in names + outs:
        assert raw(missing) != 0 and b'null' in hip.lib().nnhip_last_error(), missing
    assert raw(n_deposits=-1) != 0 and b'n_deposits' in hip.lib().nnhip_last_error()
    for bad in ((-1, B, N), (G, -1, N), (G, B, -1)):
        assert raw(counts=bad) != 0
    assert raw(capacity=-1) != 0 and raw(flags=-1) != 0 and raw(flags=4) != 0
    torch.cuda.synchronize()
    for k in WRITTEN:
        assert torch.equal(t[k], before[k]), k                                   # nothing was written
    # the wrapper refuses what would be written into a copy, and counts that are no counts
    with pytest.raises(ValueError, match='force_out'):
        call(t, 0, 0, force_out=t['force_out'].double())
    with pytest.raises(ValueError, match='hills'):
        call(t, 0, 0, hills=t['hills'][:, :, :3])
    with pytest.raises(ValueError, match='n_deposits'):
        call(t, -1, 0)
    with pytest.raises(ValueError, match='n_deposits'):
        call(t, 1.5, 0)
    with pytest.raises(ValueError, match='flags'):
        call(t, 0, -1)
    # nnhip_bias_eval's refusals
    pts = torch.zeros(4, 2, device='cuda')
    for bad in (dict(group=G), dict(group=-1), dict(n_hills=capacity + 1), dict(n_hills=-1)):
        with pytest.raises(ValueError):
            hip.bias_eval(t['hills'], t['hill_par'], **dict(dict(group=0, n_hills=1), **bad), points=pts)
    with pytest.raises(hip.HipLibraryError, match='period'):
        hip.bias_eval(t['hills'], t['hill_par'], 0, 1, pts, periods=(-1.0, 0.0))
    with pytest.raises(hip.HipLibraryError, match='period'):
        hip.bias_eval(t['hills'], t['hill_par'], 0, 1, pts, periods=(0.0, float('nan')))
    assert hip.bias_eval(t['hills'], t['hill_par'], 0, 1, pts[:0]).shape == (0,)
    # an empty batch: success, nothing to write
    e32, ef = torch.zeros(0, dtype=torch.int32, device='cuda'), torch.zeros(0, device='cuda')
    zero = torch.zeros(1, dtype=torch.int32)
    hip.bias_step(ef.view(0, 3), ef.view(0, 3), zero.cuda(), zero, zero.cuda(), zero.clone(), e32.view(0, 2, 5), ef.view(0, 2, 2),
                  ef.view(0, 4), torch.zeros(0, 8, 4, device='cuda'), 0, 0, torch.zeros(0, 3, device='cuda'), ef.view(0, 2).clone(),
                  ef.view(0, 2).clone(), e32.clone())
    # the valid call still works after all the refusals
    call(t, n_deposits, br.DEPOSIT)
    torch.cuda.synchronize()
    check_against_reference(small, p, {k: _np(t[k]) for k in WRITTEN}, n_deposits, br.DEPOSIT, {})


# ---- 3. no bias is Dynamics -------------------------------------------------------------------------------------------------------------

FRICTION = 0.02
SEED = 7
TRAJ = ('pos', 'vel', 'potential_energy', 'kinetic_energy', 'step')


def _mixed_two():
    z, pos, cell, batch, _ = util.case_inputs('mixed_rand', torch.float32)
    two = batch < 2                                                    # two systems: 21 and 9 atoms
    return cuda(z[two], pos[two], cell[:2], batch[two])


MIXED_CVS = [('torsion', 0, 1, 2, 3), ('distance', 3, 8)]


@pytest.mark.parametrize('thermostat', ['nve', 'langevin'])
def test_without_a_bias_it_is_dynamics_bit_for_bit(thermostat):
    z, pos, cell, batch = _mixed_two()
    model = make_model(util.load_state('rand'))
    T = 300.0 if thermostat == 'nve' else torch.tensor([250.0, 400.0], device='cuda')
    friction = 0.0 if thermostat == 'nve' else FRICTION

    def gen():
        return torch.Generator(device='cuda').manual_seed(SEED)
    plain = model.dynamics(z, pos, cell, batch, temperature=T, friction=friction, generator=gen()).run(20, 1)
    none = model.metadynamics(z, pos, cell, batch, [], T, friction, 0.0, 1.0, 0, generator=gen())
    idle = model.metadynamics(z, pos, cell, batch, MIXED_CVS, T, friction, 0.0, [0.3, 0.1], 5, restraint_k=0.0, restraint_center=1.0,
                              generator=gen())
    for meta in (none, idle):
        traj = meta.run(20, 1)
        for name in TRAJ:
            assert torch.equal(getattr(traj, name), getattr(plain, name)), name
        assert _same(_np(traj.pos), _np(plain.pos)) and _same(_np(traj.vel), _np(plain.vel))
        assert not traj.bias_energy.any() and not traj.restraint_energy.any() and traj.n_hills.tolist() == [0] * 20
        assert meta.n_hills == 0 and not meta.status.any()
    assert not none.collective_variables.any() and idle.collective_variables.abs().min() > 0


# ---- 4. the driver, one step at a time -----------------------------------------------------------------------------------------------

GAMMA = 6.0
WT = dict(hill_height=0.02, hill_width=[0.3, 0.1], pace=5, bias_factor=GAMMA)


def _make_wt(model, inputs, walkers=3, seed=SEED, **kw):
    a = dict(WT, **kw)
    gen = torch.Generator(device='cuda').manual_seed(seed)
    return model.metadynamics(*inputs, MIXED_CVS, 300.0, FRICTION, a.pop('hill_height'), a.pop('hill_width'), a.pop('pace'),
                              walkers=walkers, generator=gen, restraint_k=[0.5, 2.0], restraint_center=[0.4, 3.0], **a)


def test_every_recorded_step_follows_from_the_one_before_under_the_bias():
    from newtonnet_amd.metadynamics import hill_parameters
    inputs = _mixed_two()
    model = make_model(util.load_state('rand'))
    G, W, n_steps, pace = 2, 3, 40, 5
    meta = _make_wt(model, inputs)
    B, N = G * W, meta.n_atoms
    counts = _np(meta._counts).tolist()
    assert counts == [21] * 3 + [9] * 3
    p0, v0 = meta.positions, meta.velocities
    before = model.deferred_stats()
    traj = meta.run(n_steps, record_every=1)
    after = model.deferred_stats()
    assert after['repeats_needed'] == before['repeats_needed']
    assert traj.step.tolist() == list(range(1, n_steps + 1))
    assert traj.n_hills.tolist() == [W * (s // pace) for s in range(1, n_steps + 1)] and meta.n_hills == W * (n_steps // pace)
    regen = torch.Generator(device='cuda').manual_seed(SEED)
    torch.randn((N, 3), generator=regen, device='cuda')                              # the Maxwell-Boltzmann draw
    noises = [torch.randn((N, 3), generator=regen, device='cuda') for _ in range(n_steps)]
    # the final hill list: the recorded cv of the depositing steps, in (deposit, walker) order
    cv = _np(traj.cv)
    hills = [(_np(c), _np(h)) for c, h in meta.hills]
    for g in range(G):
        want = np.concatenate([cv[s - 1, g * W:(g + 1) * W] for s in range(pace, n_steps + 1, pace)])
        assert _same(hills[g][0], want), g
    par = hill_parameters([2, 2], np.array(WT['hill_width']), WT['hill_height'], GAMMA, [300.0, 300.0])
    assert _same(_np(meta._hill_par), par)
    table = np.stack([_cv_table(MIXED_CVS)] * B)
    restraint = np.tile(np.array([[0.5, 0.4], [2.0, 3.0]], dtype=np.float32), (B, 1, 1))
    assert _same(_np(meta._restraint), restraint) and _same(_np(meta._cv_def), table)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    worst = {}
    frame = [0]
    z_r, cell_r, batch_r = meta.z, meta.cell, meta.batch

    def biased(z, pos, cell, batch):
        """the model's forces on a recorded geometry plus the reference's bias on the hills recorded before that step"""
        k = frame[0]
        frame[0] += 1
        f, e = _forces(model, z, pos, cell, batch)
        x, f_model = _np(pos), _np(f)
        out = np.empty_like(f_model)
        H = W * ((k - 1) // pace) if k > 0 else 0
        for b in range(B):
            g = b // W
            rows = np.zeros((H, 4), dtype=np.float32)
            rows[:, :2], rows[:, 2] = hills[g][0][:H], hills[g][1][:H]
            w = br.walker(x[ptr[b]:ptr[b + 1]], f_model[ptr[b]:ptr[b + 1]], table[b], restraint[b], par[g], rows)
            assert w['ambiguous'] == 0 and w['status'] == 0
            out[ptr[b]:ptr[b + 1]] = w['force']
            if k > 0:
                _within(cv[k - 1, b], w['cv'], w['bcv'], worst, 'cv')
                _within(_np(traj.bias_energy[k - 1, b]), w['bias'][0], w['bbias'][0], worst, 'V')
                _within(_np(traj.restraint_energy[k - 1, b]), w['bias'][1], w['bbias'][1], worst, 'U')
                if k % pace == 0:                                                  # this step deposited: the height it wrote
                    _within(hills[g][1][H + b - g * W], w['height'], w['bheight'], worst, 'height')
        return types.SimpleNamespace(gradient_force=torch.from_numpy(out).cuda(), energy=e)
    shim = types.SimpleNamespace(_hk=meta._hk, masses=meta.masses, _sigma=meta._sigma, _c1=meta._c1, _dth=meta._dth)
    check_stepwise(biased, shim, z_r, cell_r, batch_r, [p0] + list(traj.pos), [v0] + list(traj.vel), noises, 'metadynamics')
    assert frame[0] == n_steps + 1
    print('recorded outputs against the reference, worst err / bound: ' + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()))
    heights = np.concatenate([h for _, h in hills])
    assert np.all(heights[:W] == np.float32(WT['hill_height'])) and np.all(heights > 0)          # the first deposit met no bias
    assert np.all(heights <= np.float32(WT['hill_height'])) and heights.min() < 0.999 * WT['hill_height'], 'the tempering shows nothing'
    assert float(traj.bias_energy.max()) > 1e-3 and float(traj.restraint_energy.max()) > 1e-3


# ---- 5., 6. capacity and bitwise properties -----------------------------------------------------------------------------------------

STATE = ('positions', 'velocities', 'forces', 'potential_energy', 'kinetic_energy', 'collective_variables', 'bias_energy',
         'restraint_energy')
BIASED = TRAJ + ('cv', 'bias_energy', 'restraint_energy', 'n_hills')


def test_capacity_and_bitwise_properties():
    inputs = _mixed_two()
    keep = [t.clone() for t in inputs]
    model = make_model(util.load_state('rand'))
    whole = _make_wt(model, inputs, hill_capacity=4096)
    a = whole.run(20, 1)
    assert whole._hills.shape[1] == 4096 and whole.n_hills == 12
    # the hill list grown from 4 rows on the way: the same bits
    tight = _make_wt(model, inputs, hill_capacity=4)
    b = tight.run(20, 1)
    assert tight._hills.shape[1] == 16
    for name in BIASED:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in STATE:
        assert torch.equal(getattr(whole, name), getattr(tight, name)), name
    for (c0, h0), (c1, h1) in zip(whole.hills, tight.hills):
        assert torch.equal(c0, c1) and torch.equal(h0, h1) and c0.shape == (12, 2)
    assert not tight._hills[:, 12:].any()
    # run(11, 4); run(9, 0) is run(20): the deposits are counted by the global step
    d = _make_wt(model, inputs, hill_capacity=4)
    first = d.run(11, 4)
    last = d.run(9, 0)
    assert first.step.tolist() == [4, 8, 11] and first.n_hills.tolist() == [0, 3, 6] and last.n_hills.tolist() == [12]
    for name in BIASED:
        assert torch.equal(getattr(first, name), getattr(a, name)[[3, 7, 10]]), name
        assert torch.equal(getattr(last, name)[0], getattr(a, name)[-1]), name
    # record_every changes no bit
    e = _make_wt(model, inputs)
    final = e.run(20, 0)
    for name in BIASED:
        assert torch.equal(getattr(final, name)[0], getattr(a, name)[-1]), name
    for other in (d, e):
        for name in STATE:
            assert torch.equal(getattr(other, name), getattr(whole, name)), name
        for (c0, h0), (c1, h1) in zip(whole.hills, other.hills):
            assert torch.equal(c0, c1) and torch.equal(h0, h1)
        assert other.step_count == 20 and other.n_deposits == 4
    assert e.run(0).n_hills.tolist() == [12]
    # the same seed twice; another seed differs; the caller's tensors are never modified
    assert not torch.equal(_make_wt(model, inputs, seed=SEED + 1).run(20, 0).pos, final.pos)
    for t, k in zip(inputs, keep):
        assert torch.equal(t, k)


# ---- 7. conservation in the restrained potential -----------------------------------------------------------------------------------------

def test_energy_conservation_in_the_restrained_potential():
    """2 aspirins, microcanonical, no hills, a stiff torsion restraint and a distance restraint, 0.5 fs, 400 steps.  Per molecule,
    max_n |E(n) - E(0)| of E = model energy + restraint energy + kinetic energy stays within the bound tests/test_hip_md.py forms:
    (a) the same figure of a host fp64 velocity-Verlet loop on the same extended potential (model() forces plus the reference's
    restraint force, model() energy plus the reference's U) from the same start + (b) the first-order cost of the fp32 state, sum
    over steps of [sum_i |F_i| ulp(x_i) / 2 + sum_i m_i v_i^2 2^-24], F the BIASED force + (c) 2 util.energy_tol(E).  The restraint
    energy itself must move by more than 10 x that bound, so a force inconsistent with the energy cannot pass."""
    from newtonnet_amd import dynamics as dyn_mod
    n_steps, B, n = 400, 2, 21
    z, pos, cell, batch = _bench().synthetic_aspirin(B, 0, 'cuda')
    model = make_model(util.load_state('rand'))
    cvs = [('torsion', 0, 1, 2, 3), ('distance', 4, 12)]
    table = _cv_table(cvs)
    x0 = _np(pos).astype(np.float64)
    s_start = [[float(v[0].v) for v in _values(table, x0[b * n:(b + 1) * n])] for b in range(B)]
    kappa = np.array([10.0, 15.0])
    centre = np.array([[s[0] + 0.25, s[1] + 0.15] for s in s_start])                    # [B, 2]: both restraints start displaced
    gen = torch.Generator(device='cuda').manual_seed(11)
    meta = model.metadynamics(z, pos, cell, batch, cvs, 300.0, 0.0, 0.0, [0.3, 0.1], 0, restraint_k=kappa,
                              restraint_center=centre[:, None, :], timestep=0.5, generator=gen)
    restraint = _np(meta._restraint)
    assert restraint.shape == (B, 2, 2) and _same(restraint[:, :, 0], np.tile(kappa.astype(np.float32), (B, 1)))
    p0, v0 = meta.positions, meta.velocities
    e0, k0, u0 = meta.potential_energy.clone(), meta.kinetic_energy, meta.restraint_energy
    traj = meta.run(n_steps, record_every=1)
    assert meta.n_hills == 0 and not traj.bias_energy.any() and not meta.status.any()
    m = _np(meta.masses).astype(np.float64)
    pe = np.concatenate([_np(e0)[None], _np(traj.potential_energy)]).astype(np.float64)
    ke = np.concatenate([_np(k0)[None], _np(traj.kinetic_energy)]).astype(np.float64)
    ue = np.concatenate([_np(u0)[None], _np(traj.restraint_energy)]).astype(np.float64)
    tot = pe + ke + ue
    drift = np.abs(tot - tot[0]).max(axis=0)
    par, none = np.zeros(4, dtype=np.float32), np.zeros((0, 4), dtype=np.float32)

    def evaluate(xx):
        """forces and energy of the extended potential at fp64 positions xx: the model's at fl32(xx), the restraint's from the reference"""
        f, e = _forces(model, z, torch.from_numpy(xx).float().cuda(), cell, batch)
        f, e = _np(f).astype(np.float64), _np(e).astype(np.float64)
        for b in range(B):
            w = br.walker(xx[b * n:(b + 1) * n], f[b * n:(b + 1) * n], table, restraint[b], par, none)
            f[b * n:(b + 1) * n] = w['force']
            e[b] += w['bias'][1]
        return f, e
    # (a) host fp64 velocity Verlet on the same extended potential
    dt = 0.5 * dyn_mod.FS
    x, v = _np(p0).astype(np.float64), _np(v0).astype(np.float64)
    f, e = evaluate(x)
    host = [e + (0.5 * m[:, None] * v * v).sum(1).reshape(B, n).sum(1)]
    for _ in range(n_steps):
        v = v + 0.5 * dt * f / m[:, None]
        x = x + dt * v
        f, e = evaluate(x)
        v = v + 0.5 * dt * f / m[:, None]
        host.append(e + (0.5 * m[:, None] * v * v).sum(1).reshape(B, n).sum(1))
    host = np.asarray(host)
    a = np.abs(host - host[0]).max(axis=0)
    # (b) from the recorded trajectory, with the biased forces
    b_ = np.zeros(B)
    for k in range(n_steps):
        F = evaluate(_np(traj.pos[k]).astype(np.float64))[0]
        xk, vk = _np(traj.pos[k]), _np(traj.vel[k]).astype(np.float64)
        per_atom = (np.abs(F) * mr.half_ulp32(xk)).sum(1) + m * (vk * vk).sum(1) * mr.EPS32
        b_ += per_atom.reshape(B, n).sum(1)
    c = 2.0 * util.energy_tol(pe[0])
    bound = a + b_ + c
    swing = ue.max(axis=0) - ue.min(axis=0)
    print(f'energy conservation over {n_steps} steps in the restrained potential: drift {drift} eV, bound {bound} = host fp64 {a} + fp32 '
          f'state {b_} + energy ulps {c}; drift / bound {drift / bound}; restraint energy swing {swing} eV = {swing / bound} x bound')
    assert np.all(drift <= bound), f'drift / bound {drift / bound}'
    assert np.all(swing >= 10.0 * bound), f'restraint energy swing / bound {swing / bound}: the test has no power'


# ---- 8. the grid and the calculator ------------------------------------------------------------------------------------------------------

class FakeAtoms:
    """The accessors format_data() and run_metad() use (as in tests/test_ase_calculator.py)"""
    def __init__(self, numbers, positions):
        self.numbers, self.positions = np.asarray(numbers), np.asarray(positions, dtype=np.float64)

    def __len__(self):
        return len(self.numbers)

    def get_atomic_numbers(self):
        return self.numbers

    def get_positions(self, wrap=False):
        return self.positions

    def get_cell(self):
        return np.zeros((3, 3))

    def get_pbc(self):
        return np.zeros(3, dtype=bool)


def test_bias_on_grid_and_the_calculator_form():
    from newtonnet_amd.metadynamics import Metadynamics, BiasedTrajectory, free_energy_factor
    from newtonnet_amd.utils import MLAseCalculator
    z, pos, _, _ = _bench().synthetic_aspirin(2, 1, 'cpu')
    model = make_model(util.load_state('rand'))
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda')
    frames = [FakeAtoms(z[:21].numpy(), pos[21 * k:21 * (k + 1)].numpy()) for k in range(2)]
    keep = [f.positions.copy() for f in frames]
    cvs = [('torsion', 0, 1, 2, 3)]
    G, W, n_steps, pace = 2, 4, 12, 2
    args = (300.0, FRICTION, 0.02, 0.3, pace)
    kw = dict(bias_factor=GAMMA, walkers=W)
    out = calc.run_metad(frames, cvs, n_steps, *args, record_every=4, seed=5, **kw)
    H = W * (n_steps // pace)
    assert out['step'].tolist() == [4, 8, 12] and out['n_hills'].tolist() == [8, 16, 24]
    for k in ('positions', 'velocities'):
        assert out[k].shape == (3, G, W, 21, 3) and out[k].dtype == np.float32, k
    for k in ('energy', 'kinetic_energy', 'bias_energy', 'restraint_energy'):
        assert out[k].shape == (3, G, W) and out[k].dtype == np.float32, k
    assert out['cv'].shape == (3, G, W, 2) and out['hill_centers'].shape == (G, H, 2) and out['hill_heights'].shape == (G, H)
    # the model form on the same seed: bit for bit
    zc, pc = z.cuda(), pos.cuda()
    cell, batch = torch.zeros(2, 3, 3, device='cuda'), torch.repeat_interleave(torch.arange(2), 21).cuda()
    gen = torch.Generator(device='cuda').manual_seed(5)
    meta = model.metadynamics(zc, pc, cell, batch, cvs, *args, generator=gen, **kw)
    traj = meta.run(n_steps, 4)
    assert isinstance(meta, Metadynamics) and isinstance(traj, BiasedTrajectory)
    for name, key in (('pos', 'positions'), ('vel', 'velocities'), ('potential_energy', 'energy'), ('kinetic_energy', 'kinetic_energy'),
                      ('bias_energy', 'bias_energy'), ('restraint_energy', 'restraint_energy'), ('cv', 'cv')):
        assert _same(_np(getattr(traj, name)).reshape(out[key].shape), out[key]), name
    for g, (c, h) in enumerate(meta.hills):
        assert c.shape == (H, 1) and _same(_np(c)[:, 0], out['hill_centers'][g, :, 0]) and _same(_np(h), out['hill_heights'][g])
    assert all(np.array_equal(f.positions, k) for f, k in zip(frames, keep))
    one = calc.run_metad(frames[0], cvs, 4, *args, seed=5, **kw)                       # a single structure drops the G axis
    assert one['positions'].shape == (1, W, 21, 3) and one['cv'].shape == (1, W, 2) and one['hill_centers'].shape == (2 * W, 2)
    # the bias on a grid of 257 points across the period, against the reference's hill sum
    grid = np.linspace(-np.pi, np.pi, 257).astype(np.float32)
    V = _np(meta.bias_on_grid(torch.from_numpy(grid).cuda()))
    assert V.shape == (G, 257) and V.dtype == np.float32
    worst = {}
    par = _np(meta._hill_par)
    for g in range(G):
        rows = _np(meta._hills[g, :H])
        for i, s in enumerate(grid):
            ref, _, _, amb = br.hill_sum(rows, br.B(float(s)), br.B(0.0), par[g, 0], par[g, 1], br.TWO_PI32, 0.0)
            assert amb == 0, (g, i)
            _within(V[g, i], float(ref.v), C_bound(ref), worst, 'V on the grid')
        assert V[g].max() > 0.02
    print(f'bias_on_grid: worst err / bound {worst}')
    assert np.array_equal(V, _np(meta.bias_on_grid(grid)))                              # numbers or a tensor
    F = _np(meta.free_energy(grid))
    for g in range(G):
        want = br.free_energy(V[g].astype(np.float64), GAMMA)
        np.testing.assert_allclose(F[g], want, atol=8 * br.EPS32 * np.abs(free_energy_factor(GAMMA) * V[g]).max())
        assert F[g].min() == 0.0
    # the bias a walker felt at its last evaluation is the grid's function at its cv
    meta.run(1)                                                                         # (a step that deposits nothing)
    assert meta.n_hills == H
    cv_now, V_now = meta.collective_variables, meta.bias_energy
    again = torch.stack([meta.bias_on_grid(cv_now[g * W:(g + 1) * W])[g] for g in range(G)]).reshape(-1)
    assert torch.equal(again, V_now)


def C_bound(b):
    return br.C_BIAS * float(b.e) + br.TINY32
