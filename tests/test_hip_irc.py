"""Batched reaction-path following on the HIP path (newtonnet_amd/irc.py, csrc/irc.hip).

Kernel alone: nnhip_irc_step on synthetic inputs that reach every branch at every size class (tests/irc_ref.synthetic_batch;
tests/test_irc_host.py shows on the CPU that none of their decisions is ambiguous) against its fp64 restatement on the SAME fp32
inputs, every output within the derived bound (C_IRC = 2, 2 ulp for the roots) plus half an fp32 ulp of the stored value, integers
and flags exact, everything a step must not touch bitwise untouched; the tests print err / bound.  Driver: every recorded step is
checked ONE step at a time from the recorded frames alone, so no error compounds; the path itself is measured against a host fp64
loop of the same reference driven by model() forces."""
import math

import numpy as np
import pytest
import torch

from tests import irc_ref as ir
from tests import neb_ref as nr
from tests import util
from tests.test_hip_hessian import cuda, make_model

pytestmark = pytest.mark.gpu

SENT = 777.0
STATE = ir.INTS + ir.SCALARS + ir.ARRAYS
INPUTS = ('x', 'F', 'mass', 'ptr', 'free')


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _slice(d, b):
    """molecule b of a batch (the kernel's layout) as a batch of its own"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    out = dict(d, ptr=np.array([0, a1 - a0], dtype=np.int32))
    for k in ('x', 'F', 'mass', 'free') + ir.ARRAYS:
        out[k] = d[k][a0:a1]
    for k in ir.INTS + ir.SCALARS:
        out[k] = d[k][b:b + 1]
    return out


def _reversed(d):
    """the batch with its molecules in the opposite order"""
    B = len(d['ptr']) - 1
    parts = [_slice(d, b) for b in range(B - 1, -1, -1)]
    out = dict(d, ptr=np.concatenate([[0], np.cumsum([len(p['x']) for p in parts])]).astype(np.int32))
    for k in ('x', 'F', 'mass', 'free') + ir.ARRAYS + ir.INTS + ir.SCALARS:
        out[k] = np.concatenate([p[k] for p in parts])
    return out


def _tensors(d):
    return {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in INPUTS + STATE}


def _call(t, par, flags=0, use_mask=True, **over):
    from newtonnet_amd import hip
    p = dict(par, **over)
    hip.irc_step(t['x'], t['F'], t['free'] if use_mask else None, t['mass'], t['ptr'], p['v0'], p['delta0'], p['dt_min'], p['dt_max'],
                 p['tol2'], flags, t['status'], t['armed'], t['n_steps'], t['dt'], t['dt_prev'], t['arc'], t['vel'], t['x_prev'],
                 t['v_prev'], t['a_prev'], t['pos_out'], t['fmax'])


def _launch(d, flags=0, use_mask=True):
    """one launch on a batch in the kernel's layout; returns the inputs as they are afterwards and the outputs, as numpy arrays"""
    t = _tensors(d)
    N, B = d['x'].shape[0], len(d['ptr']) - 1
    t.update(pos_out=torch.full((N, 3), SENT, device='cuda'), fmax=torch.full((B,), SENT, device='cuda'))
    _call(t, d['par'], flags, use_mask)
    return {k: _np(v) for k, v in t.items()}


# ---- 1. the kernel against fp64 on the same inputs ---------------------------------------------------------------------------------

CASES = [(k, m, 0) for k in ir.SYN_KINDS for m in (True, False)] + [(k, True, ir.CHECK_ONLY) for k in ('ordinary', 'turned', 'stop_armed')]


@pytest.mark.parametrize('kind,use_mask,flags', CASES)
def test_irc_step_against_fp64_on_the_same_inputs(kind, use_mask, flags):
    d = ir.synthetic_batch(kind)
    d = d if use_mask else ir.unmasked(d)
    out = _launch(d, flags, use_mask)
    for k in INPUTS:
        assert _same_bits(out[k], d[k]), f'{k}: an input was written'
    worst = {}
    moved = frozen = 0
    for b in range(len(d['ptr']) - 1):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        ref = ir.batch_step(d, b, flags, use_mask)
        new = ref['state']
        what = f'{kind}, mask {use_mask}, flags {flags}: molecule {b} ({a1 - a0} atoms)'
        assert not any(ref['ambiguous'].values()), f'{what}: ambiguous {ref["ambiguous"]}'
        for k in ir.INTS:
            assert int(out[k][b]) == int(new[k]), f'{what}: {k} {out[k][b]} != {int(new[k])}'
        x, xo = d['x'][a0:a1], out['pos_out'][a0:a1]
        free = d['free'][a0:a1] if use_mask else np.ones(a1 - a0, dtype=bool)
        got = {k: out[k][a0:a1].astype(np.float64) for k in ir.ARRAYS}
        got.update({k: float(out[k][b]) for k in ir.SCALARS})
        for k, v in ir.compare(ref, xo, out['fmax'][b], got, x, what).items():
            worst[k] = max(worst.get(k, 0.0), v)
        for k in ir.ARRAYS:                               # a fixed atom's rows keep their bits (NaN here), in every array
            assert _same_bits(out[k][a0:a1][~free], d[k][a0:a1][~free]), f'{what}: {k} of a fixed atom was written'
        assert _same_bits(xo[~free], x[~free]), f'{what}: a fixed atom moved'
        if ref['frozen']:
            frozen += 1
            assert _same_bits(xo, x), f'{what}: a frozen molecule moved'
            for k in ir.ARRAYS:
                assert _same_bits(out[k][a0:a1], d[k][a0:a1]), f'{what}: {k} touched'
            for k in ir.SCALARS:
                assert _same_bits(out[k][b], d[k][b]), f'{what}: {k} touched'
            continue
        moved += 1
        assert np.isfinite(xo).all() and (kind == 'vzero' or (xo[free] != x[free]).any()), f'{what}: nothing moved'
        # x_prev = x_n and v_prev = vel bitwise, dt_prev = the dt of this step
        assert _same_bits(out['x_prev'][a0:a1][free], x[free]) and _same_bits(out['v_prev'][a0:a1][free], out['vel'][a0:a1][free]), what
        assert _same_bits(out['dt_prev'][b], d['dt'][b]), what
        dt, dtn, par = float(d['dt'][b]), float(out['dt'][b]), d['par']
        if kind == 'grow_max':
            assert dtn == par['dt_max'], f'{what}: dt {dtn}'
        elif kind == 'cap2':
            assert dtn == 2 * dt, f'{what}: dt {dtn}'
        elif kind == 'shrink_min':
            assert dtn == par['dt_min'], f'{what}: dt {dtn}'
        elif kind == 'first':
            assert dtn == dt and _same_bits(out['vel'][a0:a1], d['vel'][a0:a1]), what
    if flags or kind in ('turned', 'stop_armed', 'stopped'):
        assert moved == 0 and frozen == len(ir.SYN_SIZES) + 1
    else:
        assert moved == len(ir.SYN_SIZES) and frozen == 1
    print(f'irc_step {kind}, mask {use_mask}, flags {flags}: {moved} moved, {frozen} frozen, worst err / bound '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f' (C_IRC = {ir.C_IRC}, roots at {ir.ROOT_ULPS} ulp)')


# ---- 2. bitwise: repeats, the batch around a molecule, the mask ------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['ordinary', 'first', 'shrink_min'])
def test_repeats_and_each_molecule_alone_and_reversed_give_the_bits_of_the_batch(kind):
    d = ir.synthetic_batch(kind)
    whole, again, rev = _launch(d), _launch(d), _launch(_reversed(d))
    B = len(d['ptr']) - 1
    for k in ('pos_out', 'fmax') + STATE:
        assert _same_bits(whole[k], again[k]), f'{k}: two launches on the same inputs differ'
    for b in range(B):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        one = _launch(_slice(d, b))
        r = B - 1 - b
        r0, r1 = int(rev['ptr'][r]), int(rev['ptr'][r + 1])
        what = f'{kind}: molecule {b} ({a1 - a0} atoms)'
        for k in ('pos_out',) + ir.ARRAYS:
            assert _same_bits(one[k], whole[k][a0:a1]), f'{what}: {k} alone'
            assert _same_bits(rev[k][r0:r1], whole[k][a0:a1]), f'{what}: {k} in the reversed batch'
        for k in ('fmax',) + ir.INTS + ir.SCALARS:
            assert _same_bits(one[k], whole[k][b:b + 1]), f'{what}: {k} alone'
            assert _same_bits(rev[k][r:r + 1], whole[k][b:b + 1]), f'{what}: {k} in the reversed batch'


def test_a_null_mask_means_all_atoms_free():
    d = ir.unmasked(ir.synthetic_batch('ordinary'))
    a, b = _launch(d, 0, use_mask=True), _launch(d, 0, use_mask=False)
    for k in ('pos_out', 'fmax') + STATE:
        assert _same_bits(a[k], b[k]), k
    m = ir.synthetic_batch('ordinary')
    assert not _same_bits(_launch(m)['fmax'], _launch(dict(m, free=np.ones_like(m['free'])))['fmax'])   # and a mask does something


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------

def test_irc_step_refuses_bad_arguments_and_writes_nothing():
    from newtonnet_amd import hip
    d = _slice(ir.unmasked(ir.synthetic_batch('ordinary')), 2)
    n, par = d['x'].shape[0], d['par']
    assert n == 21

    def tensors():
        t = _tensors(d)
        t.update(pos_out=torch.full((n, 3), SENT, device='cuda'), fmax=torch.full((1,), SENT, device='cuda'))
        return t
    t = tensors()
    keep = {k: v.clone() for k, v in t.items()}
    with pytest.raises(hip.HipLibraryError, match='alias'):
        _call(dict(t, pos_out=t['x']), par)
    flat = torch.zeros(3 * n + 3, device='cuda')
    with pytest.raises(hip.HipLibraryError, match='alias'):          # an overlapping view is an alias too
        _call(dict(t, x=flat[:3 * n].view(n, 3), pos_out=flat[3:].view(n, 3)), par)
    with pytest.raises(hip.HipLibraryError, match='flags'):
        _call(t, par, flags=2)
    for name in ('v0', 'delta0', 'dt_min'):
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(hip.HipLibraryError, match=name):
                _call(t, par, **{name: bad})
    with pytest.raises(hip.HipLibraryError, match='dt_max'):
        _call(t, par, dt_max=0.5 * par['dt_min'])
    with pytest.raises(hip.HipLibraryError, match='dt_max'):
        _call(t, par, dt_max=float('nan'))
    for bad in (-1.0, float('nan')):
        with pytest.raises(hip.HipLibraryError, match='tol2'):
            _call(t, par, tol2=bad)
    # the wrapper's own checks: a state array of the wrong type or size would be copied or overrun
    with pytest.raises(ValueError, match='status'):
        _call(dict(t, status=t['status'].long()), par)
    with pytest.raises(ValueError, match='vel'):
        _call(dict(t, vel=t['vel'][:-1]), par)
    with pytest.raises(ValueError, match='free'):
        _call(dict(t, free=t['free'].float()), par)
    # null mandatory pointers: straight at the C ABI (the Python wrapper would not let a None through)
    L = hip.lib()
    order = ('x', 'F', 'free', 'mass', 'ptr', 'status', 'armed', 'n_steps', 'dt', 'dt_prev', 'arc', 'vel', 'x_prev', 'v_prev', 'a_prev',
             'pos_out', 'fmax')

    def raw(t, null=(), n_mol=1, n_atoms=n):
        p = {k: (None if k in null else hip._ptr(t[k])) for k in order}
        return L.nnhip_irc_step(p['x'], p['F'], p['free'], p['mass'], p['ptr'], n_mol, n_atoms, par['v0'], par['delta0'], par['dt_min'],
                                par['dt_max'], par['tol2'], 0, p['status'], p['armed'], p['n_steps'], p['dt'], p['dt_prev'], p['arc'],
                                p['vel'], p['x_prev'], p['v_prev'], p['a_prev'], p['pos_out'], p['fmax'], hip._stream(t['x'].device))
    for name in order:
        if name != 'free':                                            # (optional)
            assert raw(t, null=(name,)) != 0, f'a null {name} was accepted'
    assert raw(t, n_mol=-1) != 0 and raw(t, n_atoms=-1) != 0
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert _same_bits(_np(t[k]), _np(v)), f'{k} was written by a refused call'
    # empty batches are no-ops that succeed
    assert raw(t, n_mol=0) == 0 and raw(t, null=order, n_mol=0, n_atoms=0) == 0
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert _same_bits(_np(t[k]), _np(v)), f'{k} was written by an empty launch'
    assert raw(t) == 0                                                # and the same call with nothing wrong moves the molecule
    torch.cuda.synchronize()
    assert not _same_bits(_np(t['pos_out']), _np(keep['pos_out'])) and int(t['n_steps'][0]) == int(keep['n_steps'][0]) + 1


def test_a_molecule_with_impossible_state_is_left_alone_and_gets_nan():
    """status outside 0 .. 2, n_steps < 0, dt outside [dt_min, dt_max] or NaN, atom offsets that leave the arrays, a free atom whose
    mass is not finite and > 0: nothing of the molecule is written, fmax_out = NaN -- and its neighbours in the batch step on"""
    base = ir.unmasked(ir.synthetic_batch('ordinary'))
    good = _launch(base)
    b = 2
    a0, a1 = int(base['ptr'][b]), int(base['ptr'][b + 1])
    N = base['x'].shape[0]

    def changed(key, value, at=b):
        arr = base[key].copy()
        arr[at] = value
        return dict(base, **{key: arr})
    bad = [changed('status', 3), changed('status', -1), changed('n_steps', -1), changed('dt', 0.001), changed('dt', 5.0),
           changed('dt', np.nan)]
    bad += [changed('mass', m, at=a0 + 3) for m in (0.0, -1.0, np.nan, np.inf)]
    for d in bad:
        out = _launch(d)
        assert np.isnan(out['fmax'][b]) and np.all(out['pos_out'][a0:a1] == SENT)
        for k in STATE:
            assert _same_bits(out[k][b], d[k][b]) if k in ir.INTS + ir.SCALARS else _same_bits(out[k][a0:a1], d[k][a0:a1]), k
        for k in ('pos_out',) + ir.ARRAYS:                            # the others are the bits of the good launch
            assert _same_bits(out[k][:a0], good[k][:a0]) and _same_bits(out[k][a1:], good[k][a1:]), k
        assert _same_bits(np.delete(out['fmax'], b), np.delete(good['fmax'], b))
    # a fixed atom may hold any mass
    d = dict(changed('mass', np.nan, at=a0 + 3), free=changed('free', False, at=a0 + 3)['free'])
    out = _launch(d)
    assert np.isfinite(out['fmax'][b]) and np.isfinite(out['pos_out'][a0:a1]).all() and int(out['n_steps'][b]) == int(d['n_steps'][b]) + 1
    # offsets that leave the arrays: nothing is read or written for such a molecule
    one = _slice(base, b)
    for ptr in ([0, a1 - a0 + 5], [-1, a1 - a0], [4, 2]):
        d = dict(one, ptr=np.array(ptr, dtype=np.int32))
        out = _launch(d)
        assert np.isnan(out['fmax'][0]) and np.all(out['pos_out'] == SENT)
        for k in STATE:
            assert _same_bits(out[k], d[k]), k
    assert N > a1


# ---- 4. the driver -------------------------------------------------------------------------------------------------------------------------

def _setup(case, weights):
    z, pos, cell, batch, _ = util.case_inputs(case, torch.float32)
    z, pos, cell, batch = cuda(z, pos, cell, batch)
    return make_model(util.load_state(weights)), z, pos, cell, batch


DISPLACEMENT = 0.05      # amu^1/2 A: where both branches leave this saddle with the widest margin (the path test says why)


@pytest.fixture(scope='module')
def saddle():
    """the shipped model and the methyl-rotation saddle of aspirin, found as in tests/test_hip_neb.py: aspirin8_ckpt molecule 0
    relaxed on the device (endpoint A), then a 7-image band (spring 0.1 eV/A^2, climbing below 0.05 eV/A) -- but tightened to
    fmax = 0.0005 eV/A, because the 0.0064 eV/A which a band stopped at 0.01 leaves on the climbing image is as large as the gradient
    this soft mode builds up over the first 0.1 amu^1/2 A, and one branch would start uphill (the path test has the figures)"""
    model, z, pos, cell, batch = _setup('aspirin8_ckpt', 'ckpt')
    z1, c1, b1 = z[:21].contiguous(), cell[:1].contiguous(), batch[:21].contiguous()
    rel = model.relaxation(z1, pos[:21], c1, b1)
    res = rel.run(600, check_every=10)
    assert bool(res.converged.all())
    A = _np(res.pos).astype(np.float64)
    zA = _np(z1)
    x0 = nr.methyl_rotation_band(zA, A, 7).astype(np.float32)
    zb = z1.repeat(7)
    bb = torch.arange(7, device='cuda').repeat_interleave(21)
    band = model.band(zb, torch.from_numpy(x0.reshape(-1, 3)).cuda(), torch.zeros(7, 3, 3, device='cuda'), bb, 7, spring=0.1,
                      fmax=0.0005, climb_below=0.05)
    out = band.run(4000, check_every=20)
    top = int(out.saddle_image[0])
    S = out.pos[21 * top:21 * (top + 1)].clone()
    f_top = float(model(z1, S.clone(), c1, b1).gradient_force.norm(dim=1).max())
    print(f'band tightened to 0.0005 eV/A in {int(out.n_steps[0])} steps, true |f| on the climbing image {f_top:.2e} eV/A')
    assert bool(out.converged[0])
    return dict(model=model, z=z1, cell=c1, batch=b1, zA=zA, A=A, pos=S, energy_A=float(res.energy[0]))


def check_stepwise(path, start, res, label):
    """start: dict(pos, force, vel, arc, dt, status) before the first step; res: a PathResult recorded with record_every = 1.
    Frames k and k + 1 are consecutive steps: one irc_ref.irc_step per path, from the state rebuilt out of the frames <= k (vel, dt
    and arc as recorded; x_prev the position and a_prev = fl32(fl32(c f) / m) of the frame before, both bitwise the kernel's; armed
    carried by the reference), must land on frame k + 1 within the bound, taking dt from the record.  A path-step with an ambiguous
    decision is skipped and counted; the state then follows what the record shows the kernel decided.  Returns (path-steps,
    skipped, worst err / bound)."""
    f32 = np.float32
    ptr = _np(path._mol_ptr)
    mass = _np(path.masses)
    free = None if path._free is None else _np(path._free).astype(bool)
    par = dict(v0=path._v0, delta0=path._delta0, dt_min=path._dt_min, dt_max=path._dt_max, tol2=path._tol2)
    fr = [start] + [dict(pos=_np(res.traj_pos[k]), force=_np(res.traj_force[k]), vel=_np(res.traj_vel[k]), arc=_np(res.traj_arc[k]),
                         dt=_np(res.traj_dt[k]), status=_np(res.traj_status[k])) for k in range(res.traj_step.numel())]
    P = len(ptr) - 1
    armed = [0] * P
    n_steps = [0] * P
    total = skipped = 0
    worst, kinds = {}, {}
    for k in range(len(fr) - 1):
        cur, nxt = fr[k], fr[k + 1]
        for p in range(P):
            sl = slice(int(ptr[p]), int(ptr[p + 1]))
            m = mass[sl]
            fmask = None if free is None else free[sl]
            st = dict(status=int(cur['status'][p]), armed=armed[p], n_steps=n_steps[p], dt=float(cur['dt'][p]), dt_prev=0.0,
                      arc=float(cur['arc'][p]), vel=cur['vel'][sl].astype(np.float64))
            if n_steps[p] >= 1:
                prev = fr[k - 1]
                a_prev = ((f32(ir.ACCEL) * ir.masked(prev['force'][sl], fmask).astype(f32)).astype(f32) / m[:, None]).astype(f32)
                st.update(dt_prev=float(prev['dt'][p]), x_prev=prev['pos'][sl].astype(np.float64), v_prev=st['vel'].copy(),
                          a_prev=a_prev.astype(np.float64))
            else:
                z3 = np.zeros_like(st['vel'])
                st.update(x_prev=z3, v_prev=z3.copy(), a_prev=z3.copy())
            ref = ir.irc_step(cur['pos'][sl], cur['force'][sl], fmask, m, st, par)
            total += 1
            what = f'{label}: step {k} -> {k + 1}, path {p}'
            got_status = int(nxt['status'][p])
            if any(ref['ambiguous'].values()):
                skipped += 1
                for name, flag in ref['ambiguous'].items():
                    kinds[name] = kinds.get(name, 0) + bool(flag)
                moved = not _same_bits(nxt['pos'][sl], cur['pos'][sl])
                ref = ir.irc_step(cur['pos'][sl], cur['force'][sl], fmask, m, st, par,
                                  decide=dict(status=got_status, armed=ref['state']['armed']))
                assert moved or got_status != 0 or not np.any(ir.masked(cur['force'][sl], fmask)), what
            else:
                assert ref['state']['status'] == got_status, f'{what}: status {got_status}, reference {ref["state"]["status"]}'
                # (the record holds neither fmax nor the stored acceleration of a step: the next step's a_prev is rebuilt from forces)
                got = dict(vel=nxt['vel'][sl], dt=float(nxt['dt'][p]), arc=float(nxt['arc'][p]))
                for name, v in ir.compare(ref, nxt['pos'][sl], None, got, cur['pos'][sl], what, skip=('fmax', 'acc')).items():
                    if not ref['frozen']:
                        worst[name] = max(worst.get(name, 0.0), v)
                if ref['frozen']:
                    assert _same_bits(nxt['pos'][sl], cur['pos'][sl]) and _same_bits(nxt['vel'][sl], cur['vel'][sl]), what
                    assert _same_bits(nxt['dt'][p], cur['dt'][p]) and _same_bits(nxt['arc'][p], cur['arc'][p]), what
            armed[p] = ref['state']['armed']
            n_steps[p] = ref['state']['n_steps']
    print(f'{label}: {total} path-steps, {skipped} skipped as ambiguous {kinds}, worst err / bound '
          + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()))
    return total, skipped, n_steps


def _start(path):
    return dict(pos=_np(path.positions), force=_np(path.forces), vel=_np(path.velocities), arc=_np(path.arc_length),
                dt=_np(path.timestep), status=_np(path.status))


@pytest.mark.parametrize('case', ['aspirin', 'mixed_rand'])
def test_every_recorded_step_follows_from_the_frames_before(case, saddle):
    if case == 'aspirin':
        model = saddle['model']
        z, pos, cell, batch = saddle['z'], saddle['pos'], saddle['cell'], saddle['batch']
        path = model.reaction_path(z, pos, cell, batch, both=True, initial_displacement=DISPLACEMENT)
    else:
        model, z, pos, cell, batch = _setup('mixed_rand', 'rand')
        g = torch.Generator().manual_seed(11)
        path = model.reaction_path(z, pos, cell, batch, direction=torch.randn(pos.shape[0], 3, generator=g).cuda(), both=True)
    P = 2 * cell.shape[0]
    assert path.n_mol == P and path.n_atoms == 2 * pos.shape[0]
    start = _start(path)
    before = model.deferred_stats()
    res = path.run(40, check_every=0, record_every=1)
    after = model.deferred_stats()
    assert after['repeats_needed'] == before['repeats_needed']
    assert res.traj_step.tolist() == list(range(1, 41)) and res.traj_pos.shape == (40, 2 * pos.shape[0], 3)
    assert res.traj_force.shape == res.traj_vel.shape == res.traj_pos.shape
    assert res.traj_energy.shape == res.traj_arc.shape == res.traj_dt.shape == res.traj_status.shape == (40, P)
    # the recorded forces and energies are the model's at the recorded positions (a repeat from the wrong buffer would show here)
    worst_f = worst_e = 0.0
    frames = [(torch.from_numpy(start['pos']).cuda(), path.forces.new_tensor(start['force']), None)]
    frames += [(res.traj_pos[k], res.traj_force[k], res.traj_energy[k]) for k in range(40)]
    for p, f, e in frames:
        out = model(path.z, p, path.cell, path.batch)
        worst_f = max(worst_f, float((out.gradient_force - f).abs().max()))
        if e is not None:
            de = _np(out.energy).astype(np.float64) - _np(e).astype(np.float64)
            worst_e = max(worst_e, float((np.abs(de) / util.energy_tol(_np(e))).max()))
    print(f'{case}: recorded against model(recorded positions): forces {worst_f:.3e} eV/A (allowed {util.FORCE_MAX_TOL}), energies '
          f'{worst_e:.3f} of util.energy_tol')
    assert worst_f <= util.FORCE_MAX_TOL and worst_e <= 1.0
    total, skipped, n_steps = check_stepwise(path, start, res, case)
    assert total == 40 * P and skipped <= 0.01 * total, f'{skipped} of {total} path-steps are ambiguous'
    assert n_steps == res.n_steps.tolist()
    assert torch.equal(res.pos, res.traj_pos[-1]) and torch.equal(res.energy, res.traj_energy[-1])
    assert torch.equal(res.arc_length, res.traj_arc[-1]) and torch.equal(res.status, res.traj_status[-1])
    # the two branches leave the saddle in opposite directions, from the same distance
    x = start['pos'].reshape(-1)
    ptr = _np(path._mol_ptr)
    s = _np(pos)
    for b in range(cell.shape[0]):
        fwd, back = slice(int(ptr[2 * b]), int(ptr[2 * b + 1])), slice(int(ptr[2 * b + 1]), int(ptr[2 * b + 2]))
        mid = s[int(ptr[2 * b]) // 2:int(ptr[2 * b]) // 2 + fwd.stop - fwd.start]
        assert np.allclose(start['pos'][fwd] - mid, -(start['pos'][back] - mid), atol=2e-6)
        assert np.array_equal(start['vel'][fwd], -start['vel'][back])
    assert np.all(start['arc'] == np.float32(DISPLACEMENT if case == 'aspirin' else 0.1)) and np.all(start['dt'] == np.float32(0.25)) and x.size
    ptr_l = ptr.astype(np.int64)
    speed = np.sqrt(np.add.reduceat((start['vel'].astype(np.float64) ** 2).sum(1), ptr_l[:-1]))
    assert np.allclose(speed, 0.02, rtol=1e-6)


RESULT = ('pos', 'energy', 'fmax', 'status', 'n_steps', 'arc_length')


def test_bitwise_properties_of_the_driver(saddle):
    model = saddle['model']
    z, pos, cell, batch = saddle['z'], saddle['pos'], saddle['cell'], saddle['batch']
    keep = [t.clone() for t in (z, pos, cell, batch)]
    fixed = torch.zeros(21, dtype=torch.bool, device='cuda')
    fixed[::5] = True

    def make(**kw):
        return model.reaction_path(z, pos, cell, batch, **dict(dict(initial_displacement=DISPLACEMENT), **kw))
    a = make().run(40, 0, record_every=1)
    assert a.traj_step.tolist() == list(range(1, 41))
    # run(13); run(27) leaves the bits of run(40); record_every and check_every change no bit
    path = make()
    first = path.run(13, 0, record_every=0)
    assert path.step_count == 13 and first.traj_pos is None and first.n_steps.tolist() == [13, 13]
    second = path.run(27, 10, record_every=7)
    assert second.traj_step.tolist() == [20, 27, 34, 40]
    for name in RESULT:
        assert torch.equal(getattr(a, name), getattr(second, name)), name
    assert torch.equal(first.pos, a.traj_pos[12]) and torch.equal(first.energy, a.traj_energy[12])
    assert torch.equal(second.traj_pos, a.traj_pos[[19, 26, 33, 39]]) and torch.equal(second.traj_dt, a.traj_dt[[19, 26, 33, 39]])
    assert torch.equal(path.positions, a.pos)
    for record, check in ((0, 0), (7, 1), (0, 7)):
        b = make().run(40, check, record_every=record)
        for name in RESULT:
            assert torch.equal(getattr(a, name), getattr(b, name)), f'record_every {record}, check_every {check}: {name}'
    # both=False is the forward branch alone, bit for bit
    f = make(both=False).run(40, 0, record_every=0)
    assert f.pos.shape == (21, 3) and torch.equal(f.pos, a.pos[:21]) and torch.equal(f.arc_length, a.arc_length[:1])
    assert torch.equal(f.energy, a.energy[:1])
    with pytest.raises(ValueError, match='both'):
        f.profile(0)
    # fixed atoms never move, the others do
    h = make(fixed=fixed).run(40, 0, record_every=1)
    held = fixed.repeat(2)
    assert torch.equal(h.traj_pos[:, held], pos[fixed].repeat(2, 1).expand(40, -1, -1)) and (h.pos[~held] != pos.repeat(2, 1)[~held]).any()
    # a stopped path keeps every bit.  0.3 amu^1/2 A along the straight line of a rotation stretches the C-H bonds: the force is
    # against the velocity from the start and both branches stop as `turned` after their first step (F.v = -0.002 on the CPU oracle)
    s = make(initial_displacement=0.3)
    r = s.run(30, 0, record_every=1)
    n = r.n_steps.tolist()
    assert r.status.tolist() == [2, 2] and max(n) < 30, (r.status.tolist(), n)
    for p, k in enumerate(n):
        sl = slice(21 * p, 21 * (p + 1))
        assert torch.equal(r.traj_pos[k - 1:, sl], r.traj_pos[k - 1, sl].expand(31 - k, 21, 3)), f'path {p} moved after step {k}'
        assert torch.equal(r.traj_arc[k - 1:, p], r.traj_arc[k - 1, p].expand(31 - k))
        assert torch.equal(r.traj_dt[k - 1:, p], r.traj_dt[k - 1, p].expand(31 - k))
    # the caller's tensors are never modified
    for t, k in zip((z, pos, cell, batch), keep):
        assert torch.equal(t, k)
    assert not pos.requires_grad


# ---- 5. the path ---------------------------------------------------------------------------------------------------------------------------

def _torsion(zA, x):
    """the dihedral (degrees) of the first methyl hydrogen about the C-C axis against the next heavy atom along the chain"""
    c, heavy, hs = nr.methyl(zA, x)
    d = np.linalg.norm(x[:, None] - x[None], axis=2)
    nb = [int(j) for j in np.flatnonzero((zA > 1) & (d[heavy] < 1.75)) if j not in (c, heavy)][0]
    b1, b2, b3 = x[c] - x[hs[0]], x[heavy] - x[c], x[nb] - x[heavy]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    m1 = np.cross(n1, b2 / np.linalg.norm(b2))
    return math.degrees(math.atan2(m1 @ n2, n1 @ n2))


def test_both_branches_run_down_to_the_methyl_minima_like_the_host_fp64_loop(saddle):
    """Methyl rotation of aspirin, shipped weights.  The band of tests/test_hip_neb.py stops at a NEB force of 0.01 eV/A, which
    leaves a true force of 0.0064 eV/A on the climbing image: as large as the gradient the mode (110i cm^-1, -0.054 eV/(A^2 amu))
    builds up over 0.1 amu^1/2 A, so one branch would start uphill.  On the CPU oracle (fp64 model and host loop) that is what
    happens: from that saddle the forward branch fails the turned test at its first step (F.v = -1.7e-4 eV/fs at the start of 0.1)
    for the initial displacements 0.1, 0.2, 0.3 and 0.5, and even with the band tightened to 0.002 eV/A it passes only at 0.05 and
    0.06 (of 0.02 .. 0.1), with F.v = +1e-6 and +3e-6.  Chosen here: the band tightened to fmax = 0.0005 eV/A (true force 2.3e-5 eV/A on the oracle, 2027 band
    steps) and initial_displacement = 0.05 amu^1/2 A, where the oracle gives F.v = +4.8e-5 and +4.4e-5 eV/fs at the second launch
    on the two branches (cos 0.08 and 0.07), the largest margin of the displacements 0.02 .. 0.1 tried -- at 0.1 the straight line
    along this ROTATION has stretched the C-H bonds so far that the margin is down to 4e-6.  Everything else is the default.
    The yardstick is irc_ref.follow (fp64 positions and arithmetic) driven by model() from the same start.  Both device branches
    must stop (status 1 or 2) within 1.5 x the host loop's steps, with an arc length within 2 x the host loop's largest single
    step of the host's (an end point is only defined to one step), energies that never rise by more than 2 util.energy_tol along a
    branch, methyl torsions that move in opposite senses, end points from which model.relaxation reaches the energy of endpoint A
    within 2 util.energy_tol (three-fold symmetry), and a profile with its maximum at the saddle.
    On the CPU oracle: forward 43 steps to arc 1.692 amu^1/2 A (torsion 70.7 -> 126.9 degrees), backward 51 steps to 2.037 (67.4
    -> 5.7 degrees), both `turned`, largest step 0.042, end points 0.0372 and 0.0371 eV below the saddle (barrier 0.0378), relaxed
    end points 0.03806 and 0.03804 eV below it.
    Measured on an MI355X when the test was written: band tightened in 2059 steps (true |f| on the climbing image 3.9e-4 eV/A); device 43 and 51 steps (limit 76), both
    `turned`, arc 1.6918 and 2.0373 amu^1/2 A, 0.0328 and 0.0325 eV/A left at the end points, which lie 0.0371 eV below the
    saddle; host fp64 loop on model() forces 43 and 51 steps, arc 1.6919 and 2.0373, largest step 0.0416 and 0.0417; torsion 70.7
    -> 126.9 and 67.4 -> 5.7 degrees; relaxation from the end points in 26 and 21 steps to the fp32 energy of endpoint A exactly
    (allowed 0.0078 eV); the profile is flat to the last bit within 0.07 amu^1/2 A of the saddle, its maximum."""
    model, z1, zA = saddle['model'], saddle['z'], saddle['zA']
    S = saddle['pos']
    path = model.reaction_path(z1, S, saddle['cell'], saddle['batch'], both=True, initial_displacement=DISPLACEMENT)
    start = _start(path)
    e_start = _np(path.potential_energy).astype(np.float64)
    mass = _np(path.masses).astype(np.float64)

    def energy_forces(x):
        out = model(path.z, torch.from_numpy(x).float().cuda(), path.cell, path.batch)
        return _np(out.energy).astype(np.float64), _np(out.gradient_force).astype(np.float64)
    host = ir.follow(energy_forces, start['pos'].astype(np.float64), start['vel'].astype(np.float64), mass, [0, 21, 42], arc0=0.05,
                     max_steps=400)
    assert all(s in (1, 2) for s in host['status']), f'the host loop did not stop: {host["status"]} after {host["n_steps"]} steps'
    limit = int(math.floor(1.5 * host['n_steps'].max()))
    res = path.run(limit, check_every=5, record_every=1)
    n, status, arc = res.n_steps.tolist(), res.status.tolist(), _np(res.arc_length).astype(np.float64)
    ends = _np(res.pos).astype(np.float64).reshape(2, 21, 3)
    tors = [(_torsion(zA, start['pos'][21 * p:21 * (p + 1)].astype(np.float64)), _torsion(zA, ends[p])) for p in range(2)]
    E_s = float(res.profile(0)[1][res.profile(0)[0] == 0][0])
    print(f'device: status {status}, steps {n}, arc {arc.round(4).tolist()}, fmax at the end {_np(res.fmax).round(4).tolist()}, saddle - end '
          f'{(E_s - _np(res.energy).astype(np.float64)).round(5).tolist()} eV; host fp64 loop: status {host["status"].tolist()}, steps '
          f'{host["n_steps"].tolist()}, arc {host["arc"].round(4).tolist()}, largest step {host["max_step"].round(4).tolist()} (limit {limit} '
          f'steps); torsion forward {tors[0][0]:.1f} -> {tors[0][1]:.1f}, backward {tors[1][0]:.1f} -> {tors[1][1]:.1f} degrees')
    for p in range(2):
        assert status[p] in (1, 2), f'branch {p} has not stopped within {limit} steps'
        assert n[p] <= math.floor(1.5 * host['n_steps'][p]), f'branch {p}: {n[p]} steps, host {host["n_steps"][p]}'
        assert abs(arc[p] - host['arc'][p]) <= 2.0 * host['max_step'][p], f'branch {p}: arc {arc[p]}, host {host["arc"][p]}'
        E = _np(res.traj_energy[:, p]).astype(np.float64)
        E = np.concatenate([[float(_np(path._saddle_energy)[0]), e_start[p]], E])
        rise = float(np.diff(E).max())
        assert rise <= 2.0 * float(util.energy_tol(E[0])), f'branch {p}: the energy rises by {rise:.2e} eV in one step'
    assert (tors[0][1] - tors[0][0]) * (tors[1][1] - tors[1][0]) < 0 and min(abs(t[1] - t[0]) for t in tors) > 30.0
    # the end points relax into the minimum of endpoint A (the methyl group has turned by +-60 degrees: three-fold symmetry)
    rel = model.relaxation(path.z, res.pos, path.cell, path.batch)
    relaxed = rel.run(300, check_every=10)
    tol = 2.0 * float(util.energy_tol(saddle['energy_A']))
    dE = _np(relaxed.energy).astype(np.float64) - saddle['energy_A']
    print(f'relaxed end points: {relaxed.n_steps.tolist()} steps, energy - E(A) {dE.tolist()} eV (allowed {tol:.4f}), barrier '
          f'{E_s - saddle["energy_A"]:.5f} eV')
    assert bool(relaxed.converged.all()) and np.all(np.abs(dE) <= tol)
    a, e, x = res.profile(0)
    k0 = int((a == 0).nonzero()[0])
    print(f'profile around the saddle: arc {a[k0 - 4:k0 + 5].tolist()}, energy - max {(e[k0 - 4:k0 + 5] - e.max()).tolist()}')
    assert k0 == n[1] + 1 and float(e[k0]) == float(e.max()) and torch.equal(x[k0], S) and bool((a[1:] > a[:-1]).all())
    assert abs(float(a[0]) + arc[1]) < 1e-6 and abs(float(a[-1]) - arc[0]) < 1e-6 and a.numel() == n[0] + n[1] + 3


# ---- 6. interfaces ------------------------------------------------------------------------------------------------------------------------

def test_a_minimum_is_refused_without_a_direction(saddle):
    from newtonnet_amd.irc import ReactionPath
    model, z, cell, batch = saddle['model'], saddle['z'], saddle['cell'], saddle['batch']
    A = torch.from_numpy(saddle['A']).float().cuda()
    with pytest.raises(ValueError, match='imaginary'):
        model.reaction_path(z, A, cell, batch)
    g = torch.Generator().manual_seed(3)
    path = model.reaction_path(z, A, cell, batch, direction=torch.randn(21, 3, generator=g).cuda())     # with one it is served
    assert isinstance(path, ReactionPath) and path.n_mol == 2
    with pytest.raises(ValueError, match='vanishes'):
        model.reaction_path(z, A, cell, batch, direction=torch.zeros(21, 3, device='cuda'))
    with pytest.raises(ValueError, match='masses'):
        model.reaction_path(z, A, cell, batch, direction=torch.ones(21, 3, device='cuda'), masses=torch.zeros(21, device='cuda'))
    with pytest.raises(ValueError, match='is on'):
        model.reaction_path(z, A, cell, batch, direction=torch.ones(21, 3))
    for bad in (dict(max_steps=-1), dict(max_steps=3, check_every=-1), dict(max_steps=3, record_every=2.5)):
        with pytest.raises(ValueError):
            path.run(**bad)
    # the sign convention: the component of largest magnitude of the direction is positive, whatever sign came in
    d = torch.randn(21, 3, generator=g).cuda()
    p1, p2 = (model.reaction_path(z, A, cell, batch, direction=s * d) for s in (1.0, -1.0))
    assert torch.equal(p1.positions, p2.positions) and torch.equal(p1.velocities, p2.velocities)
    big = int(d.abs().reshape(-1).argmax())
    assert float(p1.velocities[:21].reshape(-1)[big]) > 0 > float(p1.velocities[21:].reshape(-1)[big])


def test_calculator_irc_equals_the_model_path(saddle):
    from newtonnet_amd.irc import PathResult
    from newtonnet_amd.utils import MLAseCalculator
    from tests.test_hip_md import FakeAtoms
    model, zA = saddle['model'], saddle['zA']
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda')
    S = _np(saddle['pos'])
    other = S + np.array([0.5, -0.3, 0.2], dtype=np.float32)              # the same saddle somewhere else: other numbers
    frames = [FakeAtoms(zA, S), FakeAtoms(zA, other)]
    keep = [f.positions.copy() for f in frames]
    out = calc.irc(frames, max_steps=25, record_every=5, initial_displacement=DISPLACEMENT)
    assert all(np.array_equal(f.positions, k) for f, k in zip(frames, keep))
    z = torch.from_numpy(np.tile(zA, 2)).long().cuda()
    pos = torch.from_numpy(np.concatenate([S, other])).cuda()
    batch = torch.arange(2, device='cuda').repeat_interleave(21)
    path = model.reaction_path(z, pos, torch.zeros(2, 3, 3, device='cuda'), batch, initial_displacement=DISPLACEMENT)
    along = _np(path.velocities[:21])
    res = path.run(25, check_every=10, record_every=5)
    assert isinstance(res, PathResult) and res.n_steps.tolist() == [25] * 4
    for k, name in (('status', 'status'), ('n_steps', 'n_steps'), ('fmax', 'fmax'), ('arc_length', 'arc_length')):
        assert out[k].shape == (2, 2) and np.array_equal(out[k], _np(getattr(res, name)).reshape(2, 2)), k
    for b in range(2):
        arc, energy, xyz = (_np(t) for t in res.profile(b))
        assert np.array_equal(out['arc'][b], arc) and np.array_equal(out['energy'][b], energy) and np.array_equal(out['positions'][b], xyz)
        images = out['images'][b]
        assert len(images) == len(arc) == 2 * (1 + 5) + 1             # per branch: the start and 5 recorded steps; the saddle between
        assert np.all(np.diff(arc) > 0) and arc[6] == 0 and arc[5] == -np.float32(DISPLACEMENT) and arc[7] == np.float32(DISPLACEMENT)
        assert np.array_equal(xyz[6], _np(pos[21 * b:21 * (b + 1)]))
        assert np.array_equal(xyz[-1], _np(res.pos[42 * b:42 * b + 21])) and np.array_equal(xyz[0], _np(res.pos[42 * b + 21:42 * b + 42]))
        for k, image in enumerate(images):
            assert isinstance(image, FakeAtoms) and np.array_equal(image.positions, xyz[k].astype(np.float64))
            assert image.info['energy'] == float(energy[k]) and image.info['arc_length'] == float(arc[k])
            assert np.array_equal(image.get_atomic_numbers(), zA)
    # a single frame drops the frame axis; a direction of the caller's is taken as it is (here: the mode the device found)
    one = calc.irc(frames[0], direction=along, max_steps=7, record_every=0, initial_displacement=DISPLACEMENT)
    assert one['status'].shape == (2,) and one['n_steps'].tolist() == [7, 7] and len(one['images']) == 5 and one['arc'].shape == (5,)
