"""Batched geometry relaxation on the HIP path (newtonnet_amd/relax.py, csrc/relax.hip).

Kernel alone: nnhip_lbfgs_step on synthetic inputs that reach every branch at every size class (tests/relax_ref.synthetic_batch;
tests/test_relax_host.py shows on the CPU that none of its decisions is ambiguous) against its fp64 restatement on the SAME fp32
inputs, every output within the derived first-order bound (C_RX = 2) plus half an fp32 ulp of the stored value, integers and flags
exact, everything a step must not touch bitwise untouched; the tests print err / bound.  Driver: every recorded step is checked
ONE step at a time from the recorded frames alone, so no error compounds; convergence is measured against a host fp64 loop of the
same reference driven by model() forces."""
import math

import numpy as np
import pytest
import torch

from tests import relax_ref as rr
from tests import util
from tests.test_hip_hessian import cuda, make_model

pytestmark = pytest.mark.gpu

SENT = 777.0
INTS = ('converged', 'n_steps', 'n_pairs', 'head')


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def syn():
    return rr.synthetic_batch()


def _slice(d, b):
    """molecule b of a batch (the kernel's layout) as a batch of its own"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    out = dict(d, ptr=np.array([0, a1 - a0], dtype=np.int32))
    for k in ('x', 'F', 'f_prev', 'free'):
        out[k] = d[k][a0:a1]
    for k in ('S', 'Y'):
        out[k] = np.ascontiguousarray(d[k][:, a0:a1])
    out['rho'] = d['rho'][b:b + 1]
    for k in INTS:
        out[k] = d[k][b:b + 1]
    return out


def _launch(d, flags=0, use_mask=True):
    """one launch on a batch in the kernel's layout; returns the inputs as they are afterwards and the outputs, as numpy arrays"""
    from newtonnet_amd import hip
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ('x', 'F', 'f_prev', 'S', 'Y', 'rho', 'ptr', 'free') + INTS}
    N, B = d['x'].shape[0], len(d['ptr']) - 1
    pos_out = torch.full((N, 3), SENT, device='cuda')
    fmax = torch.full((B,), SENT, device='cuda')
    work = torch.full((N, 3), SENT, device='cuda')
    hip.lbfgs_step(t['x'], t['F'], t['free'] if use_mask else None, t['ptr'], d['memory'], d['tol2'], d['alpha'], d['maxstep'], flags,
                   t['converged'], t['n_steps'], t['n_pairs'], t['head'], t['S'], t['Y'], t['rho'], t['f_prev'], work, pos_out, fmax)
    out = {k: _np(v) for k, v in t.items()}
    out.update(pos_out=_np(pos_out), fmax=_np(fmax))
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the kernel against fp64 on the same inputs ---------------------------------------------------------------------------------

@pytest.mark.parametrize('flags', [0, rr.CHECK_ONLY])
def test_lbfgs_step_against_fp64_on_the_same_inputs(syn, flags):
    d = syn
    out = _launch(d, flags)
    assert _same_bits(out['x'], d['x']) and _same_bits(out['F'], d['F']) and _same_bits(out['ptr'], d['ptr'])       # inputs intact
    worst = dict(x=0.0, fmax=0.0, rho=0.0)
    seen = set()
    for b, kind in enumerate(d['kinds']):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        st = rr.batch_state(d, b)
        ref = rr.batch_step(d, b, flags)
        new = ref['state']
        what = f'molecule {b} ({kind}, {a1 - a0} atoms, flags {flags})'
        seen.add((kind, ref['frozen'], ref['accepted'], ref['clamped']))
        for k in INTS:
            assert int(out[k][b]) == int(new[k]), f'{what}: {k} {out[k][b]} != {int(new[k])}'
        e, bound = abs(float(out['fmax'][b]) - ref['fmax']), ref['b_fmax'] + rr.half_ulp32(ref['fmax'])
        assert e <= bound, f'{what}: fmax err / bound {e / bound:.3f}'
        worst['fmax'] = max(worst['fmax'], e / bound)
        x, xo = d['x'][a0:a1], out['pos_out'][a0:a1]
        free = d['free'][a0:a1]
        S1, Y1, rho1 = out['S'][:, a0:a1], out['Y'][:, a0:a1], out['rho'][b]
        S0, Y0, rho0 = d['S'][:, a0:a1], d['Y'][:, a0:a1], d['rho'][b]
        if ref['frozen']:
            assert _same_bits(xo, x), f'{what}: a frozen molecule moved'
            assert _same_bits(S1, S0) and _same_bits(Y1, Y0) and _same_bits(rho1, rho0), f'{what}: history touched'
            assert _same_bits(out['f_prev'][a0:a1], d['f_prev'][a0:a1]), f'{what}: f_prev touched'
            continue
        err = np.abs(xo.astype(np.float64) - ref['x_out'])
        bx = ref['bx'] + rr.half_ulp32(ref['x_out'])
        assert np.all(err <= bx), f'{what}: positions err / bound {float((err / bx).max()):.3f}'
        worst['x'] = max(worst['x'], float((err / bx).max()))
        assert _same_bits(xo[~free], x[~free]), f'{what}: a fixed atom moved'
        assert (xo[free] != x[free]).any(), f'{what}: nothing moved'
        h0, h1 = st['head'], new['head']
        # S[new head] = fl32(pos_out - pos_in) on the stored values, bitwise; f_prev = the masked forces, bitwise
        assert _same_bits(S1[h1], rr.stored_s(xo, x).astype(np.float32)), f'{what}: S[head]'
        assert _same_bits(out['f_prev'][a0:a1], rr.masked(d['F'][a0:a1], free).astype(np.float32)), f'{what}: f_prev'
        for k in range(d['memory']):
            if k != h1:
                assert _same_bits(S1[k], S0[k]), f'{what}: S[{k}] touched'
            if not (ref['accepted'] and k == h0):
                assert _same_bits(Y1[k], Y0[k]) and _same_bits(rho1[k], rho0[k]), f'{what}: Y / rho [{k}] touched'
        if ref['accepted']:
            assert _same_bits(Y1[h0], new['Y'][h0].astype(np.float32)), f'{what}: Y[head] is not fl32(f_prev - f)'
            e, bound = abs(float(rho1[h0]) - new['rho'][h0]), ref['b_rho_new'] + rr.half_ulp32(new['rho'][h0])
            assert e <= bound, f'{what}: rho err / bound {e / bound:.3f}'
            worst['rho'] = max(worst['rho'], e / bound)
    if flags == 0:
        for want in ([('accept', False, True, c) for c in (False, True)] + [('first', False, None, c) for c in (False, True)]
                     + [(k, False, False, c) for k in ('reject_neg', 'reject_cos') for c in (False, True)]
                     + [('converged', True, None, False), ('converging', True, None, False), ('empty', True, None, False)]):
            assert want in seen, want
    print(f'lbfgs_step flags = {flags}, {len(d["kinds"])} molecules, {d["x"].shape[0]} atoms: worst err / bound '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f' (C_RX = {rr.C_RX})')


def test_a_null_mask_means_all_atoms_free(syn):
    d = dict(syn, free=np.ones_like(syn['free']))
    a, b = _launch(d, 0, use_mask=True), _launch(d, 0, use_mask=False)
    for k in ('pos_out', 'fmax', 'S', 'Y', 'rho', 'f_prev') + INTS:
        assert _same_bits(a[k], b[k]), k
    assert not _same_bits(a['pos_out'], _launch(syn, 0)['pos_out'])          # and the mask of the other tests does something


# ---- 2. a molecule's result does not depend on the batch ----------------------------------------------------------------------------

def test_each_molecule_alone_gives_the_bits_it_gave_in_the_batch(syn):
    d = syn
    whole = _launch(d, 0)
    for b in range(len(d['kinds'])):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        one = _launch(_slice(d, b), 0)
        what = f'molecule {b} ({d["kinds"][b]}, {a1 - a0} atoms)'
        assert _same_bits(one['pos_out'], whole['pos_out'][a0:a1]) and _same_bits(one['fmax'], whole['fmax'][b:b + 1]), what
        assert _same_bits(one['S'], whole['S'][:, a0:a1]) and _same_bits(one['Y'], whole['Y'][:, a0:a1]), what
        assert _same_bits(one['rho'], whole['rho'][b:b + 1]) and _same_bits(one['f_prev'], whole['f_prev'][a0:a1]), what
        for k in INTS:
            assert _same_bits(one[k], whole[k][b:b + 1]), f'{what}: {k}'


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------

def test_lbfgs_step_refuses_aliases_null_pointers_and_bad_memory(syn):
    from newtonnet_amd import hip
    d = _slice(syn, 40)
    n, m = d['x'].shape[0], d['memory']
    assert n > 0

    def tensors():
        t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ('x', 'F', 'f_prev', 'S', 'Y', 'rho', 'ptr', 'free') + INTS}
        t.update(pos_out=torch.full((n, 3), SENT, device='cuda'), fmax=torch.full((1,), SENT, device='cuda'),
                 work=torch.full((n, 3), SENT, device='cuda'))
        return t

    def call(t, memory=m, flags=0, alpha=d['alpha'], maxstep=d['maxstep'], tol2=d['tol2']):
        hip.lbfgs_step(t['x'], t['F'], t['free'], t['ptr'], memory, tol2, alpha, maxstep, flags, t['converged'], t['n_steps'],
                       t['n_pairs'], t['head'], t['S'], t['Y'], t['rho'], t['f_prev'], t['work'], t['pos_out'], t['fmax'])
    t = tensors()
    keep = {k: v.clone() for k, v in t.items()}
    with pytest.raises(hip.HipLibraryError, match='alias'):
        call(dict(t, pos_out=t['x']))
    flat = torch.zeros(3 * n + 3, device='cuda')
    with pytest.raises(hip.HipLibraryError, match='alias'):          # an overlapping view is an alias too
        call(dict(t, x=flat[:3 * n].view(n, 3), pos_out=flat[3:].view(n, 3)))
    with pytest.raises(hip.HipLibraryError, match='memory'):
        call(dict(t, S=t['S'][:0], Y=t['Y'][:0], rho=t['rho'][:, :0]), memory=0)
    with pytest.raises(hip.HipLibraryError, match='flags'):
        call(t, flags=2)
    with pytest.raises(hip.HipLibraryError, match='alpha'):
        call(t, alpha=0.0)
    with pytest.raises(hip.HipLibraryError, match='maxstep'):
        call(t, maxstep=float('nan'))
    with pytest.raises(hip.HipLibraryError, match='tol2'):
        call(t, tol2=-1.0)
    # null mandatory pointers: straight at the C ABI (the Python wrapper would not let a None through)
    L = hip.lib()
    order = ('x', 'F', 'free', 'ptr', 'converged', 'n_steps', 'n_pairs', 'head', 'S', 'Y', 'rho', 'f_prev', 'work', 'pos_out', 'fmax')

    def raw(t, null=(), n_mol=1, n_atoms=n):
        p = {k: (None if k in null else hip._ptr(t[k])) for k in order}
        return L.nnhip_lbfgs_step(p['x'], p['F'], p['free'], p['ptr'], n_mol, n_atoms, m, d['tol2'], d['alpha'], d['maxstep'], 0,
                                  p['converged'], p['n_steps'], p['n_pairs'], p['head'], p['S'], p['Y'], p['rho'], p['f_prev'],
                                  p['work'], p['pos_out'], p['fmax'], hip._stream(t['x'].device))
    for name in order:
        if name in ('free', 'work'):
            continue                                                  # optional (work: only needed above 64 atoms)
        assert raw(t, null=(name,)) != 0, f'a null {name} was accepted'
    big = _slice(syn, int(np.argmax(np.diff(syn['ptr']) > 64)))
    assert big['x'].shape[0] > 64
    tb = {k: torch.from_numpy(np.ascontiguousarray(big[k])).cuda() for k in ('x', 'F', 'f_prev', 'S', 'Y', 'rho', 'ptr', 'free') + INTS}
    nb = big['x'].shape[0]
    tb.update(pos_out=torch.full((nb, 3), SENT, device='cuda'), fmax=torch.full((1,), SENT, device='cuda'), work=None)
    assert raw(dict(tb, work=torch.zeros(1, device='cuda')), null=('work',), n_atoms=nb) != 0, 'no scratch above 64 atoms was accepted'
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(t[k], v), f'{k} was written by a refused call'
    assert torch.all(tb['pos_out'] == SENT)
    # empty batches are no-ops that succeed
    assert raw(t, n_mol=0) == 0 and raw(t, null=order, n_mol=0, n_atoms=0) == 0
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(t[k], v), f'{k} was written by an empty launch'
    e3, e1 = torch.zeros(0, 3, device='cuda'), torch.zeros(0, device='cuda')
    ints = [torch.zeros(2, dtype=torch.int32, device='cuda') for _ in range(4)]
    fm = torch.full((2,), SENT, device='cuda')
    hip.lbfgs_step(e3, e3.clone(), None, torch.zeros(3, dtype=torch.int32, device='cuda'), m, d['tol2'], d['alpha'], d['maxstep'], 0,
                   *ints, torch.zeros(m, 0, 3, device='cuda'), torch.zeros(m, 0, 3, device='cuda'), torch.zeros(2, m, device='cuda'),
                   e3.clone(), None, e3.clone(), fm)                  # two molecules without atoms: converged from the start
    assert ints[0].tolist() == [1, 1] and ints[1].tolist() == [0, 0] and fm.tolist() == [0.0, 0.0]


# ---- 4. stepwise consistency of the driver ------------------------------------------------------------------------------------------

def _setup(case, weights):
    z, pos, cell, batch, _ = util.case_inputs(case, torch.float32)
    z, pos, cell, batch = cuda(z, pos, cell, batch)
    return make_model(util.load_state(weights)), z, pos, cell, batch


def check_stepwise(rel, frames_pos, frames_force, frames_pairs, free, label):
    """frames k and k + 1 are consecutive steps: one relax_ref.lbfgs_step per molecule from the state rebuilt out of the frames
    <= k (s from stored position differences, y from recorded force differences, rho = 1 / y.s with its bound carried along) must
    land on frame k + 1 within the bound.  A molecule-step with an ambiguous decision is skipped and counted; the state then
    follows what the recording shows the kernel decided.  Returns (molecule-steps, skipped, rejected pairs)."""
    ptr = _np(rel._mol_ptr)
    B, m = len(ptr) - 1, rel.memory
    states = [rr.new_state(int(ptr[b + 1] - ptr[b]), m) for b in range(B)]
    total = skipped = rejected = 0
    worst = 0.0
    for k in range(len(frames_pos) - 1):
        for b in range(B):
            sl = slice(int(ptr[b]), int(ptr[b + 1]))
            x, x1, F = frames_pos[k][sl], frames_pos[k + 1][sl], frames_force[k][sl]
            fr = None if free is None else free[sl]
            st = states[b]
            ref = rr.lbfgs_step(x, F, fr, st, rel._tol2, rel._alpha, rel._maxstep)
            total += 1
            amb = ref['ambiguous']
            p0, p1 = int(frames_pairs[k][b]), int(frames_pairs[k + 1][b])
            stayed = _same_bits(x1, x)
            if any(amb.values()):
                skipped += 1
                if not st['converged']:
                    # what the kernel decided, from the recording: a frozen molecule keeps its bits, an accepted pair raises n_pairs
                    # (or keeps a full ring full, where a rejection would have cost a pair)
                    accept = None if st['n_steps'] == 0 else p1 == min(p0 + 1, m)
                    ref = rr.lbfgs_step(x, F, fr, st, rel._tol2, rel._alpha, rel._maxstep, converge=stayed, accept=accept)
            else:
                what = f'{label}: step {k} -> {k + 1}, molecule {b}'
                assert ref['frozen'] == stayed or not np.any(rr.masked(F, fr)), f'{what}: frozen {ref["frozen"]}, bits kept {stayed}'
                assert ref['state']['n_pairs'] == p1, f'{what}: n_pairs {p1}, reference {ref["state"]["n_pairs"]}'
                rejected += ref['accepted'] is False
                err = np.abs(x1.astype(np.float64) - ref['x_out'])
                bx = ref['bx'] + rr.half_ulp32(ref['x_out'])
                assert np.all(err <= bx), f'{what}: positions err / bound {float((err / bx).max()):.3f}'
                if not ref['frozen']:
                    worst = max(worst, float((err / bx).max()))
            new = ref['state']
            if not ref['frozen']:
                new['S'][new['head']] = rr.stored_s(x1, x)            # the fp32 difference of the stored positions, as the kernel
            states[b] = new
    print(f'{label}: {total} molecule-steps, {skipped} skipped as ambiguous, {rejected} rejected pairs, worst err / bound {worst:.4f}')
    return total, skipped, rejected, states


@pytest.mark.parametrize('case,weights', [('mixed_rand', 'rand'), ('aspirin8_ckpt', 'ckpt')])
def test_every_recorded_step_follows_from_the_frames_before(case, weights):
    model, z, pos, cell, batch = _setup(case, weights)
    rel = model.relaxation(z, pos, cell, batch)
    p0, f0 = rel.positions, rel.forces.clone()
    before = model.deferred_stats()
    res = rel.run(40, check_every=0, record_every=1)
    after = model.deferred_stats()
    assert after['repeats_needed'] == before['repeats_needed']
    assert res.traj_step.tolist() == list(range(1, 41)) and res.traj_pos.shape == (40,) + tuple(pos.shape)
    assert res.traj_force.shape == res.traj_pos.shape and res.traj_energy.shape == res.traj_n_pairs.shape == (40, cell.shape[0])
    frames_pos = [p0] + list(res.traj_pos)
    frames_force = [f0] + list(res.traj_force)
    # the recorded forces are the model's at the recorded positions (a repeat from the wrong buffer would show here)
    worst = 0.0
    for p, f in zip(frames_pos, frames_force):
        worst = max(worst, float((model(z, p, cell, batch).gradient_force - f).abs().max()))
    print(f'{case}: recorded forces against model(recorded positions): max difference {worst:.3e} eV/A (allowed {util.FORCE_MAX_TOL})')
    assert worst <= util.FORCE_MAX_TOL
    pairs = [np.zeros(cell.shape[0], dtype=np.int64)] + [_np(t) for t in res.traj_n_pairs]
    total, skipped, rejected, states = check_stepwise(rel, [_np(t) for t in frames_pos], [_np(t) for t in frames_force], pairs, None,
                                                      case)
    assert skipped <= 0.01 * total, f'{skipped} of {total} molecule-steps are ambiguous'
    n_steps = _np(res.n_steps)
    assert [st['n_steps'] for st in states] == n_steps.tolist() and torch.equal(res.pos, res.traj_pos[-1])
    assert torch.equal(res.energy, res.traj_energy[-1])
    if case == 'mixed_rand':
        assert rejected >= 1, 'no pair was rejected: the reject branch was not exercised'
        assert (n_steps == 0).any(), 'no molecule was converged before its first step'
        assert bool(res.converged[torch.from_numpy(n_steps == 0).cuda()].all())


# ---- 5. convergence -----------------------------------------------------------------------------------------------------------------------

def test_aspirins_converge_like_the_host_fp64_loop():
    """aspirin8_ckpt, shipped weights, fmax = 0.01 eV/A, memory 16.  The yardstick is relax_ref.minimise (fp64 positions and
    arithmetic) driven by model() forces from the same start.  All 8 molecules must converge within 1.5 x the host loop's slowest
    molecule (without a line search the path is not monotone and fp32 rounding shifts step counts: on the CPU oracle the slowest
    molecule moved by up to 15 %), the recomputed fmax must be below 0.01 + util.FORCE_MAX_TOL, and every molecule's energy drop
    must be at least 90 % of the host loop's.  Measured on an MI355X when the test was written: device 129, 180, 93, 158, 89, 139,
    220, 172 steps, host 129, 185, 94, 158, 89, 140, 227, 172 (limit 340); recomputed fmax 0.0051 .. 0.0099 eV/A; energy drops 0.95 ..
    1.89 eV, equal to the host loop's in every printed digit."""
    model, z, pos, cell, batch = _setup('aspirin8_ckpt', 'ckpt')
    ptr = np.arange(9) * 21

    def energy_forces(x):
        out = model(z, torch.from_numpy(x).float().cuda(), cell, batch)
        return _np(out.energy).astype(np.float64), _np(out.gradient_force).astype(np.float64)
    host = rr.minimise(energy_forces, _np(pos).astype(np.float64), ptr, fmax=0.01, memory=16, max_steps=500)
    assert host['converged'].all(), f'the host loop did not converge: {host["n_steps"]}'
    limit = int(math.floor(1.5 * host['n_steps'].max()))
    rel = model.relaxation(z, pos, cell, batch, fmax=0.01, memory=16)
    e0 = _np(rel.potential_energy).astype(np.float64)
    res = rel.run(limit, check_every=10)
    n_steps = _np(res.n_steps)
    out = model(z, res.pos, cell, batch)
    fmax = _np(out.gradient_force.norm(dim=1).reshape(8, 21).max(dim=1).values)
    drop, host_drop = e0 - _np(res.energy).astype(np.float64), host['energy0'] - host['energy']
    print(f'steps per molecule: device {n_steps.tolist()}, host fp64 {host["n_steps"].tolist()} (limit {limit}); fmax recomputed '
          f'{fmax}; energy drop device {drop}, host {host_drop}')
    assert bool(res.converged.all()), f'not converged within {limit} steps: {n_steps.tolist()}, fmax {_np(res.fmax)}'
    assert n_steps.max() <= limit
    assert np.all(fmax < 0.01 + util.FORCE_MAX_TOL)
    assert np.all(_np(res.fmax) < 0.01) and torch.equal(res.energy, out.energy)
    assert np.all(host_drop > 0.5) and np.all(drop >= 0.9 * host_drop)


# ---- 6. bitwise properties ----------------------------------------------------------------------------------------------------------------

RESULT = ('pos', 'energy', 'fmax', 'converged', 'n_steps')


def test_bitwise_properties():
    model, z, pos, cell, batch = _setup('aspirin8_ckpt', 'ckpt')
    keep = [t.clone() for t in (z, pos, cell, batch)]
    fixed = torch.zeros(168, dtype=torch.bool, device='cuda')
    fixed[::5] = True

    def run(max_steps, check_every, record_every=0, **kw):
        return model.relaxation(z, pos, cell, batch, **kw).run(max_steps, check_every, record_every)
    # the same run twice; check_every = 0 (never reads, all 300 launches), 1 and 7 (stop early)
    a = run(300, 0, record_every=1)
    assert bool(a.converged.all()) and a.traj_step.tolist() == list(range(1, 301))
    for every in (0, 1, 7):
        b = run(300, every)
        for name in RESULT:
            assert torch.equal(getattr(a, name), getattr(b, name)), f'check_every = {every}: {name}'
    # after n_steps[b] every recorded frame of molecule b is constant, bit for bit
    n_steps = a.n_steps.tolist()
    assert max(n_steps) < 300 and min(n_steps) > 40
    for b, n in enumerate(n_steps):
        sl = slice(21 * b, 21 * (b + 1))
        assert torch.equal(a.traj_pos[n - 1:, sl], a.traj_pos[n - 1, sl].expand(301 - n, 21, 3)), f'molecule {b} moved after step {n}'
        assert not torch.equal(a.traj_pos[n - 2, sl], a.traj_pos[n - 1, sl])
        assert torch.equal(a.traj_energy[n - 1:, b], a.traj_energy[n - 1, b].expand(301 - n))
        assert torch.equal(a.traj_n_pairs[n - 1:, b], a.traj_n_pairs[n - 1, b].expand(301 - n))
    # run(a); run(b) leaves the bits of run(a + b); recording changes nothing
    rel = model.relaxation(z, pos, cell, batch)
    first = rel.run(23, 0)
    assert rel.step_count == 23 and first.n_steps.tolist() == [23] * 8
    second = rel.run(300 - 23, 10, record_every=50)
    assert second.traj_step[0].item() == 73
    for name in RESULT:
        assert torch.equal(getattr(a, name), getattr(second, name)), name
    assert torch.equal(first.pos, a.traj_pos[22]) and torch.equal(first.energy, a.traj_energy[22])
    assert torch.equal(rel.positions, a.pos)
    again = rel.run(5, 0)                                               # everything has converged: nothing changes any more
    for name in RESULT:
        assert torch.equal(getattr(a, name), getattr(again, name)), name
    # fixed atoms never move, the others do; the fixed forces do not count for convergence
    h = run(300, 10, record_every=1, fixed=fixed)
    assert torch.equal(h.traj_pos[:, fixed], pos[fixed].expand(h.traj_pos.shape[0], -1, -1)) and torch.equal(h.pos[fixed], pos[fixed])
    assert (h.pos[~fixed] != pos[~fixed]).any() and bool(h.converged.all())
    f = model(z, h.pos, cell, batch).gradient_force
    assert float(f[~fixed].norm(dim=1).max()) < 0.01 + util.FORCE_MAX_TOL and float(f[fixed].norm(dim=1).max()) > 0.05
    # the caller's tensors are never modified
    for t, k in zip((z, pos, cell, batch), keep):
        assert torch.equal(t, k)
    assert not pos.requires_grad


# ---- 7. interfaces ------------------------------------------------------------------------------------------------------------------------

def test_calculator_relax_equals_the_model_path():
    from newtonnet_amd.relax import Relaxation, RelaxResult
    from newtonnet_amd.utils import MLAseCalculator
    from tests.test_hip_md import FakeAtoms
    model, z, pos, cell, batch = _setup('aspirin8_ckpt', 'ckpt')
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda')
    zc, pc = _np(z), _np(pos)
    frames = [FakeAtoms(zc[21 * k:21 * (k + 1)], pc[21 * k:21 * (k + 1)]) for k in range(3)]
    keep = [f.positions.copy() for f in frames]
    fixed = np.zeros(21, dtype=bool)
    fixed[3] = True
    out = calc.relax(frames, fmax=0.05, max_steps=60, fixed=fixed)
    assert all(np.array_equal(f.positions, k) for f, k in zip(frames, keep))
    assert out['positions'].shape == (3, 21, 3) and out['positions'].dtype == np.float32
    for k, dt in (('energy', np.float32), ('fmax', np.float32), ('converged', np.bool_), ('n_steps', np.int64)):
        assert out[k].shape == (3,) and out[k].dtype == dt, k
    rel = model.relaxation(z[:63], pos[:63], cell[:3], batch[:63], fmax=0.05, fixed=torch.from_numpy(np.tile(fixed, 3)).cuda())
    res = rel.run(60, check_every=10)
    assert isinstance(rel, Relaxation) and isinstance(res, RelaxResult) and res.traj_pos is None
    assert np.array_equal(out['positions'].reshape(63, 3), _np(res.pos)) and np.array_equal(out['energy'], _np(res.energy))
    assert np.array_equal(out['fmax'], _np(res.fmax)) and np.array_equal(out['converged'], _np(res.converged))
    assert np.array_equal(out['n_steps'], _np(res.n_steps)) and np.array_equal(out['positions'][:, 3], pc[:63].reshape(3, 21, 3)[:, 3])
    one = calc.relax(frames[0], fmax=0.05, max_steps=7)                 # a single frame drops the frame axis
    assert one['positions'].shape == (21, 3) and one['energy'].shape == () and one['n_steps'] == 7 and not one['converged']
    for bad in (dict(max_steps=-1), dict(max_steps=3, check_every=-1), dict(max_steps=3, record_every=2.5)):
        with pytest.raises(ValueError):
            rel.run(**bad)
    assert rel.run(0).n_steps.tolist() == res.n_steps.tolist()
