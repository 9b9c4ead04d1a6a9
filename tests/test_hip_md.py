"""Batched molecular dynamics on the HIP path (newtonnet_amd/dynamics.py, csrc/md.hip).

Kernel alone: nnhip_md_step on random inputs against its fp64 restatement on the SAME fp32 inputs (tests/md_ref.py), every output
within the derived first-order rounding bound (C_MD = 2) plus half an fp32 ulp of the stored value; the tests print err / bound.
Driver: every recorded step is checked ONE step at a time -- forces recomputed on the recorded positions, noise regenerated from
the seed -- so no error compounds and no chaos term has to be guessed; velocities get hk_i x util.FORCE_MAX_TOL on top, in case a
recomputed force took another path through the library.  Energy conservation is measured against a host fp64 integrator plus the
first-order cost of keeping the state in fp32."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import md_ref as mr
from tests import util
from tests.test_hip_hessian import cuda, make_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. the kernels against fp64 on the same inputs ---------------------------------------------------------------------------

def _random_inputs(N, seed):
    rng = np.random.default_rng(seed)
    f32 = np.float32
    x, v, F = (rng.uniform(-8, 8, (N, 3)).astype(f32), rng.uniform(-0.2, 0.2, (N, 3)).astype(f32), rng.uniform(-5, 5, (N, 3)).astype(f32))
    m = rng.choice(np.array([1.008, 12.011, 14.007, 15.999], dtype=f32), N)
    dt = 0.5 * 0.0982269
    hk, sigma = (0.5 * dt / m.astype(np.float64)).astype(f32), np.sqrt(0.02 * 8.617333262e-5 * 300.0 / m.astype(np.float64)).astype(f32)
    xi = rng.standard_normal((N, 3)).astype(f32)
    fixed = rng.random(N) < 0.25
    hk[fixed], sigma[fixed], v[fixed] = 0, 0, 0
    return dict(x=x, v=v, F=F, m=m, hk=hk, sigma=sigma, xi=xi, fixed=fixed, dth=float(f32(0.5 * dt)), c1=float(f32(np.exp(-0.01))))


@pytest.mark.parametrize('with_noise', [False, True])
@pytest.mark.parametrize('flags', [mr.BEGIN, mr.FINISH, mr.BEGIN | mr.FINISH])
@pytest.mark.parametrize('N', [1, 9, 63, 64, 65, 257, 1000])
def test_md_step_against_fp64_on_the_same_inputs(N, flags, with_noise):
    from newtonnet_amd import hip
    d = _random_inputs(N, 100 + N)
    t = {k: torch.from_numpy(d[k]).cuda() for k in ('x', 'v', 'F', 'm', 'hk', 'sigma', 'xi')}
    SENT = 777.0
    pos_out = torch.full((N, 3), SENT, device='cuda')
    ke = torch.full((N,), SENT, device='cuda')
    vel = t['v'].clone()
    hip.md_step(t['x'] if flags & mr.BEGIN else None, vel, t['F'], t['hk'], d['dth'], d['c1'], flags,
                pos_out=pos_out if flags & mr.BEGIN else None, mass=t['m'], sigma=t['sigma'] if with_noise else None,
                noise=t['xi'] if with_noise else None, ke_out=ke if flags & mr.FINISH else None)
    ref = mr.md_step(flags, d['x'], d['v'], d['F'], d['hk'], d['m'], d['sigma'] if with_noise else None,
                     d['xi'] if with_noise else None, d['c1'], d['dth'])
    assert torch.equal(t['x'], torch.from_numpy(d['x']).cuda()) and torch.equal(t['F'], torch.from_numpy(d['F']).cuda())   # inputs intact
    worst = {}
    e_v = np.abs(_np(vel).astype(np.float64) - ref['v'])
    worst['v'] = float((e_v / (ref['bv'] + mr.half_ulp32(ref['v']))).max())
    assert np.all(e_v <= ref['bv'] + mr.half_ulp32(ref['v']))
    if flags & mr.BEGIN:
        e_x = np.abs(_np(pos_out).astype(np.float64) - ref['x'])
        worst['x'] = float((e_x / (ref['bx'] + mr.half_ulp32(ref['x']))).max())
        assert np.all(e_x <= ref['bx'] + mr.half_ulp32(ref['x']))
        assert np.array_equal(_np(pos_out)[d['fixed']], d['x'][d['fixed']])          # fixed atoms: bitwise where they were
        assert not np.any(_np(vel)[d['fixed']])
    else:
        assert torch.all(pos_out == SENT)
    if flags & mr.FINISH:
        e_k = np.abs(_np(ke).astype(np.float64) - ref['ke'])
        worst['ke'] = float((e_k / (ref['bke'] + mr.half_ulp32(ref['ke']))).max())
        assert np.all(e_k <= ref['bke'] + mr.half_ulp32(ref['ke']))
    else:
        assert torch.all(ke == SENT)
    print(f'md_step N = {N}, flags = {flags}, noise {with_noise}: worst err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items())
          + f' (C_MD = {mr.C_MD})')


@pytest.mark.parametrize('sizes', [(1, 9, 21, 300), (5000,), (0, 3, 0)])
def test_md_kinetic_is_within_the_sum_bound_and_bitwise_repeatable(sizes):
    from newtonnet_amd import hip
    rng = np.random.default_rng(sum(sizes))
    N = sum(sizes)
    ke = (rng.random(N) * 0.3).astype(np.float32)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    ke_d, ptr_d = torch.from_numpy(ke).cuda(), torch.from_numpy(ptr).cuda()
    a, b = hip.md_kinetic(ke_d, ptr_d), hip.md_kinetic(ke_d, ptr_d)
    assert a.shape == (len(sizes),) and torch.equal(a, b)
    for k, n in enumerate(sizes):
        seg = ke[ptr[k]:ptr[k + 1]].astype(np.float64)
        err, bound = abs(float(a[k]) - seg.sum()), mr.kinetic_sum_bound(seg) + mr.half_ulp32(seg.sum())
        print(f'md_kinetic molecule of {n} atoms: err / bound {err / bound if bound else 0.0:.4f}')
        assert err <= bound
        if n <= 1:
            assert float(a[k]) == (float(seg[0]) if n else 0.0)


# ---- 2. aliasing and bad arguments --------------------------------------------------------------------------------------------

def test_md_step_refuses_aliased_positions_and_half_given_noise():
    from newtonnet_amd import hip
    d = _random_inputs(65, 5)
    t = {k: torch.from_numpy(d[k]).cuda() for k in ('x', 'v', 'F', 'm', 'hk', 'sigma', 'xi')}
    x0, v0 = t['x'].clone(), t['v'].clone()
    out = torch.full((65, 3), 777.0, device='cuda')
    with pytest.raises(hip.HipLibraryError, match='alias'):
        hip.md_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 1.0, mr.BEGIN, pos_out=t['x'])
    with pytest.raises(hip.HipLibraryError, match='alias'):          # an overlapping view is an alias too
        flat = torch.zeros(3 * 65 + 3, device='cuda')
        hip.md_step(flat[:195].view(65, 3), t['v'], t['F'], t['hk'], d['dth'], 1.0, mr.BEGIN, pos_out=flat[3:].view(65, 3))
    with pytest.raises(hip.HipLibraryError, match='sigma and noise'):
        hip.md_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 0.99, mr.BEGIN, pos_out=out, sigma=t['sigma'])
    with pytest.raises(hip.HipLibraryError, match='sigma and noise'):
        hip.md_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 0.99, mr.BEGIN, pos_out=out, noise=t['xi'])
    with pytest.raises(hip.HipLibraryError, match='flags'):
        hip.md_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 1.0, 0, pos_out=out)
    with pytest.raises(hip.HipLibraryError):                         # begin without an output
        hip.md_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 1.0, mr.BEGIN)
    torch.cuda.synchronize()
    assert torch.equal(t['x'], x0) and torch.equal(t['v'], v0) and torch.all(out == 777.0)      # nothing was written
    empty = torch.zeros(0, 3, device='cuda')
    hip.md_step(empty, empty.clone(), empty, torch.zeros(0, device='cuda'), d['dth'], 1.0, mr.BEGIN, pos_out=empty.clone())   # no-op


# ---- 3. stepwise consistency of the driver ------------------------------------------------------------------------------------

def _forces(model, z, pos, cell, batch):
    out = model(z, pos, cell, batch)
    return out.gradient_force.clone(), out.energy.clone()


def check_stepwise(model, dyn, z, cell, batch, frames_pos, frames_vel, noises, label):
    """frames k and k + 1 are consecutive full steps: one md_ref.full_step from frame k, with the forces the model returns on the
    two recorded geometries and the noise of that step, must land on frame k + 1 within the bound"""
    hk, m = _np(dyn._hk), _np(dyn.masses)
    sigma = None if dyn._sigma is None else _np(dyn._sigma)
    F = [_np(_forces(model, z, p, cell, batch)[0]) for p in frames_pos]
    worst_x = worst_v = 0.0
    for k in range(len(frames_pos) - 1):
        xi = None if sigma is None else _np(noises[k])
        ref = mr.full_step(_np(frames_pos[k]), _np(frames_vel[k]), F[k], F[k + 1], hk, m, sigma, xi, dyn._c1, dyn._dth)
        bx = ref['bx'] + mr.half_ulp32(ref['x'])
        bv = ref['bv'] + mr.half_ulp32(ref['v']) + hk.astype(np.float64)[:, None] * util.FORCE_MAX_TOL
        e_x = np.abs(_np(frames_pos[k + 1]).astype(np.float64) - ref['x'])
        e_v = np.abs(_np(frames_vel[k + 1]).astype(np.float64) - ref['v'])
        worst_x, worst_v = max(worst_x, float((e_x / bx).max())), max(worst_v, float((e_v / bv).max()))
        assert np.all(e_x <= bx), f'{label}: step {k} -> {k + 1}: positions err / bound {float((e_x / bx).max()):.3f}'
        assert np.all(e_v <= bv), f'{label}: step {k} -> {k + 1}: velocities err / bound {float((e_v / bv).max()):.3f}'
    print(f'{label}: {len(frames_pos) - 1} steps, worst err / bound positions {worst_x:.4f}, velocities {worst_v:.4f}')


def run_and_check(model, z, pos, cell, batch, n_steps, label, seed=7, **kw):
    """Dynamics.run(n_steps, record_every=1) from a seeded generator, then check_stepwise over (initial state, every step)"""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    dyn = model.dynamics(z, pos, cell, batch, generator=gen, **kw)
    p0, v0 = dyn.positions, dyn.velocities
    before = model.deferred_stats()
    traj = dyn.run(n_steps, record_every=1)
    after = model.deferred_stats()
    assert traj.step.tolist() == list(range(1, n_steps + 1)) and traj.pos.shape == (n_steps,) + tuple(pos.shape)
    # the noise of the run, regenerated: the generator's draws are the Maxwell-Boltzmann one (if any), then one per step
    regen = torch.Generator(device='cuda').manual_seed(seed)
    if kw.get('velocities') is None and kw.get('temperature') is not None:
        torch.randn(tuple(pos.shape), generator=regen, device='cuda')
    noises = [torch.randn(tuple(pos.shape), generator=regen, device='cuda') for _ in range(n_steps)] if dyn._sigma is not None else None
    check_stepwise(model, dyn, z, cell, batch, [p0] + list(traj.pos), [v0] + list(traj.vel), noises, label)
    return dyn, traj, before, after


@pytest.mark.parametrize('thermostat', ['nve', 'langevin'])
@pytest.mark.parametrize('case', ['mixed_rand', 'aspirin8_rand'])
def test_every_recorded_step_follows_from_the_one_before(case, thermostat):
    z, pos, cell, batch, _ = util.case_inputs(case, torch.float32)
    z, pos, cell, batch = cuda(z, pos, cell, batch)
    model = make_model(util.load_state('rand'))
    if thermostat == 'nve':
        kw = dict(temperature=300.0)
    else:
        kw = dict(temperature=torch.linspace(200.0, 400.0, cell.shape[0]).cuda(), friction=0.02)
    dyn, traj, before, after = run_and_check(model, z, pos, cell, batch, 40, f'{case} {thermostat}', **kw)
    assert (dyn._sigma is None) == (thermostat == 'nve')
    assert after['repeats_needed'] == before['repeats_needed']
    assert after['deferred_calls'] - before['deferred_calls'] >= 40 - 2
    # (a molecule of one atom has no kinetic energy once its centre-of-mass momentum is gone: >= 0, and > 0 for the others)
    assert float(traj.kinetic_energy.min()) >= 0 and torch.isfinite(traj.total_energy).all()
    assert bool((traj.kinetic_energy[:, _np(dyn._counts) > 1] > 0).all())
    np.testing.assert_allclose(_np(traj.temperature), 2.0 * _np(traj.kinetic_energy) / (3.0 * 8.617333262e-5 * _np(dyn._counts)[None, :]),
                               rtol=1e-6)


# ---- 4. the repeat path ---------------------------------------------------------------------------------------------------------

def _closing_halves(n_mol=8, seed=0):
    """n_mol molecules of 24 atoms: two 12-atom clusters, each a 3 x 4 sheet of 1.0 A spacing with N(0, 0.02^2) jitter (minimum
    distance above 0.9 A), face to face, the second shifted along x until the nearest atoms of the two are 5.3 A apart -- outside
    the 5 A cutoff: no edge between the halves.  Sheets, because a capacity only overflows when the edge count JUMPS: the model
    re-centres its capacity (count + 1/16 + 256) as soon as a count comes within 1/32 of it, so a count that creeps up never
    repeats a step.  Face to face, whole shells of pairs (directly opposite, one spacing aside, ...) cross the cutoff within a
    step or two: moved rigidly, the 2112 directed edges stay until step 6 and are 2606 at step 9, above the capacity 2500 taken
    at the start, and 4316 at step 30"""
    rng = np.random.default_rng(seed)
    sheet = np.stack(np.meshgrid([0.0], np.arange(3) * 1.0, np.arange(4) * 1.0, indexing='ij'), -1).reshape(-1, 3)
    pos, side = [], []
    for _ in range(n_mol):
        a, b = sheet + rng.normal(0, 0.02, sheet.shape), sheet + rng.normal(0, 0.02, sheet.shape)
        for half in (a, b):
            assert (np.linalg.norm(half[:, None, :] - half[None, :, :], axis=-1) + 9.0 * np.eye(12)).min() >= 0.9
        lo, hi = 0.0, 20.0
        for _ in range(60):                       # bisection on the shift: the nearest distance grows with it
            mid = 0.5 * (lo + hi)
            near = np.linalg.norm(a[:, None, :] - (b + [mid, 0, 0])[None, :, :], axis=-1).min()
            lo, hi = (mid, hi) if near < 5.3 else (lo, mid)
        b = b + [hi, 0, 0]
        assert abs(np.linalg.norm(a[:, None, :] - b[None, :, :], axis=-1).min() - 5.3) < 1e-6
        pos += [a, b]
        side += [np.full(12, 1.0), np.full(12, -1.0)]
    pos, side = np.concatenate(pos).astype(np.float32), np.concatenate(side)
    z = np.tile(np.array([6, 6, 6, 8, 8, 7, 1, 1, 1, 1, 6, 8]), 2 * n_mol)
    batch = np.repeat(np.arange(n_mol), 24)
    return z, pos, batch, side


def test_a_step_that_outgrows_its_edge_capacity_is_repeated_from_the_right_positions():
    from newtonnet_amd import dynamics as dyn_mod
    z, pos, batch, side = _closing_halves()
    z, pos, batch = torch.from_numpy(z).long().cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(batch).long().cuda()
    cell = torch.zeros(8, 3, 3, device='cuda')
    model = make_model(util.load_state('rand'))
    # each half moves 0.025 A per 0.5 fs step towards the other: the gap closes by 0.05 A per step; 12 amu everywhere keeps the
    # model's forces from changing that within 30 steps
    vel = torch.zeros(192, 3)
    vel[:, 0] = torch.from_numpy(side * 0.025 / (0.5 * dyn_mod.FS)).float()
    masses = torch.full((192,), 12.0, device='cuda')
    n_first = model(z, pos, cell, batch).n_edges
    dyn, traj, before, after = run_and_check(model, z, pos, cell, batch, 30, 'closing halves', velocities=vel.cuda(), masses=masses)
    n_last = model(z, traj.pos[-1], cell, batch).n_edges
    print(f'closing halves: {n_first} edges at the start, {n_last} after 30 steps; repeats needed {before["repeats_needed"]} -> '
          f'{after["repeats_needed"]}')
    assert n_last > n_first + n_first // 16 + 256, 'the set-up does not outgrow the capacity'
    assert after['repeats_needed'] > before['repeats_needed'], 'no deferred step had to be repeated'


# ---- 5. bitwise properties --------------------------------------------------------------------------------------------------------

def test_bitwise_properties():
    z, pos, cell, batch, _ = util.case_inputs('mixed_rand', torch.float32)
    z, pos, cell, batch = cuda(z, pos, cell, batch)
    keep = [t.clone() for t in (z, pos, cell, batch)]
    model = make_model(util.load_state('rand'))
    ladder = torch.linspace(200.0, 400.0, cell.shape[0]).cuda()

    def langevin(seed, n, every):
        gen = torch.Generator(device='cuda').manual_seed(seed)
        return model.dynamics(z, pos, cell, batch, temperature=ladder, friction=0.02, generator=gen).run(n, every)
    a, b, c = langevin(7, 20, 1), langevin(7, 20, 1), langevin(8, 20, 1)
    for name in ('pos', 'vel', 'potential_energy', 'kinetic_energy', 'step'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name                       # the same seed twice
    assert not torch.equal(a.pos, c.pos)
    e5 = langevin(7, 20, 5)
    assert e5.step.tolist() == [5, 10, 15, 20]
    for name in ('pos', 'vel', 'potential_energy', 'kinetic_energy'):
        assert torch.equal(getattr(e5, name), getattr(a, name)[4::5]), name                 # record_every = 1 and 5 at the common steps
    assert langevin(7, 7, 3).step.tolist() == [3, 6, 7] and langevin(7, 7, 0).step.tolist() == [7]
    # friction = 0 with a temperature equals the microcanonical run (same initial velocities; the temperature then only seeds them)
    gen = torch.Generator(device='cuda').manual_seed(3)
    d1 = model.dynamics(z, pos, cell, batch, temperature=300.0, friction=0.0, generator=gen)
    v0 = d1.velocities
    state = gen.get_state()
    t1 = d1.run(20, 1)
    assert torch.equal(gen.get_state(), state)                                             # no noise was drawn
    d2 = model.dynamics(z, pos, cell, batch, velocities=v0)
    t2 = d2.run(40, 1)
    for name in ('pos', 'vel', 'potential_energy', 'kinetic_energy'):
        assert torch.equal(getattr(t1, name), getattr(t2, name)[:20]), name
    # run(20); run(20) equals run(40)
    t1b = d1.run(20, 0)
    assert t1b.step.tolist() == [40] and d1.step_count == 40
    assert torch.equal(t1b.pos[0], t2.pos[-1]) and torch.equal(t1b.vel[0], t2.vel[-1])
    assert torch.equal(t1b.potential_energy[0], t2.potential_energy[-1]) and torch.equal(t1b.kinetic_energy[0], t2.kinetic_energy[-1])
    assert torch.equal(d1.positions, d2.positions) and torch.equal(d1.velocities, d2.velocities)
    assert torch.equal(d1.potential_energy, d2.potential_energy) and torch.equal(d1.kinetic_energy, d2.kinetic_energy)
    assert torch.equal(d1.forces, d2.forces)
    # the same for Langevin, where the noise stream has to continue across the calls
    gen = torch.Generator(device='cuda').manual_seed(7)
    d3 = model.dynamics(z, pos, cell, batch, temperature=ladder, friction=0.02, generator=gen)
    d3.run(11, 4)
    t3 = d3.run(9, 0)
    assert torch.equal(t3.pos[0], a.pos[-1]) and torch.equal(t3.vel[0], a.vel[-1]) and torch.equal(t3.kinetic_energy[0], a.kinetic_energy[-1])
    # the caller's tensors are never modified
    for t, k in zip((z, pos, cell, batch), keep):
        assert torch.equal(t, k)
    assert not pos.requires_grad


# ---- 6. energy conservation -------------------------------------------------------------------------------------------------------

def test_energy_conservation_against_a_host_fp64_integrator():
    """4 aspirins, seeded weights, table masses, Maxwell-Boltzmann at 300 K, 0.5 fs, 400 steps microcanonical.  Per molecule,
    max_n |E_tot(n) - E_tot(0)| <= (a) the same figure of a host fp64 velocity-Verlet loop driven by model() forces from the same
    start + (b) the first-order cost of the fp32 state, sum over steps of [sum_i |F_i| ulp(x_i) / 2 + sum_i m_i v_i^2 2^-24] +
    (c) 2 util.energy_tol(E); and the kinetic energy must move by at least 10 x that bound, or the test would show nothing."""
    from newtonnet_amd import dynamics as dyn_mod
    n_steps = 400
    z, pos, cell, batch = _bench().synthetic_aspirin(4, 0, 'cuda')
    model = make_model(util.load_state('rand'))
    gen = torch.Generator(device='cuda').manual_seed(11)
    dyn = model.dynamics(z, pos, cell, batch, temperature=300.0, timestep=0.5, generator=gen)
    p0, v0 = dyn.positions, dyn.velocities
    e0, k0 = dyn.potential_energy.clone(), dyn.kinetic_energy
    traj = dyn.run(n_steps, record_every=1)
    B, n = 4, 21
    m = _np(dyn.masses).astype(np.float64)
    pe = np.concatenate([_np(e0)[None], _np(traj.potential_energy)]).astype(np.float64)
    ke = np.concatenate([_np(k0)[None], _np(traj.kinetic_energy)]).astype(np.float64)
    tot = pe + ke
    drift = np.abs(tot - tot[0]).max(axis=0)
    # (a) host fp64 velocity Verlet on the same model, the procedure of test_md_loop_conserves_total_energy with real masses
    dt = 0.5 * dyn_mod.FS
    x, v = _np(p0).astype(np.float64), _np(v0).astype(np.float64)

    def evaluate(xx):
        f, e = _forces(model, z, torch.from_numpy(xx).float().cuda(), cell, batch)
        return _np(f).astype(np.float64), _np(e).astype(np.float64)
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
    # (b) from the recorded trajectory
    b = np.zeros(B)
    for k in range(n_steps):
        F = _np(_forces(model, z, traj.pos[k], cell, batch)[0]).astype(np.float64)
        xk, vk = _np(traj.pos[k]), _np(traj.vel[k]).astype(np.float64)
        per_atom = (np.abs(F) * mr.half_ulp32(xk)).sum(1) + m * (vk * vk).sum(1) * mr.EPS32
        b += per_atom.reshape(B, n).sum(1)
    c = 2.0 * util.energy_tol(pe[0])
    bound = a + b + c
    swing = ke.max(axis=0) - ke.min(axis=0)
    print(f'energy conservation over {n_steps} steps: drift {drift} eV, bound {bound} = host fp64 {a} + fp32 state {b} + energy ulps {c}; '
          f'drift / bound {drift / bound}; kinetic energy swing {swing} eV = {swing / bound} x bound; E_pot(0) {pe[0]}')
    assert np.all(drift <= bound), f'drift / bound {drift / bound}'
    assert np.all(swing >= 10.0 * bound), f'kinetic energy swing / bound {swing / bound}: the test has no power'


# ---- 7. periodic molecules --------------------------------------------------------------------------------------------------------

def test_periodic_images_give_the_same_forces_and_a_periodic_run_is_stepwise_consistent():
    z, pos, cell, batch, _ = util.case_inputs('pbc_batch2_rand', torch.float32)
    z, pos, cell, batch = cuda(z, pos, cell, batch)
    model = make_model(util.load_state('rand'))
    f0, e0 = _forces(model, z, pos, cell, batch)
    gen = torch.Generator().manual_seed(2)
    k = torch.randint(-2, 3, (pos.shape[0], 3), generator=gen).float().cuda()
    shifted = (pos.double() + torch.einsum('nk,nkd->nd', k.double(), cell[batch].double())).float()
    f1, e1 = _forces(model, z, shifted, cell, batch)
    df, de = float((f1 - f0).abs().max()), _np((e1 - e0).abs())
    print(f'periodic images (|k| <= 2): max |dF| {df:.3e} eV/A (allowed {util.FORCE_MAX_TOL}), |dE| {de} (allowed {util.energy_tol(_np(e0))})')
    assert df <= util.FORCE_MAX_TOL and np.all(de <= util.energy_tol(_np(e0)))
    run_and_check(model, z, pos, cell, batch, 20, 'pbc_batch2 nve', temperature=300.0)


# ---- 8. interfaces ----------------------------------------------------------------------------------------------------------------

class FakeAtoms:
    """The accessors format_data() and run_md() use (as in tests/test_ase_calculator.py), plus optional masses and momenta"""
    def __init__(self, numbers, positions, masses=None, momenta=None):
        self.numbers, self.positions = np.asarray(numbers), np.asarray(positions, dtype=np.float64)
        if masses is not None:
            self.get_masses = lambda: np.asarray(masses, dtype=np.float64)
        if momenta is not None:
            self.get_momenta = lambda: np.asarray(momenta, dtype=np.float64)

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


def test_interfaces_shapes_seed_and_rest():
    from newtonnet_amd.dynamics import Dynamics, Trajectory
    from newtonnet_amd.utils import MLAseCalculator
    z, pos, _, _ = _bench().synthetic_aspirin(3, 1, 'cpu')
    model = make_model(util.load_state('rand'))
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda')
    frames = [FakeAtoms(z[:21].numpy(), pos[21 * k:21 * (k + 1)].numpy()) for k in range(3)]
    keep = [f.positions.copy() for f in frames]
    out = calc.run_md(frames, 6, temperature=300.0, friction=0.01, record_every=4, seed=5)
    assert out['step'].tolist() == [4, 6] and out['step'].dtype == np.int64
    assert out['positions'].shape == out['velocities'].shape == (2, 3, 21, 3) and out['positions'].dtype == np.float32
    assert out['energy'].shape == out['kinetic_energy'].shape == (2, 3) and out['energy'].dtype == np.float32
    again = calc.run_md(frames, 6, temperature=300.0, friction=0.01, record_every=4, seed=5)
    other = calc.run_md(frames, 6, temperature=300.0, friction=0.01, record_every=4, seed=6)
    assert all(np.array_equal(out[k], again[k]) for k in out) and not np.array_equal(out['positions'], other['positions'])
    assert all(np.array_equal(f.positions, k) for f, k in zip(frames, keep))
    one = calc.run_md(frames[0], 3)                                    # a single frame squeezes; no temperature: from rest
    assert one['positions'].shape == (1, 21, 3) and one['energy'].shape == (1,) and one['kinetic_energy'].shape == (1,)
    # masses and momenta of the object are used: p = m v in the internal units
    masses = np.full(21, 12.0)
    mom = np.zeros((21, 3))
    mom[:, 0] = 12.0 * 0.01
    moving = calc.run_md(FakeAtoms(z[:21].numpy(), pos[:21].numpy(), masses=masses, momenta=mom), 0)
    assert moving['step'].tolist() == [0] and np.allclose(moving['velocities'][0, :, 0], 0.01, rtol=1e-6)
    assert abs(float(moving['kinetic_energy'][0]) - 0.5 * 12.0 * 21 * 1e-4) <= 1e-6 * 0.0126
    # model.dynamics: a Dynamics whose run returns device tensors of the stated shapes and dtypes
    zc, pc = z.cuda(), pos.cuda()
    cell, batch = torch.zeros(3, 3, 3, device='cuda'), torch.repeat_interleave(torch.arange(3), 21).cuda()
    dyn = model.dynamics(zc, pc, cell, batch, temperature=100.0)
    traj = dyn.run(5, record_every=2)
    assert isinstance(dyn, Dynamics) and isinstance(traj, Trajectory) and traj.step.tolist() == [2, 4, 5]
    for bad in (dict(n_steps=-1), dict(n_steps=2.5), dict(n_steps=3, record_every=-1)):
        with pytest.raises(ValueError):
            dyn.run(**bad)
    assert dyn.step_count == 5 and dyn.run(0).step.tolist() == [5]
    assert traj.pos.shape == traj.vel.shape == (3, 63, 3) and traj.pos.is_cuda and traj.pos.dtype == torch.float32
    for name in ('potential_energy', 'kinetic_energy', 'total_energy', 'temperature'):
        assert getattr(traj, name).shape == (3, 3) and getattr(traj, name).dtype == torch.float32
    assert dyn.positions.shape == dyn.velocities.shape == dyn.forces.shape == (63, 3) and dyn.kinetic_energy.shape == (3,)
    assert torch.equal(dyn.positions, traj.pos[-1]) and torch.equal(dyn.potential_energy, traj.potential_energy[-1])
    # zero-temperature Langevin from rest where no atom feels a force (every atom alone inside the cutoff): nothing moves
    lone = torch.tensor([[0.0, 0.0, 0.0], [7.0, 0.0, 0.0], [0.0, 9.0, 0.0]], device='cuda')
    zl, bl = torch.tensor([6, 8, 1], device='cuda'), torch.zeros(3, dtype=torch.long, device='cuda')
    rest = model.dynamics(zl, lone, torch.zeros(1, 3, 3, device='cuda'), bl, temperature=0.0, friction=0.02)
    assert not rest.forces.any()
    tr = rest.run(10, 1)
    assert torch.equal(tr.pos, lone[None].expand(10, 3, 3)) and not tr.vel.any() and not tr.kinetic_energy.any()
    # fixed atoms stay where they are, bit for bit, while the others move
    fixed = torch.zeros(63, dtype=torch.bool, device='cuda')
    fixed[::2] = True
    held = model.dynamics(zc, pc, cell, batch, temperature=300.0, friction=0.02, fixed=fixed)
    th = held.run(8, 0)
    assert torch.equal(th.pos[0][fixed], pc[fixed]) and not th.vel[0][fixed].any() and (th.pos[0][~fixed] != pc[~fixed]).any()
