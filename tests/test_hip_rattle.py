"""Bond-length constraints on the HIP path (csrc/rattle.hip, newtonnet_amd/dynamics.py, newtonnet_amd/constraints.py).

Kernel alone: nnhip_md_step_constrained on the batches of tests/rattle_ref.py (`case`) -- the constraints as stored within the
derived bound, every output against the fp64 restatement converged to 1e-13 on the SAME fp32 inputs within the bound rattle_ref
states, and the bitwise properties (repeats, a molecule alone and inside a batch, an unconstrained molecule against nnhip_md_step,
fixed atoms, a batch shifted by 100 A).  Failure path: max_iter = 1 and the breakdown guard mark failure and store finite values.
Driver: every recorded step of constrained runs at 2 fs is checked ONE step at a time, as tests/test_hip_md.py does.
Every test prints its worst err / bound."""
import numpy as np
import pytest
import torch

from tests import rattle_ref as rr
from tests import util
from tests.test_hip_hessian import cuda, make_model

pytestmark = pytest.mark.gpu

SENT = 777.0
FLAGS = [(rr.FINISH, False), (rr.BEGIN, False), (rr.BEGIN, True), (rr.FINISH | rr.BEGIN, False), (rr.FINISH | rr.BEGIN, True),
         (rr.PROJECT, False)]


def _np(t):
    return t.detach().cpu().numpy()


def _tables(d):
    from newtonnet_amd import constraints as con
    return con.device_tables(d['prep'], d['d2'], torch.from_numpy(d['mol_ptr']).cuda())


def call(d, flags, noise, tol=rr.TOL, max_iter=rr.MAX_ITER, tables=None, n_failed=None):
    """one launch on the inputs of a case; returns dict(x, v, ke: tensors (sentinels where the launch writes nothing), n_failed,
    n_sweeps, t: the input tensors)"""
    from newtonnet_amd import hip
    t = {k: torch.from_numpy(d[k]).cuda() for k in ('x', 'v', 'F', 'm', 'hk', 'w', 'sigma', 'xi')}
    N, B = d['x'].shape[0], len(d['sizes'])
    pos_out, ke = torch.full((N, 3), SENT, device='cuda'), torch.full((N,), SENT, device='cuda')
    vel = t['v'].clone()
    n_failed = torch.zeros(B, dtype=torch.int32, device='cuda') if n_failed is None else n_failed
    n_sweeps = torch.full((B,), -1, dtype=torch.int32, device='cuda')
    moves = bool(flags & (rr.BEGIN | rr.PROJECT))
    hip.md_step_constrained(t['x'], vel, None if flags == rr.PROJECT else t['F'], t['hk'], t['w'], d['dth'], d['inv_dth'], d['c1'],
                            flags, _tables(d) if tables is None else tables, tol, max_iter, n_failed, n_sweeps,
                            pos_out=pos_out if moves else None, mass=t['m'], sigma=t['sigma'] if noise else None,
                            noise=t['xi'] if noise else None, ke_out=ke if flags & rr.FINISH else None)
    return dict(x=pos_out, v=vel, ke=ke, n_failed=n_failed, n_sweeps=n_sweeps, t=t)


def sub_case(d, b):
    """molecule b of a case as a batch of its own"""
    from newtonnet_amd import constraints as con
    a0, a1 = int(d['mol_ptr'][b]), int(d['mol_ptr'][b + 1])
    T = d['T']
    mine = T.mol == b
    pairs = np.stack([T.gi[mine] - a0, T.gj[mine] - a0], axis=1).astype(np.int64).reshape(-1, 2)
    prep = con.prepare(pairs, None, np.zeros(a1 - a0, dtype=np.int64), 1, d['fixed'][a0:a1], 256)
    d2 = d['d2'][mine][prep.order]
    out = {k: d[k][a0:a1] for k in ('x', 'v', 'F', 'm', 'hk', 'w', 'sigma', 'xi', 'fixed')}
    mol_ptr = np.array([0, a1 - a0], dtype=np.int32)
    out.update(mol_ptr=mol_ptr, prep=prep, d2=d2, sizes=[a1 - a0], T=rr.Tables(prep, d2, mol_ptr),
               **{k: d[k] for k in ('dth', 'inv_dth', 'c1')})
    return out


# ---- 1. the kernel against fp64 on the same inputs, and the constraints as stored ------------------------------------------------

@pytest.mark.parametrize('flags, noise', FLAGS)
@pytest.mark.parametrize('name', list(rr.BATCHES))
def test_constrained_step_against_fp64_and_the_constraints_as_stored(name, flags, noise):
    from newtonnet_amd import hip
    d = rr.case(name)
    T = d['T']
    got, again = call(d, flags, noise), call(d, flags, noise)
    t = got['t']
    for k in ('x', 'v', 'F', 'w', 'hk'):
        assert torch.equal(t[k], torch.from_numpy(d[k]).cuda()), k                          # inputs intact
    for k in ('x', 'v', 'ke', 'n_sweeps', 'n_failed'):
        assert torch.equal(got[k], again[k]), k                                             # repeats are bitwise equal
    assert not got['n_failed'].any()
    sweeps = _np(got['n_sweeps'])
    assert np.all(sweeps[~T.has] == 0) and np.all(sweeps[T.has] >= 1) and sweeps.max() < rr.MAX_ITER // 2
    moves = bool(flags & (rr.BEGIN | rr.PROJECT))
    x, v, ke = _np(got['x']), _np(got['v']), _np(got['ke'])
    assert np.isfinite(v).all() and (not moves or np.isfinite(x).all())
    if not moves:
        assert torch.all(got['x'] == SENT)
    if not flags & rr.FINISH:
        assert torch.all(got['ke'] == SENT)
    # the constraints on what is stored
    worst = {}
    p_err, p_bound, v_err, v_bound = rr.stored_residuals(T, x if moves else d['x'], v, rr.TOL, d['dth'])
    if moves:
        worst['stored |r|^2'] = float((p_err / p_bound).max())
        assert np.all(p_err <= p_bound), worst
    worst['stored r.dv'] = float((v_err / v_bound).max())
    assert np.all(v_err <= v_bound), worst
    # against fp64 converged to 1e-13
    ref = rr.run(d, flags, noise, bound_tol=rr.TOL)
    assert not ref['failed'].any()
    raw, rel = rr.ratios(dict(x=x if moves else None, v=v, ke=ke if flags & rr.FINISH else None), ref, T, flags, noise)
    worst.update({f'{k} vs fp64': r for k, r in rel.items()})
    print(f'{name} flags {flags} noise {noise}: worst err / bound ' + ', '.join(f'{k} {r:.3f}' for k, r in worst.items())
          + f'; (err - rest) / summed response {raw} (MARGIN = {rr.MARGIN:.2f}); sweeps {sweeps.tolist()}')
    assert max(rel.values()) <= 1.0, rel
    # fixed atoms: bitwise where they were, zero velocity
    if d['fixed'].any():
        assert not np.any(v[d['fixed']]) and (not moves or np.array_equal(x[d['fixed']], d['x'][d['fixed']]))
    # a molecule without constraints: nnhip_md_step's bits
    free = ~T.con_atom
    if free.any():
        if flags == rr.PROJECT:
            assert np.array_equal(x[free], d['x'][free]) and np.array_equal(v[free], d['v'][free])
        else:
            vel, pos_out, ke2 = t['v'].clone(), torch.full_like(got['x'], SENT), torch.full_like(got['ke'], SENT)
            hip.md_step(t['x'] if moves else None, vel, t['F'], t['hk'], d['dth'], d['c1'], flags, pos_out=pos_out if moves else None,
                        mass=t['m'], sigma=t['sigma'] if noise else None, noise=t['xi'] if noise else None,
                        ke_out=ke2 if flags & rr.FINISH else None)
            idx = torch.from_numpy(free).cuda()
            assert torch.equal(got['v'][idx], vel[idx]) and torch.equal(got['x'][idx], pos_out[idx]) and torch.equal(got['ke'][idx], ke2[idx])


@pytest.mark.parametrize('flags, noise', FLAGS)
def test_a_batch_shifted_by_100_angstrom_takes_the_same_sweeps(flags, noise):
    """positions are multiples of 2^-16, so x + 100 is exact and the molecule-relative y is the same bit for bit: the solver cannot
    know where the molecule sits -- the same sweeps AND the same velocity bits"""
    a, b = rr.case('mixed'), rr.case('mixed_shift')
    assert np.array_equal((b['x'].astype(np.float64) - 100.0).astype(np.float32), a['x'])
    ga, gb = call(a, flags, noise), call(b, flags, noise)
    assert torch.equal(ga['n_sweeps'], gb['n_sweeps']) and not gb['n_failed'].any()
    con_atom = torch.from_numpy(a['T'].con_atom).cuda()
    assert torch.equal(ga['v'][con_atom], gb['v'][con_atom])
    print(f'flags {flags} noise {noise}: sweeps {ga["n_sweeps"].tolist()} at 0 and at 100 A')


@pytest.mark.parametrize('flags, noise', [(rr.FINISH | rr.BEGIN, True), (rr.PROJECT, False)])
def test_a_molecule_gives_the_same_bits_alone_and_inside_a_batch(flags, noise):
    d = rr.case('mixed9')
    whole = call(d, flags, noise)
    for b, n in enumerate(d['sizes']):
        if n == 0:
            continue
        one = call(sub_case(d, b), flags, noise)
        sl = slice(int(d['mol_ptr'][b]), int(d['mol_ptr'][b + 1]))
        for k in ('x', 'v', 'ke'):
            assert torch.equal(whole[k][sl], one[k]), (b, k)
        assert int(whole['n_sweeps'][b]) == int(one['n_sweeps'][0])


# ---- 2. the failure path -------------------------------------------------------------------------------------------------------

def test_max_iter_1_marks_failure_stores_finite_values_and_leaves_the_neighbours_alone():
    d = rr.case('mixed')
    flags = rr.FINISH | rr.BEGIN
    got = call(d, flags, True, max_iter=1)
    names = rr.BATCHES['mixed']
    failed = _np(got['n_failed'])
    assert failed[names.index('water')] == 1 and failed[names.index('free3')] == 0 and failed[names.index('empty')] == 0
    for k in ('x', 'v', 'ke'):
        assert torch.isfinite(got[k]).all(), k
    assert int(got['n_sweeps'].max()) == 1
    for b, n in enumerate(d['sizes']):                     # every molecule: the bits it gives alone under the same max_iter
        if n:
            one = call(sub_case(d, b), flags, True, max_iter=1)
            sl = slice(int(d['mol_ptr'][b]), int(d['mol_ptr'][b + 1]))
            assert all(torch.equal(got[k][sl], one[k]) for k in ('x', 'v', 'ke')) and int(one['n_failed'][0]) == failed[b]
    # sticky: a second launch on the same counters adds one
    again = call(d, flags, True, max_iter=1, n_failed=got['n_failed'].clone())
    assert np.array_equal(_np(again['n_failed']), 2 * failed)


@pytest.mark.parametrize('flags', [rr.PROJECT, rr.BEGIN])
def test_the_breakdown_guard_marks_failure_and_stores_finite_values(flags):
    """s.r <= NNHIP_MDC_GUARD d2.  Through the entry point the velocities are tangent before every drift, so s.r = |r|^2 + dth r.u
    stays at |r|^2 however far the bond turns; the guard is reached when the geometry is far from the table: a bond at 0.3 of its
    constrained length has s.r = 0.09 d2.  The constraint is skipped (no division by a small s.r), the molecule marked.
    (A reference rotated by 90 degrees against the drifted bond, the textbook breakdown, cannot be expressed through the entry
    point: it has no reference input of its own -- the reference of a drift is the position the drift starts from.)"""
    d = rr.case('diatomic')
    d['d2'] = (d['d2'] / np.float32(0.09)).astype(np.float32)
    d['T'] = rr.Tables(d['prep'], d['d2'], d['mol_ptr'])
    got = call(d, flags, False)
    assert int(got['n_failed'][0]) == 1
    assert torch.isfinite(got['x']).all() and torch.isfinite(got['v']).all()
    ref = rr.run(d, flags, False, fp32=True, tol=rr.TOL, max_iter=rr.MAX_ITER)
    assert ref['failed'][0]
    if flags == rr.PROJECT:                               # the skipped constraint moved nothing
        assert torch.equal(got['x'][1] - got['x'][0], got['t']['x'][1] - got['t']['x'][0])


def test_the_guard_on_one_molecule_of_a_batch_leaves_its_neighbours_their_bits():
    """the mixed batch with the table of its CH4 alone scaled so that every C-H sits at 0.3 of its constrained length: CH4 is
    marked and stores finite values, every other molecule has the bits of the batch with the sound table"""
    d = rr.case('mixed')
    flags, b = rr.FINISH | rr.BEGIN, rr.BATCHES['mixed'].index('ch4')
    sound = call(d, flags, True)
    bad = dict(d, d2=np.where(d['T'].mol == b, d['d2'] / np.float32(0.09), d['d2']).astype(np.float32))
    got = call(bad, flags, True)
    assert _np(got['n_failed']).tolist() == [int(k == b) for k in range(len(d['sizes']))] and not sound['n_failed'].any()
    for k in ('x', 'v', 'ke'):
        assert torch.isfinite(got[k]).all(), k
        others = torch.from_numpy(d['batch'] != b).cuda()
        assert torch.equal(got[k][others], sound[k][others]), k
    mine = torch.from_numpy(d['batch'] == b).cuda()
    assert not torch.equal(got['x'][mine], sound['x'][mine])
    keep = torch.arange(len(d['sizes']), device='cuda') != b
    assert torch.equal(got['n_sweeps'][keep], sound['n_sweeps'][keep])


def test_the_wrapper_refuses_aliasing_large_molecules_unsorted_tables_and_bad_flags():
    from newtonnet_amd import constraints as con
    from newtonnet_amd import hip
    d = rr.case('mixed')
    t = {k: torch.from_numpy(d[k]).cuda() for k in ('x', 'v', 'F', 'm', 'hk', 'w')}
    keep = {k: v.clone() for k, v in t.items()}
    N, B = d['x'].shape[0], len(d['sizes'])
    out = torch.full((N, 3), SENT, device='cuda')
    nf, ns = torch.zeros(B, dtype=torch.int32, device='cuda'), torch.zeros(B, dtype=torch.int32, device='cuda')
    tab = _tables(d)

    def step(flags=rr.BEGIN, pos_out=out, tables=tab, tol=rr.TOL, max_iter=rr.MAX_ITER, x=t['x']):
        hip.md_step_constrained(x, t['v'], t['F'], t['hk'], t['w'], d['dth'], d['inv_dth'], 1.0, flags, tables, tol, max_iter, nf, ns,
                                pos_out=pos_out, mass=t['m'])
    with pytest.raises(hip.HipLibraryError, match='alias'):
        step(pos_out=t['x'])
    for flags in (0, 5, 6, 8):
        with pytest.raises(hip.HipLibraryError, match='flags'):
            step(flags=flags)
    with pytest.raises(hip.HipLibraryError, match='tol'):
        step(tol=0.0)
    with pytest.raises(hip.HipLibraryError, match='max_iter'):
        step(max_iter=0)
    bad = tab.col_ptr_host.clone()
    bad[1] = bad[2] + 1
    assert bool((bad[1:] < bad[:-1]).any())
    with pytest.raises(hip.HipLibraryError, match='unsorted'):
        step(tables=tab._replace(col_ptr_host=bad))
    worse = tab.mol_col_ptr_host.clone()
    worse[-1] += 1
    with pytest.raises(hip.HipLibraryError, match='unsorted'):
        step(tables=tab._replace(mol_col_ptr_host=worse))
    with pytest.raises(ValueError, match='n_failed'):
        hip.md_step_constrained(t['x'], t['v'], t['F'], t['hk'], t['w'], d['dth'], d['inv_dth'], 1.0, rr.BEGIN, tab, rr.TOL, 10,
                                nf.long(), ns, pos_out=out, mass=t['m'])
    # a molecule with a constraint and one atom more than the LDS form takes
    n = hip.md_constrained_max_atoms() + 1
    assert n == hip.MDC_MAX_ATOMS + 1
    prep = con.prepare(np.array([[0, 1]]), None, np.zeros(n, dtype=np.int64), 1)
    big = con.device_tables(prep, np.ones(1, dtype=np.float32), torch.tensor([0, n], dtype=torch.int32).cuda())
    z3, z1 = torch.zeros(n, 3, device='cuda'), torch.ones(n, device='cuda')
    big_out = torch.full((n, 3), SENT, device='cuda')
    one = torch.zeros(1, dtype=torch.int32, device='cuda')
    with pytest.raises(hip.HipLibraryError, match='above the'):
        hip.md_step_constrained(z3, z3.clone(), z3, z1, z1, d['dth'], d['inv_dth'], 1.0, rr.BEGIN, big, rr.TOL, 10, one, one.clone(),
                                pos_out=big_out)
    torch.cuda.synchronize()
    assert all(torch.equal(t[k], keep[k]) for k in t) and torch.all(out == SENT) and torch.all(big_out == SENT)     # nothing written
    assert not nf.any() and not ns.any() and not one.any()
    empty = torch.zeros(0, 3, device='cuda')
    hip.md_step_constrained(empty, empty.clone(), empty, z1[:0], z1[:0], d['dth'], d['inv_dth'], 1.0, rr.BEGIN, tab, rr.TOL, 10, nf, ns,
                            pos_out=empty.clone())                                                       # n_atoms = 0: a no-op


# ---- 3. the driver ---------------------------------------------------------------------------------------------------------------

def _forces(model, z, pos, cell, batch):
    return model(z, pos, cell, batch).gradient_force.clone()


def _aspirin8():
    z, pos, cell, batch, _ = util.case_inputs('aspirin8_rand', torch.float32)
    return cuda(z, pos, cell, batch)


def _ref_tables(dyn):
    """rattle_ref.Tables of a Dynamics (its sorted pairs coloured again: the order within a converged solve does not matter)"""
    from newtonnet_amd import constraints as con
    prep = con.prepare(_np(dyn.constraint_pairs), None, _np(dyn.batch), dyn.n_mol)
    d2 = _np(dyn._con.con_d2)[prep.order]
    return rr.Tables(prep, d2, _np(dyn._mol_ptr))


def check_stepwise(model, dyn, T, z, cell, batch, frames_pos, frames_vel, noises, label):
    """frames k and k + 1 are consecutive full steps: BEGIN with the forces at frame k, FINISH with those at frame k + 1, in fp64
    converged to 1e-13, must land on frame k + 1 within the kernel-alone bound of the two launches + hk x util.FORCE_MAX_TOL"""
    hk, m, w = _np(dyn._hk), _np(dyn.masses), _np(dyn._inv_mass)
    sigma = None if dyn._sigma is None else _np(dyn._sigma)
    F = [_np(_forces(model, z, p, cell, batch)) for p in frames_pos]
    worst = dict(x=0.0, v=0.0)
    for k in range(len(frames_pos) - 1):
        xi = None if sigma is None else _np(noises[k])
        args = dict(sigma=sigma, xi=xi, c1=dyn._c1, dth=dyn._dth, inv_dth=dyn._inv_dth)
        a = rr.launch(rr.BEGIN, _np(frames_pos[k]), _np(frames_vel[k]), F[k], hk, m, w, T, bound_tol=dyn._con_tol, **args)
        a['U'] = rr.launch(rr.BEGIN, _np(frames_pos[k]), _np(frames_vel[k]), F[k], hk, m, w, T, tol=dyn._con_tol, **args)['n_sweeps']
        b = rr.launch(rr.FINISH, _np(frames_pos[k + 1]), a['v'], F[k + 1], hk, m, w, T, bound_tol=dyn._con_tol, dth=dyn._dth,
                      inv_dth=dyn._inv_dth)
        b['U'] = a['U']
        assert not a['failed'].any() and not b['failed'].any()
        bx, bva, _ = rr.fp64_bounds(a, T, rr.BEGIN, xi is not None)
        _, bvb, _ = rr.fp64_bounds(b, T, rr.FINISH, False)
        bv = bva + bvb + hk.astype(np.float64)[:, None] * util.FORCE_MAX_TOL
        e_x = np.abs(_np(frames_pos[k + 1]).astype(np.float64) - a['x'])
        e_v = np.abs(_np(frames_vel[k + 1]).astype(np.float64) - b['v'])
        worst['x'], worst['v'] = max(worst['x'], float((e_x / bx).max())), max(worst['v'], float((e_v / bv).max()))
        assert np.all(e_x <= bx), f'{label}: step {k} -> {k + 1}: positions err / bound {float((e_x / bx).max()):.3f}'
        assert np.all(e_v <= bv), f'{label}: step {k} -> {k + 1}: velocities err / bound {float((e_v / bv).max()):.3f}'
    print(f'{label}: {len(frames_pos) - 1} steps, worst err / bound positions {worst["x"]:.4f}, velocities {worst["v"]:.4f}')


@pytest.mark.parametrize('thermostat', ['nve', 'langevin'])
def test_every_recorded_step_of_a_constrained_run_follows_from_the_one_before(thermostat):
    z, pos, cell, batch = _aspirin8()
    model = make_model(util.load_state('rand'))
    kw = dict(temperature=300.0) if thermostat == 'nve' else dict(temperature=300.0, friction=0.02)
    gen = torch.Generator(device='cuda').manual_seed(7)
    dyn = model.dynamics(z, pos, cell, batch, generator=gen, timestep=2.0, constraints='h-bonds', **kw)
    assert dyn.constraint_pairs.shape == (64, 2)
    p0, v0 = dyn.positions, dyn.velocities
    n_steps = 40
    traj = dyn.run(n_steps, record_every=1)
    regen = torch.Generator(device='cuda').manual_seed(7)
    torch.randn(tuple(pos.shape), generator=regen, device='cuda')                      # the Maxwell-Boltzmann draw
    noises = [torch.randn(tuple(pos.shape), generator=regen, device='cuda') for _ in range(n_steps)] if dyn._sigma is not None else None
    T = _ref_tables(dyn)
    check_stepwise(model, dyn, T, z, cell, batch, [p0] + list(traj.pos), [v0] + list(traj.vel), noises, f'aspirin8 h-bonds {thermostat} 2 fs')
    assert not dyn.constraint_failures.any() and int(dyn.constraint_sweeps.max()) < dyn._con_max_iter // 4
    dof = 3 * 21 - 8
    np.testing.assert_allclose(_np(traj.temperature), 2.0 * _np(traj.kinetic_energy) / (dof * 8.617333262e-5), rtol=1e-6)


def test_bond_lengths_hold_over_200_steps_and_the_bitwise_properties():
    z, pos, cell, batch = _aspirin8()
    model = make_model(util.load_state('rand'))

    def make(seed=7, **kw):
        gen = torch.Generator(device='cuda').manual_seed(seed)
        return model.dynamics(z, pos, cell, batch, temperature=300.0, friction=0.02, timestep=2.0, generator=gen, constraints='h-bonds', **kw)
    dyn = make()
    traj = dyn.run(200, record_every=1)
    T = _ref_tables(dyn)
    worst = 0.0
    for k in range(200):
        p_err, p_bound, v_err, v_bound = rr.stored_residuals(T, _np(traj.pos[k]), _np(traj.vel[k]), dyn._con_tol, dyn._dth)
        worst = max(worst, float((p_err / p_bound).max()), float((v_err / v_bound).max()))
        assert np.all(p_err <= p_bound) and np.all(v_err <= v_bound), k
    sweeps = int(dyn.constraint_sweeps.max())
    print(f'200 Langevin steps at 2 fs, 64 X-H bonds: worst stored residual / bound {worst:.3f}; failures '
          f'{dyn.constraint_failures.tolist()}; sweeps of the last launch {sweeps} (max_iter {dyn._con_max_iter})')
    assert not dyn.constraint_failures.any() and sweeps < dyn._con_max_iter // 4
    assert torch.isfinite(traj.total_energy).all()
    # seeded repeats, record_every 0 against 7, run(13); run(27) against run(40)
    a, b = make().run(40, 0), make().run(40, 7)
    assert b.step.tolist() == [7, 14, 21, 28, 35, 40]
    c = make()
    c.run(13, 0)
    c27 = c.run(27, 0)
    for name in ('pos', 'vel', 'potential_energy', 'kinetic_energy'):
        assert torch.equal(getattr(a, name)[0], getattr(b, name)[-1]), name
        assert torch.equal(getattr(a, name)[0], getattr(c27, name)[0]), name
    assert torch.equal(a.pos[0], traj.pos[39]) and torch.equal(a.vel[0], traj.vel[39]) and torch.equal(a.kinetic_energy[0], traj.kinetic_energy[39])
    assert not torch.equal(make(seed=8).run(40, 0).pos, a.pos)


def test_initial_velocities_are_tangent_and_given_lengths_are_imposed():
    """Maxwell-Boltzmann draws are projected at construction.  Temperature: per molecule 2 KE / ((3 n - C) k_B) with the centre of
    mass momentum removed, so 3 n - C - 3 = 52 degrees of freedom carry kinetic energy and the estimate over B = 8 molecules is
    T chi^2_(416) / 440: mean 300 x 416 / 440 = 283.6 K, standard deviation 300 sqrt(2 x 416) / 440 = 19.7 K; the test allows 4."""
    from newtonnet_amd import constraints as con
    z, pos, cell, batch = _aspirin8()
    model = make_model(util.load_state('rand'))
    gen = torch.Generator(device='cuda').manual_seed(3)
    dyn = model.dynamics(z, pos, cell, batch, temperature=300.0, timestep=2.0, generator=gen, constraints='h-bonds')
    T = _ref_tables(dyn)
    p_err, p_bound, v_err, v_bound = rr.stored_residuals(T, _np(dyn.positions), _np(dyn.velocities), dyn._con_tol, dyn._dth)
    assert np.all(p_err <= p_bound) and np.all(v_err <= v_bound)
    t_est = float((2.0 * dyn.kinetic_energy / (dyn._dof * 8.617333262e-5)).mean())
    mean, std = 300.0 * 416 / 440, 300.0 * np.sqrt(2.0 * 416) / 440
    print(f'projected Maxwell-Boltzmann at 300 K: estimate {t_est:.1f} K, expected {mean:.1f} +- {std:.1f} K; stored residual / bound '
          f'{float((p_err / p_bound).max()):.3f}, {float((v_err / v_bound).max()):.3f}')
    assert abs(t_est - mean) <= 4.0 * std
    # the same draw without constraints is NOT tangent
    free = model.dynamics(z, pos, cell, batch, temperature=300.0, timestep=2.0, generator=torch.Generator(device='cuda').manual_seed(3))
    _, _, v_err, v_bound = rr.stored_residuals(T, _np(free.positions), _np(free.velocities), dyn._con_tol, dyn._dth)
    assert np.all(v_err.reshape(8, 8).max(1) > 10.0 * v_bound.max())
    # explicit lengths: 1.09 A for every C-H, the present distance for O-H
    pairs, lengths = con.hydrogen_constraints(z, pos, batch)
    lengths = torch.where(z[pairs[:, 0]] == 6, torch.full_like(lengths, 1.09), lengths)
    given = model.dynamics(z, pos, cell, batch, timestep=2.0, constraints=(pairs, lengths))
    x = given.positions.double()
    cp = given.constraint_pairs
    dist = (x[cp[:, 0]] - x[cp[:, 1]]).norm(dim=1)
    assert torch.equal(given.constraint_lengths, lengths[torch.from_numpy(con.prepare(_np(pairs), None, _np(batch), 8).order).cuda()])
    p_err, p_bound, _, _ = rr.stored_residuals(_ref_tables(given), _np(given.positions), None, given._con_tol, given._dth)
    assert np.all(p_err <= p_bound) and float((dist - given.constraint_lengths.double()).abs().max()) < 1e-5
    assert int((z[cp[:, 0]] == 6).sum()) == 56 and float((dist[z[cp[:, 0]] == 6] - 1.09).abs().max()) < 1e-5
    assert not torch.equal(given.positions, pos) and not given.velocities.any() and not given.constraint_failures.any()
    with pytest.raises(ValueError, match='could not be brought onto the constraints'):
        model.dynamics(z, pos, cell, batch, constraints=(pairs, lengths), constraint_max_iter=1)
    with pytest.raises(ValueError, match='two molecules'):
        model.dynamics(z, pos, cell, batch, constraints=(torch.tensor([[0, 21]], device='cuda'), None))


class FakeAtoms:
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


def test_run_md_with_constraints_matches_model_dynamics_bitwise():
    from newtonnet_amd.utils import MLAseCalculator
    z, pos, cell, batch, _ = util.case_inputs('aspirin8_rand', torch.float32)
    model = make_model(util.load_state('rand'))
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda')
    frames = [FakeAtoms(z[:21].numpy(), pos[21 * k:21 * (k + 1)].numpy()) for k in range(3)]
    out = calc.run_md(frames, 12, timestep=2.0, temperature=300.0, friction=0.01, record_every=5, seed=5, constraints='h-bonds')
    assert out['step'].tolist() == [5, 10, 12] and out['constraint_failures'].tolist() == [0, 0, 0]
    zc, pc, cc, bc = calc.format_data(frames)
    gen = torch.Generator(device='cuda').manual_seed(5)
    dyn = model.dynamics(zc, pc.float(), cc.float(), bc, temperature=300.0, friction=0.01, timestep=2.0, generator=gen, constraints='h-bonds')
    traj = dyn.run(12, 5)
    assert np.array_equal(out['positions'].reshape(3, 63, 3), _np(traj.pos)) and np.array_equal(out['velocities'].reshape(3, 63, 3), _np(traj.vel))
    assert np.array_equal(out['energy'], _np(traj.potential_energy)) and np.array_equal(out['kinetic_energy'], _np(traj.kinetic_energy))
    # pairs within one frame, applied to every frame: the same bits as the global pairs
    from newtonnet_amd import constraints as con
    local = _np(con.hydrogen_constraints(zc[:21], pc[:21], bc[:21])[0])
    again = calc.run_md(frames, 12, timestep=2.0, temperature=300.0, friction=0.01, record_every=5, seed=5, constraints=(local, None))
    assert all(np.array_equal(out[k], again[k]) for k in out)
    # device tensors are taken as well; one structure drops the frame axis, of constraint_failures too
    one = calc.run_md(frames[0], 3, timestep=2.0, constraints=(torch.from_numpy(local).cuda(), torch.full((8,), 1.05).cuda()),
                      constraint_max_iter=40)
    assert one['positions'].shape == (1, 21, 3) and one['constraint_failures'].shape == () and int(one['constraint_failures']) == 0
    bond = np.linalg.norm(one['positions'][0, local[:, 0]].astype(np.float64) - one['positions'][0, local[:, 1]], axis=1)
    assert np.abs(bond - 1.05).max() < 1e-5
    free = calc.run_md(frames, 12, timestep=2.0, temperature=300.0, friction=0.01, record_every=5, seed=5)
    assert 'constraint_failures' not in free and not np.array_equal(free['positions'], out['positions'])



# ---- 4. energy conservation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('timestep', [0.5, 2.0])
def test_energy_conservation_of_constrained_nve_against_a_host_fp64_loop(timestep):
    """4 aspirins (the first four of aspirin8_rand), seeded weights, 'h-bonds', Maxwell-Boltzmann at 300 K (projected), 400
    microcanonical steps.  Per molecule, max_n |E_tot(n) - E_tot(0)| <= (a) the same figure of a host fp64 loop of the same scheme
    (rattle_ref.host_energy_drift, model() forces) at the same tolerance from the same start + (b) the first-order cost of the fp32
    state, as test_hip_md has it, sum over steps of [sum_i |F_i| ulp(x_i) / 2 + sum_i m_i v_i^2 2^-24] + (c) 2 util.energy_tol(E) +
    (d) 2 x |the host figure at the tolerance - the host figure at 1e-13|: what stopping the solves at the tolerance does to the
    energy, a reference-only measurement.  The 2 fs run must also not blow up: no constraint failure, finite energies, and a
    drift below the molecule's initial kinetic energy.  Both figures are printed.
    Observed: 0.5 fs drift 0.75, 0.60, 0.42, 0.41 meV against host figures of 0.74, 0.59, 0.42, 0.41 meV at either tolerance (tolerance
    term <= 0.003 meV), drift / bound 0.72 .. 0.82; 2 fs drift 10.1, 10.9, 6.7, 6.9 meV against 10.1, 10.9, 9.6, 7.4 meV of the host
    loop at 1e-13, drift / bound <= 0.88."""
    from tests import md_ref as mr
    n_steps, B, n = 400, 4, 21
    z, pos, cell, batch = _aspirin8()
    z, pos, cell, batch = z[:B * n], pos[:B * n], cell[:B], batch[:B * n]
    model = make_model(util.load_state('rand'))
    gen = torch.Generator(device='cuda').manual_seed(11)
    dyn = model.dynamics(z, pos, cell, batch, temperature=300.0, timestep=timestep, generator=gen, constraints='h-bonds')
    p0, v0 = dyn.positions, dyn.velocities
    e0, k0 = dyn.potential_energy.clone(), dyn.kinetic_energy
    traj = dyn.run(n_steps, record_every=1)
    m = _np(dyn.masses).astype(np.float64)
    pe = np.concatenate([_np(e0)[None], _np(traj.potential_energy)]).astype(np.float64)
    ke = np.concatenate([_np(k0)[None], _np(traj.kinetic_energy)]).astype(np.float64)
    tot = pe + ke
    drift = np.abs(tot - tot[0]).max(axis=0)
    T = _ref_tables(dyn)

    def evaluate(xx):
        out = model(z, torch.from_numpy(xx).float().cuda(), cell, batch)
        return _np(out.gradient_force).astype(np.float64), _np(out.energy).astype(np.float64)
    args = (evaluate, _np(p0), _np(v0), _np(dyn._hk), m, _np(dyn._inv_mass), T, dyn._dth, dyn._inv_dth)
    a, a13 = rr.host_energy_drift(*args, dyn._con_tol, n_steps), rr.host_energy_drift(*args, 1e-13, n_steps)
    b = np.zeros(B)
    for k in range(n_steps):
        F = _np(_forces(model, z, traj.pos[k], cell, batch)).astype(np.float64)
        xk, vk = _np(traj.pos[k]), _np(traj.vel[k]).astype(np.float64)
        b += ((np.abs(F) * mr.half_ulp32(xk)).sum(1) + m * (vk * vk).sum(1) * mr.EPS32).reshape(B, n).sum(1)
    c = 2.0 * util.energy_tol(pe[0])
    d = 2.0 * np.abs(a - a13)
    bound = a + b + c + d
    swing = ke.max(axis=0) - ke.min(axis=0)
    print(f'constrained NVE, {timestep} fs x {n_steps}: drift {drift} eV, bound {bound} = host fp64 at tol {a} + fp32 state {b} + energy '
          f'ulps {c} + tolerance term {d} (host at 1e-13: {a13}); drift / bound {drift / bound}; kinetic energy swing {swing} eV; '
          f'initial kinetic energy {ke[0]} eV; failures {dyn.constraint_failures.tolist()}')
    assert not dyn.constraint_failures.any() and np.isfinite(tot).all()
    assert np.all(drift < ke[0]), f'blow-up: drift {drift} eV against an initial kinetic energy of {ke[0]} eV'
    assert np.all(drift <= bound), f'drift / bound {drift / bound}'
    if timestep == 0.5:      # (at 2 fs over 800 fs the host loops leave the device's trajectory -- one of them meets a close contact
        # that costs it 0.8 eV -- so there the bound is the reference's own scatter; the power of the test is the 0.5 fs case)
        assert np.all(swing >= 10.0 * bound), f'kinetic energy swing / bound {swing / bound}: the test has no power'
