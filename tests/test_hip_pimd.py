"""Path-integral molecular dynamics on the HIP path (newtonnet_amd/pimd.py, csrc/pimd.hip).

Kernel alone: nnhip_pimd_step on synthetic inputs against its fp64 restatement on the SAME fp32 inputs (tests/pimd_ref.py), every
output within the derived first-order rounding bound (C_PI = 2) plus half an fp32 ulp of the stored value; the tests print err /
bound.  Driver: with one bead it is `Dynamics` bit for bit; every recorded step is checked ONE step at a time -- forces recomputed
on the recorded bead positions, noise regenerated from the seed -- so no error compounds; RPMD conserves the ring-polymer energy as
well as a host fp64 loop of the same scheme plus the first-order cost of keeping the state in fp32; the estimators are recomputed
from the recorded frames."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import pimd_ref as pr
from tests import util
from tests.test_hip_hessian import cuda, make_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_B = 8.617333262e-5


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. the kernel against fp64 on the same inputs ------------------------------------------------------------------------------

def _synthetic(P, sizes, seed):
    """systems of `sizes` atoms x P slots: |u| <= 8, |w| <= 0.2, |F| <= 5 eV / A, tables of hydrogen / carbon at 300 K and below"""
    from newtonnet_amd import pimd
    rng = np.random.default_rng(seed)
    f32 = np.float32
    G = len(sizes)
    ptr = np.concatenate([[0], np.cumsum(np.repeat(sizes, P))]).astype(np.int32)
    N = int(ptr[-1])
    u, w, F = (rng.uniform(-8, 8, (N, 3)).astype(f32), rng.uniform(-0.2, 0.2, (N, 3)).astype(f32), rng.uniform(-5, 5, (N, 3)).astype(f32))
    xi = rng.standard_normal((N, 3)).astype(f32)
    T = np.linspace(300.0, 200.0, G)
    m = np.concatenate([np.tile(rng.choice(np.array([1.008, 12.011]), n), P) for n in sizes])          # one mass per atom, in every slot
    mol = np.repeat(np.arange(G * P), np.repeat(sizes, P))
    tab, one_minus = pimd.mode_tables(P, T, 0.25, 0.01, 1.0)
    dt = 0.25 * pimd.FS
    hk = (0.5 * dt / m).astype(f32)
    sigma = np.sqrt(one_minus.reshape(-1)[mol] * K_B * (P * T)[mol // P] / m).astype(f32)
    C = pimd.transform_matrix(P).astype(f32)
    return dict(ptr=ptr, u=u, w=w, F=F, xi=xi, m=m.astype(f32), hk=hk, sigma=sigma, C=C, tab=tab.reshape(G * P, 5))


def _launch(d, P, flags, with_noise, est=True, sentinel=777.0):
    from newtonnet_amd import hip
    t = {k: torch.from_numpy(d[k]).cuda() for k in ('u', 'w', 'F', 'xi', 'm', 'hk', 'sigma', 'C', 'tab', 'ptr')}
    N = d['u'].shape[0]
    pos_out = torch.full((N, 3), sentinel, device='cuda')
    est_out = torch.full((N, 4), sentinel, device='cuda')
    hip.pimd_step(t['u'], t['w'], t['F'], t['C'], t['tab'], t['hk'], t['ptr'], torch.from_numpy(d['ptr']), P, flags,
                  pos_out=pos_out if flags & pr.BEGIN else None, mass=t['m'], sigma=t['sigma'] if with_noise else None,
                  noise=t['xi'] if with_noise else None, est_out=est_out if (flags & pr.FINISH and est) else None)
    return t, pos_out, est_out


def _reference(d, P, flags, with_noise):
    def fn(**a):
        return pr.pimd_step(flags, a['u'], a['w'], a['F'], d['C'], a['tab'], a['hk'], a['m'], a['sigma'] if with_noise else None,
                            a['xi'] if with_noise else None)
    return pr.flat(fn, d['ptr'], P, dict(u=d['u'], w=d['w'], F=d['F'], xi=d['xi'], hk=d['hk'], m=d['m'], sigma=d['sigma']),
                   dict(tab=d['tab']))


@pytest.mark.parametrize('with_noise', [False, True])
@pytest.mark.parametrize('flags', [pr.FINISH, pr.BEGIN, pr.FINISH | pr.BEGIN])
@pytest.mark.parametrize('P', [1, 2, 3, 5, 8, 33, 64])
def test_pimd_step_against_fp64_on_the_same_inputs(P, flags, with_noise):
    from newtonnet_amd import hip
    cap = hip.pimd_tile_atoms(P)
    sizes = [cap - 1, cap, cap + 1, 1]                 # one below, at and one above a tile, and a single atom
    d = _synthetic(P, sizes, 100 + P)
    t, pos_out, est_out = _launch(d, P, flags, with_noise)
    ref = _reference(d, P, flags, with_noise)
    for k in ('F', 'xi', 'm', 'hk', 'sigma', 'C', 'tab', 'ptr'):                              # inputs intact
        assert np.array_equal(_np(t[k]), d[k]), k
    worst = {}

    def check(name, got, want, bound):
        e = np.abs(_np(got).astype(np.float64) - want)
        b = bound + pr.half_ulp32(want)
        worst[name] = float((e / b).max())
        assert np.all(e <= b), f'{name}: err / bound {worst[name]:.3f}'
    check('w', t['w'], ref['w'], ref['bw'])
    if flags & pr.BEGIN:
        check('u', t['u'], ref['u'], ref['bu'])
        check('x', pos_out, ref['x'], ref['bx'])
    else:
        assert np.array_equal(_np(t['u']), d['u']) and torch.all(pos_out == 777.0)
    if flags & pr.FINISH:
        check('est', est_out, ref['est'], ref['best'])
        assert not _np(est_out)[:, 3].any()
    else:
        assert torch.all(est_out == 777.0)
    print(f'pimd_step P = {P}, sizes {sizes}, flags = {flags}, noise {with_noise}: worst err / bound '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f' (C_PI = {pr.C_PI})')
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize('with_noise', [False, True])
@pytest.mark.parametrize('flags', [pr.FINISH, pr.BEGIN, pr.FINISH | pr.BEGIN])
@pytest.mark.parametrize('N', [1, 257])
def test_one_bead_gives_md_step_bits(N, flags, with_noise):
    """csrc/pimd.hip's head comment: with P = 1 (C = [1], a = 1, b = dth, d = 0) the chain is md_step_kernel's.  The products with 1
    and fma(0, u, w) are exact, so u plays pos_in and every output carries nnhip_md_step's bits."""
    from newtonnet_amd import hip
    assert (pr.FINISH, pr.BEGIN) == (hip.MD_FINISH, hip.MD_BEGIN)
    d = _synthetic(1, [N], 700 + N)
    dth, c1 = np.float32(0.5 * 0.25 * 0.0982269), np.float32(np.exp(-0.01))
    d['C'] = np.ones((1, 1), dtype=np.float32)
    d['tab'] = np.array([[1.0, dth, 0.0, c1, 0.0]], dtype=np.float32)
    t, pos_out, est_out = _launch(d, 1, flags, with_noise)
    m = {k: torch.from_numpy(d[k]).cuda() for k in ('u', 'w', 'F', 'xi', 'm', 'hk', 'sigma')}
    md_pos, md_ke = torch.full((N, 3), 777.0, device='cuda'), torch.full((N,), 777.0, device='cuda')
    begin, finish = bool(flags & pr.BEGIN), bool(flags & pr.FINISH)
    hip.md_step(m['u'] if begin else None, m['w'], m['F'], m['hk'], float(dth), float(c1), flags, pos_out=md_pos if begin else None,
                mass=m['m'], sigma=m['sigma'] if with_noise else None, noise=m['xi'] if with_noise else None,
                ke_out=md_ke if finish else None)

    def same(name, got, want):
        assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32)), f'{name}: not the bits of nnhip_md_step'
    same('w', t['w'], m['w'])
    same('pos_out', pos_out, md_pos)                              # (both still the sentinel without begin)
    same('u', t['u'], md_pos if begin else m['u'])
    same('est_out[:, 0]', est_out[:, 0], md_ke)                   # (both still the sentinel without finish)
    assert not torch.equal(m['w'], torch.from_numpy(d['w']).cuda())


# ---- 2. what a launch may not touch ---------------------------------------------------------------------------------------------

def test_what_a_launch_may_not_touch_and_refusals():
    from newtonnet_amd import hip
    P = 5
    cap = hip.pimd_tile_atoms(P)
    d = _synthetic(P, [cap + 3, 2], 9)
    N = d['u'].shape[0]
    # est_out = NULL writes none; two identical launches give identical bits
    a, pos_a, est_a = _launch(d, P, pr.FINISH | pr.BEGIN, True, est=False)
    assert torch.all(est_a == 777.0)
    a, pos_a, est_a = _launch(d, P, pr.FINISH | pr.BEGIN, True)
    b, pos_b, est_b = _launch(d, P, pr.FINISH | pr.BEGIN, True)
    for x, y in ((a['u'], b['u']), (a['w'], b['w']), (pos_a, pos_b), (est_a, est_b)):
        assert torch.equal(x, y)
    # finish alone writes neither u nor pos_out (covered per case above as well)
    c, pos_c, _ = _launch(d, P, pr.FINISH, False)
    assert np.array_equal(_np(c['u']), d['u']) and torch.all(pos_c == 777.0)
    # a system's outputs do not depend on the rest of the batch: the second system alone
    n0 = P * (cap + 3)
    alone = {k: (v[n0:] if v.shape[0] == N else v) for k, v in d.items()}
    alone['ptr'] = (d['ptr'][P:] - d['ptr'][P]).astype(np.int32)
    alone['tab'] = d['tab'][P:]
    e, pos_e, est_e = _launch(alone, P, pr.FINISH | pr.BEGIN, True)
    assert torch.equal(e['u'], a['u'][n0:]) and torch.equal(e['w'], a['w'][n0:]) and torch.equal(pos_e, pos_a[n0:])
    assert torch.equal(est_e, est_a[n0:])
    # ---- refusals: NNHIP_E_INVALID, nothing launched
    t = {k: torch.from_numpy(d[k]).cuda() for k in ('u', 'w', 'F', 'xi', 'm', 'hk', 'sigma', 'C', 'tab', 'ptr')}
    keep_u, keep_w = t['u'].clone(), t['w'].clone()
    out, est = torch.full((N, 3), 777.0, device='cuda'), torch.full((N, 4), 777.0, device='cuda')
    host = torch.from_numpy(d['ptr'])

    def call(flags=pr.FINISH | pr.BEGIN, ptr_host=host, n_beads=P, C=t['C'], tab=t['tab'], pos_out=out, **kw):
        hip.pimd_step(t['u'], t['w'], t['F'], C, tab, t['hk'], t['ptr'], ptr_host, n_beads, flags, pos_out=pos_out, **kw)
    short = host.clone()
    short[-1] -= 1
    shifted = host.clone()
    shifted[0] = 1
    unequal = host.clone()
    unequal[1] += 1
    for bad, match in ((dict(ptr_host=short), 'mol_ptr must run'), (dict(ptr_host=shifted), 'mol_ptr must run'),
                       (dict(ptr_host=unequal), 'equal counts'),
                       (dict(n_beads=0, C=torch.zeros(0, device='cuda')), 'n_beads'),
                       (dict(n_beads=65, C=torch.zeros(65, 65, device='cuda')), 'n_beads'),
                       (dict(n_beads=3, C=torch.zeros(3, 3, device='cuda')), 'n_beads'),           # 10 molecules: 3 does not divide
                       (dict(pos_pending=out), 'alias'),
                       (dict(sigma=t['sigma']), 'sigma and noise'), (dict(noise=t['xi']), 'sigma and noise'),
                       (dict(flags=pr.BEGIN, est_out=est, mass=t['m']), 'est_out needs finish'),
                       (dict(est_out=est), 'mass'), (dict(flags=0), 'flags'), (dict(flags=4), 'flags'),
                       (dict(pos_out=None), 'pos_out')):
        with pytest.raises(hip.HipLibraryError, match=match):
            call(**bad)
    flat = torch.zeros(3 * N + 3, device='cuda')
    with pytest.raises(hip.HipLibraryError, match='alias'):                                        # an overlapping view is an alias too
        call(pos_pending=flat[:3 * N].view(N, 3), pos_out=flat[3:].view(N, 3))
    torch.cuda.synchronize()
    assert torch.equal(t['u'], keep_u) and torch.equal(t['w'], keep_w) and torch.all(out == 777.0) and torch.all(est == 777.0)
    assert not flat.any()
    empty = torch.zeros(0, 3, device='cuda')
    zero_ptr = torch.zeros(P + 1, dtype=torch.int32)
    hip.pimd_step(empty.clone(), empty.clone(), empty, t['C'], t['tab'][:P], torch.zeros(0, device='cuda'), zero_ptr.cuda(), zero_ptr, P,
                  pr.BEGIN, pos_out=empty.clone())                                                # no atoms: a no-op


# ---- 3. one bead is Dynamics ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('thermostat', ['nve', 'langevin'])
def test_one_bead_is_dynamics_bit_for_bit(thermostat):
    z, pos, cell, batch = _bench().synthetic_aspirin(8, 0, 'cuda')
    model = make_model(util.load_state('rand'))
    if thermostat == 'nve':
        T, friction = 300.0, 0.0
    else:
        T, friction = torch.linspace(200.0, 400.0, 8).cuda(), 0.02
    dyn = model.dynamics(z, pos, cell, batch, temperature=T, friction=friction, timestep=0.25,
                         generator=torch.Generator(device='cuda').manual_seed(5))
    ref = dyn.run(20, record_every=1)
    pi = model.path_integral(z, pos, cell, batch, 1, T, timestep=0.25, centroid_friction=friction,
                             generator=torch.Generator(device='cuda').manual_seed(5))
    assert (pi._sigma is None) == (thermostat == 'nve')
    got = pi.run(20, record_every=1)
    for name in ('pos', 'vel', 'kinetic_energy', 'potential_energy'):
        x, y = getattr(got, name), getattr(ref, name)
        assert x.dtype == torch.float32 and torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert torch.equal(got.step, ref.step) and torch.equal(got.mode_pos, got.pos) and torch.equal(got.mode_vel, got.vel)


# ---- 4. stepwise consistency of the driver --------------------------------------------------------------------------------------

def _forces(model, z, pos, cell, batch):
    out = model(z, pos, cell, batch)
    return out.gradient_force.clone(), out.energy.clone()


def check_stepwise(model, z, cell, batch, ptr, P, C, tab, hk, m, sigma, frames_u, frames_w, frames_x, noises, label):
    """frames k and k + 1 are consecutive full steps: one pimd_ref.full_step from the mode state of frame k, with the forces the
    model returns on the two recorded bead geometries and the noise of that step, must land on frame k + 1 within the bound; and the
    recorded bead positions are the back-transform of the recorded mode positions"""
    F = [_np(_forces(model, z, x, cell, batch)[0]) for x in frames_x]
    c_abs = np.abs(C.astype(np.float64)).sum(1)                                               # [P]: sum_s |C[k][s]|
    slot = np.concatenate([np.repeat(np.arange(P), n) for _, n in pr.systems(ptr, P)])
    force_term = hk.astype(np.float64)[:, None] * c_abs[slot][:, None] * util.FORCE_MAX_TOL
    worst = dict(u=0.0, w=0.0, x=0.0, back=0.0)
    for k in range(len(frames_x)):
        def back(**a):
            x, bx = pr.transform(C.astype(np.float64), a['u'].astype(np.float64), 0.0, transpose=True)
            return dict(x=x, bx=pr.C_PI * bx + pr.TINY32)
        r = pr.flat(back, ptr, P, dict(u=_np(frames_u[k])), {})
        e = np.abs(_np(frames_x[k]).astype(np.float64) - r['x'])
        b = r['bx'] + pr.half_ulp32(r['x'])
        worst['back'] = max(worst['back'], float((e / b).max()))
        assert np.all(e <= b), f'{label}: frame {k}: bead positions against the back-transform, err / bound {float((e / b).max()):.3f}'
    for k in range(len(frames_x) - 1):
        xi = None if sigma is None else _np(noises[k])

        def fn(**a):
            return pr.full_step(a['u'], a['w'], a['F0'], a['F1'], C, a['tab'], a['hk'], a['m'], a.get('sigma'), a.get('xi'))
        rows = dict(u=_np(frames_u[k]), w=_np(frames_w[k]), F0=F[k], F1=F[k + 1], hk=hk, m=m)
        if sigma is not None:
            rows.update(sigma=sigma, xi=xi)
        ref = pr.flat(fn, ptr, P, rows, dict(tab=tab))
        for name, got, extra in (('u', frames_u[k + 1], 0.0), ('w', frames_w[k + 1], force_term), ('x', frames_x[k + 1], 0.0)):
            e = np.abs(_np(got).astype(np.float64) - ref[name])
            b = ref['b' + name] + pr.half_ulp32(ref[name]) + extra
            worst[name] = max(worst[name], float((e / b).max()))
            assert np.all(e <= b), f'{label}: step {k} -> {k + 1}: {name} err / bound {float((e / b).max()):.3f}'
    print(f'{label}: {len(frames_x) - 1} steps, worst err / bound ' + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()))


def run_and_check(model, z, pos, cell, batch, P, n_steps, label, seed=7, **kw):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    pi = model.path_integral(z, pos, cell, batch, P, generator=gen, **kw)
    u0, w0, x0 = pi.mode_positions, pi.mode_velocities, pi.positions
    before = model.deferred_stats()
    traj = pi.run(n_steps, record_every=1)
    after = model.deferred_stats()
    N = pi.n_atoms
    assert traj.step.tolist() == list(range(1, n_steps + 1)) and traj.pos.shape == (n_steps, N, 3) and N == P * pos.shape[0]
    regen = torch.Generator(device='cuda').manual_seed(seed)
    torch.randn((N, 3), generator=regen, device='cuda')                                       # the initial mode velocities
    noises = [torch.randn((N, 3), generator=regen, device='cuda') for _ in range(n_steps)] if pi._sigma is not None else None
    # the tables of the reference are formed HERE, from the arguments, not taken from the object under test
    from newtonnet_amd import pimd
    from newtonnet_amd.vibrations import table_masses
    G = cell.shape[0]
    T = kw['temperature']
    T = _np(T).astype(np.float64) if isinstance(T, torch.Tensor) else np.full(G, float(T))
    cf, mf, dt_fs = kw.get('centroid_friction', 0.0), kw.get('mode_friction', 1.0), kw.get('timestep', 0.25)
    ptr = np.concatenate([[0], np.cumsum(np.repeat(np.bincount(_np(batch), minlength=G), P))]).astype(np.int32)
    mol = np.repeat(np.arange(G * P), np.diff(ptr))
    m = _np(table_masses(pi.z)).astype(np.float64)
    tab, one_minus = pimd.mode_tables(P, T, dt_fs, cf, mf)
    hk = (0.5 * dt_fs * pimd.FS / m).astype(np.float32)
    sigma = None
    if cf > 0.0 or (mf > 0.0 and P > 1):
        sigma = np.sqrt(one_minus.reshape(-1)[mol] * K_B * (P * T)[mol // P] / m).astype(np.float32)
    C = pimd.transform_matrix(P).astype(np.float32)
    assert np.array_equal(ptr, _np(pi._mol_ptr)) and (sigma is None) == (pi._sigma is None)
    check_stepwise(model, pi.z, pi.cell, pi.batch, ptr, P, C, tab.reshape(G * P, 5), hk, m.astype(np.float32), sigma,
                   [u0] + list(traj.mode_pos), [w0] + list(traj.mode_vel), [x0] + list(traj.pos), noises, label)
    if pi._sigma is None:
        assert torch.equal(regen.get_state(), gen.get_state())                               # no noise was drawn
    return pi, traj, before, after


@pytest.mark.parametrize('case, P, scheme', [('mixed_rand', 4, 'pile'), ('aspirin8_rand', 8, 'trpmd'), ('aspirin8_rand', 3, 'rpmd')])
def test_every_recorded_step_follows_from_the_one_before(case, P, scheme):
    z, pos, cell, batch, _ = util.case_inputs(case, torch.float32)
    z, pos, cell, batch = cuda(z, pos, cell, batch)
    model = make_model(util.load_state('rand'))
    G = cell.shape[0]
    kw = dict(pile=dict(temperature=torch.linspace(200.0, 400.0, G).cuda(), centroid_friction=0.01, mode_friction=1.0),
              trpmd=dict(temperature=300.0, centroid_friction=0.0, mode_friction=1.0),
              rpmd=dict(temperature=300.0, centroid_friction=0.0, mode_friction=0.0))[scheme]
    pi, traj, before, after = run_and_check(model, z, pos, cell, batch, P, 12, f'{case} P = {P} {scheme}', **kw)
    assert (pi._sigma is None) == (scheme == 'rpmd')
    assert after['repeats_needed'] == before['repeats_needed']
    assert after['deferred_calls'] - before['deferred_calls'] >= 12 - 2
    for name in ('potential', 'kinetic_virial', 'kinetic_primitive', 'ring_polymer_energy'):
        assert getattr(traj, name).shape == (12, G) and torch.isfinite(getattr(traj, name)).all()
    assert not hasattr(traj, 'total_energy') and not hasattr(traj, 'temperature')          # meaningless per slot: not offered


# ---- 5. bitwise properties ------------------------------------------------------------------------------------------------------

FIELDS = ('pos', 'vel', 'mode_pos', 'mode_vel', 'potential_energy', 'kinetic_energy', 'potential', 'kinetic_virial', 'kinetic_primitive',
          'ring_polymer_energy', 'centroid', 'radius_of_gyration')


def test_bitwise_properties():
    z, pos, cell, batch, _ = util.case_inputs('mixed_rand', torch.float32)
    z, pos, cell, batch = cuda(z, pos, cell, batch)
    keep = [t.clone() for t in (z, pos, cell, batch)]
    model = make_model(util.load_state('rand'))
    ladder = torch.linspace(200.0, 400.0, cell.shape[0]).cuda()
    keep_ladder = ladder.clone()

    def make(seed):
        gen = torch.Generator(device='cuda').manual_seed(seed)
        return model.path_integral(z, pos, cell, batch, 4, ladder, centroid_friction=0.01, generator=gen)
    before = model.deferred_stats()
    a, b, c = make(7).run(12, 1), make(7).run(12, 1), make(8).run(12, 1)
    after = model.deferred_stats()
    assert after['repeats_needed'] == before['repeats_needed'] and after['deferred_calls'] - before['deferred_calls'] >= 3 * (12 - 2)
    for name in FIELDS + ('step',):
        assert torch.equal(getattr(a, name), getattr(b, name)), name                       # the same seed twice
    assert not torch.equal(a.pos, c.pos)
    e4 = make(7).run(12, 4)
    assert e4.step.tolist() == [4, 8, 12]
    for name in FIELDS:
        assert torch.equal(getattr(e4, name), getattr(a, name)[3::4]), name                 # record_every changes no bit
    d = make(7)
    d.run(7, 3)
    t = d.run(5, 0)
    assert t.step.tolist() == [12] and d.step_count == 12
    for name in FIELDS:
        assert torch.equal(getattr(t, name)[0], getattr(a, name)[-1]), name                 # run(7); run(5) is run(12)
    for x, k in zip((z, pos, cell, batch, ladder), keep + [keep_ladder]):
        assert torch.equal(x, k)
    # a restart from the recorded bead positions and velocities is accepted, and starts where the record stands (to rounding)
    r = model.path_integral(z, pos, cell, batch, 4, ladder, centroid_friction=0.01, bead_positions=a.pos[-1], bead_velocities=a.vel[-1])
    assert float((r.mode_positions - a.mode_pos[-1]).abs().max()) <= 1e-5 and float((r.mode_velocities - a.mode_vel[-1]).abs().max()) <= 1e-6


# ---- 6. RPMD conserves the ring-polymer energy ----------------------------------------------------------------------------------

def test_rpmd_conserves_the_ring_polymer_energy_against_a_host_fp64_integrator():
    """2 aspirins x 4 beads, seeded weights, table masses, 300 K, 0.25 fs, 200 steps, both frictions 0.  Per system,
    max_n |E_rp(n) - E_rp(0)| <= (a) the same figure of a host fp64 loop of the same scheme driven by model() forces from the same
    start + (b) the first-order cost of the fp32 state, sum over steps and rows of |dE/du_k| ulp(u_k) / 2 + m w_k^2 2^-24 with
    dE/du_k = m omega_k^2 u_k - f_k, + (c) 2 P util.energy_tol(E); and the kinetic energy must move by at least 10 x that bound."""
    from newtonnet_amd import pimd
    n_steps, G, P, n = 200, 2, 4, 21
    z, pos, cell, batch = _bench().synthetic_aspirin(G, 0, 'cuda')
    model = make_model(util.load_state('rand'))
    gen = torch.Generator(device='cuda').manual_seed(11)
    pi = model.path_integral(z, pos, cell, batch, P, 300.0, timestep=0.25, centroid_friction=0.0, mode_friction=0.0, generator=gen)
    u0, w0 = _np(pi.mode_positions).astype(np.float64), _np(pi.mode_velocities).astype(np.float64)
    first = pi.run(0)
    traj = pi.run(n_steps, record_every=1)
    e_rp = np.concatenate([_np(first.ring_polymer_energy), _np(traj.ring_polymer_energy)])
    ke = np.concatenate([_np(first.kinetic_energy), _np(traj.kinetic_energy)]).astype(np.float64).reshape(-1, G, P).sum(2)
    drift = np.abs(e_rp - e_rp[0]).max(axis=0)
    m = _np(pi.masses).astype(np.float64).reshape(G, P, n)
    C = pimd.transform_matrix(P)
    tab = pimd.mode_tables(P, [300.0] * G, 0.25, 0.0, 0.0, dtype=np.float64)[0]            # [G, P, 5]
    a, b, d, hw2 = (tab[:, :, j, None, None] for j in (0, 1, 2, 4))
    hk = 0.5 * 0.25 * pimd.FS / m[..., None]

    def evaluate(u):
        x = np.einsum('ks,gkic->gsic', C, u)
        f, e = _forces(model, pi.z, torch.from_numpy(x.reshape(-1, 3)).float().cuda(), pi.cell, pi.batch)
        F = _np(f).astype(np.float64).reshape(G, P, n, 3)
        return np.einsum('ks,gsic->gkic', C, F), _np(e).astype(np.float64).reshape(G, P)

    def energy(u, w, e):
        return (0.5 * m[..., None] * w * w).sum((1, 2, 3)) + (m[..., None] * hw2 * u * u).sum((1, 2, 3)) + e.sum(1)
    # (a) the host fp64 loop
    u, w = u0.reshape(G, P, n, 3), w0.reshape(G, P, n, 3)
    f, e = evaluate(u)
    host = [energy(u, w, e)]
    for _ in range(n_steps):
        w = w + hk * f
        u, w = a * u + b * w, d * u + a * w
        u, w = a * u + b * w, d * u + a * w
        f, e = evaluate(u)
        w = w + hk * f
        host.append(energy(u, w, e))
    host = np.asarray(host)
    ta = np.abs(host - host[0]).max(axis=0)
    # (b) from the recorded trajectory
    tb = np.zeros(G)
    C32 = _np(pi._ctab).astype(np.float64)
    for k in range(n_steps):
        F = _np(_forces(model, pi.z, traj.pos[k], pi.cell, pi.batch)[0]).astype(np.float64).reshape(G, P, n, 3)
        fk = np.einsum('ks,gsic->gkic', C32, F)
        uk, wk = _np(traj.mode_pos[k]).reshape(G, P, n, 3), _np(traj.mode_vel[k]).astype(np.float64).reshape(G, P, n, 3)
        grad = np.abs(2.0 * m[..., None] * hw2 * uk.astype(np.float64) - fk)
        tb += (grad * pr.half_ulp32(uk)).sum((1, 2, 3)) + (m[..., None] * wk * wk).sum((1, 2, 3)) * pr.EPS32
    tc = 2.0 * P * util.energy_tol(_np(first.potential_energy).astype(np.float64).reshape(G, P)[:, 0])
    bound = ta + tb + tc
    swing = ke.max(axis=0) - ke.min(axis=0)
    print(f'ring-polymer energy over {n_steps} steps: drift {drift} eV, bound {bound} = host fp64 {ta} + fp32 state {tb} + energy ulps {tc}; '
          f'drift / bound {drift / bound}; kinetic energy swing {swing} eV = {swing / bound} x bound; E_rp(0) {e_rp[0]}')
    assert np.all(drift <= bound), f'drift / bound {drift / bound}'
    assert np.all(swing >= 10.0 * bound), f'kinetic energy swing / bound {swing / bound}: the test has no power'


# ---- 7. the estimators against the recorded frames ------------------------------------------------------------------------------

def test_estimators_against_the_recorded_frames():
    G, P, n, T = 3, 4, 21, 250.0
    z, pos, cell, batch = _bench().synthetic_aspirin(G, 2, 'cuda')
    model = make_model(util.load_state('rand'))
    gen = torch.Generator(device='cuda').manual_seed(3)
    pi = model.path_integral(z, pos, cell, batch, P, T, centroid_friction=0.01, generator=gen)
    traj = pi.run(30, record_every=10)
    Rec = 3
    m = _np(pi.masses).astype(np.float64).reshape(G, P, n)
    C = _np(pi._ctab).astype(np.float64)
    hw2 = _np(pi._mode_tab).astype(np.float64).reshape(G, P, 5)[:, :, 4]
    for r in range(Rec):
        F = _np(_forces(model, pi.z, traj.pos[r], pi.cell, pi.batch)[0]).astype(np.float64).reshape(G, P, n, 3)
        f = np.einsum('ks,gsic->gkic', C, F)
        u = _np(traj.mode_pos[r]).astype(np.float64).reshape(G, P, n, 3)
        x = _np(traj.pos[r]).astype(np.float64).reshape(G, P, n, 3)
        e = _np(traj.potential_energy[r]).astype(np.float64).reshape(G, P)
        np.testing.assert_allclose(_np(traj.potential[r]), e.mean(1), rtol=1e-5)
        virial = 1.5 * n * K_B * T - (u[:, 1:] * f[:, 1:]).sum((1, 2, 3)) / (2.0 * P)
        np.testing.assert_allclose(_np(traj.kinetic_virial[r]), virial, rtol=1e-5)
        spring = (m[..., None] * hw2[:, :, None, None] * u * u).sum((1, 2, 3))
        np.testing.assert_allclose(_np(traj.kinetic_primitive[r]), 1.5 * n * P * K_B * T - spring / P, rtol=1e-5)
        c = x.mean(1)
        np.testing.assert_allclose(_np(traj.centroid[r]).reshape(G, n, 3), c, rtol=1e-5, atol=1e-6)
        rg = np.sqrt(((x - c[:, None]) ** 2).sum(3).mean(1))
        np.testing.assert_allclose(_np(traj.radius_of_gyration[r]).reshape(G, n), rg, rtol=1e-5)
        assert rg.min() > 0.0
        w = _np(traj.mode_vel[r]).astype(np.float64).reshape(G, P, n, 3)
        kinetic = (0.5 * m[..., None] * w * w).sum((1, 2, 3))
        np.testing.assert_allclose(_np(traj.ring_polymer_energy[r]), kinetic + spring + e.sum(1), rtol=1e-5)
        v = np.einsum('ks,gkic->gsic', C, w)
        np.testing.assert_allclose(_np(traj.vel[r]).reshape(G, P, n, 3), v, rtol=1e-5, atol=1e-7)
        print(f'frame {r}: potential {e.mean(1)}, centroid virial {virial}, primitive {1.5 * n * P * K_B * T - spring / P} eV; '
              f'largest radius of gyration {rg.max():.4f} A')


# ---- 8. the calculator ----------------------------------------------------------------------------------------------------------

class PeriodicAtoms:
    def __init__(self, numbers, positions, cell):
        self.numbers, self.positions, self.cell = np.asarray(numbers), np.asarray(positions, dtype=np.float64), np.asarray(cell, dtype=np.float64)

    def __len__(self):
        return len(self.numbers)

    def get_atomic_numbers(self):
        return self.numbers

    def get_positions(self, wrap=False):
        return self.positions

    def get_cell(self):
        return self.cell

    def get_pbc(self):
        return np.ones(3, dtype=bool)


def test_calculator_form():
    from newtonnet_amd import pimd
    from newtonnet_amd.utils import MLAseCalculator
    from newtonnet_amd.vibrations import table_masses
    from tests.test_hip_md import FakeAtoms
    z, pos, _, _ = _bench().synthetic_aspirin(3, 1, 'cpu')
    model = make_model(util.load_state('rand'))
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda')
    frames = [FakeAtoms(z[:21].numpy(), pos[21 * k:21 * (k + 1)].numpy()) for k in range(3)]
    keep = [f.positions.copy() for f in frames]
    P = 4
    out = calc.run_pimd(frames, P, 300.0, 6, centroid_friction=0.01, record_every=4, seed=5)
    assert out['step'].tolist() == [4, 6] and out['step'].dtype == np.int64
    for k in ('positions', 'velocities', 'mode_positions', 'mode_velocities'):
        assert out[k].shape == (2, 3, P, 21, 3) and out[k].dtype == np.float32, k
    assert out['energy'].shape == (2, 3, P) and out['centroid'].shape == (2, 3, 21, 3) and out['radius_of_gyration'].shape == (2, 3, 21)
    for k in ('potential', 'kinetic_virial', 'kinetic_primitive', 'ring_polymer_energy'):
        assert out[k].shape == (2, 3), k
    again = calc.run_pimd(frames, P, 300.0, 6, centroid_friction=0.01, record_every=4, seed=5)
    other = calc.run_pimd(frames, P, 300.0, 6, centroid_friction=0.01, record_every=4, seed=6)
    assert all(np.array_equal(out[k], again[k]) for k in out) and not np.array_equal(out['positions'], other['positions'])
    assert all(np.array_equal(f.positions, k) for f, k in zip(frames, keep))
    one = calc.run_pimd(frames[0], P, 300.0, 3)                                            # a single structure drops the G axis
    assert one['positions'].shape == (1, P, 21, 3) and one['energy'].shape == (1, P) and one['potential'].shape == (1,)
    assert one['centroid'].shape == (1, 21, 3) and one['radius_of_gyration'].shape == (1, 21)
    # masses of the object are used: a heavier ring spreads less in the same time
    heavy = calc.run_pimd(FakeAtoms(z[:21].numpy(), pos[:21].numpy(), masses=np.full(21, 100.0)), P, 300.0, 3, seed=1)
    light = calc.run_pimd(FakeAtoms(z[:21].numpy(), pos[:21].numpy(), masses=np.full(21, 1.0)), P, 300.0, 3, seed=1)
    assert heavy['radius_of_gyration'].max() < light['radius_of_gyration'].min()
    # one periodic structure, RPMD: the positions stay unwrapped and every step follows from the one before
    zp, pp, cp, bp, _ = util.case_inputs('pbc_batch2_rand', torch.float32)
    sel = bp == 1
    n = int(sel.sum())
    atoms = PeriodicAtoms(zp[sel].numpy(), pp[sel].numpy(), cp[1].numpy())
    T, dt, P = 300.0, 0.25, 2
    per = calc.run_pimd(atoms, P, T, 5, timestep=dt, centroid_friction=0.0, mode_friction=0.0, record_every=1, seed=2)
    assert per['positions'].shape == (5, P, n, 3)
    assert np.abs(np.diff(per['positions'], axis=0)).max() < 0.05                          # no jump by a cell vector
    zr = zp[sel].repeat(P).cuda()
    m = _np(table_masses(zr.cpu())).astype(np.float64)
    tab = pimd.mode_tables(P, [T], dt, 0.0, 0.0)[0].reshape(P, 5)
    hk = (0.5 * dt * pimd.FS / m).astype(np.float32)
    ptr = (np.arange(P + 1) * n).astype(np.int32)
    dev = [[torch.from_numpy(np.ascontiguousarray(per[k][r])).reshape(-1, 3).cuda() for r in range(5)]
           for k in ('mode_positions', 'mode_velocities', 'positions')]
    check_stepwise(model, zr, cp[1:2].repeat(P, 1, 1).cuda(), torch.arange(P).repeat_interleave(n).cuda(), ptr, P,
                   pimd.transform_matrix(P).astype(np.float32), tab, hk, m.astype(np.float32), None, dev[0], dev[1], dev[2], None,
                   'periodic, calculator')
