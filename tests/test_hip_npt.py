"""Constant-pressure batched molecular dynamics on the HIP path (newtonnet_amd/npt.py, csrc/npt.hip).

Kernels alone: nnhip_npt_barostat and nnhip_npt_step on random inputs against their fp64 restatement on the SAME fp32 inputs
(tests/npt_ref.py), every output within the derived first-order rounding bound (C_MD = 2, 2 ulp for expf and the root) plus half an
fp32 ulp of the stored value; the tests print err / bound.  Driver: every recorded step is checked ONE step at a time -- forces and
virial recomputed by the device model on the recorded positions and cell, both noises regenerated from the seed -- so no error
compounds and no chaos term has to be guessed; velocities get hk_i x util.FORCE_MAX_TOL and the virial VIRIAL_TOL on top, in case a
recomputed result took another path through the library.  Ensemble: the two kernels sample the ideal gas's volume distribution."""
import numpy as np
import pytest
import torch

from tests import md_ref as mr
from tests import npt_ref as nr
from tests import util
from tests.test_hip_hessian import cuda, make_model
from tests.test_npt_host import GAS, GAS_EXACT, gas_margin, host_gas

pytestmark = pytest.mark.gpu

K_B = 8.617333262e-5
DT = 0.5 * 0.0982269


def _np(t):
    return t.detach().cpu().numpy()


def _within(got, ref, bound, what, worst):
    """|got - ref| <= bound + half an ulp of the stored value, everywhere; notes the worst ratio"""
    ref, bound = np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64) + mr.half_ulp32(ref)
    err = np.abs(np.asarray(got).astype(np.float64) - ref)
    ratio = float((err / bound).max()) if err.size else 0.0
    worst[what] = max(worst.get(what, 0.0), ratio)
    assert np.all(err <= bound), f'{what}: err / bound {ratio:.3f}'


# ---- 1. the barostat kernel against fp64 on the same inputs -------------------------------------------------------------------

SIZES = (0, 1, 255, 257, 600)       # empty; below, straddling and above one pass of the 256 threads


def _barostat_inputs(triclinic, seed):
    rng = np.random.default_rng(seed)
    f32 = np.float32
    B, N = len(SIZES), sum(SIZES)
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    m = rng.choice(np.array([1.008, 12.011, 14.007, 15.999], dtype=f32), N)
    v = (rng.standard_normal((N, 3)) * np.sqrt(K_B * 300.0 / m.astype(np.float64))[:, None]).astype(f32)
    F = rng.uniform(-5, 5, (N, 3)).astype(f32)
    hk = (0.5 * DT / m.astype(np.float64)).astype(f32)
    cell = np.zeros((B, 3, 3))
    for b in range(B):
        cell[b] = np.diag(rng.uniform(9.0, 16.0, 3))
        if triclinic:
            cell[b] += np.tril(rng.normal(0, 2.0, (3, 3)), -1) + np.triu(rng.normal(0, 0.7, (3, 3)), 1)
    assert np.all(np.linalg.det(cell) > 500.0)
    W = rng.normal(0, 4.0, (B, 3, 3)).astype(f32)
    a = (0.18 * rng.uniform(0.5, 2.0, B)).astype(f32)
    p0 = (nr.BAR * rng.uniform(-500.0, 2000.0, B)).astype(f32)
    s2 = (2.0 * K_B * 300.0 * a.astype(np.float64)).astype(f32)
    xi = rng.standard_normal(B).astype(f32)
    return dict(ptr=ptr, m=m, v=v, F=F, hk=hk, cell=cell.astype(f32), W=W, a=a, p0=p0, s2=s2, xi=xi)


def _launch_barostat(t, with_force, with_noise, a=None, cell_out=None):
    from newtonnet_amd import hip
    B = t['cell'].shape[0]
    out = dict(cell_out=torch.full((B, 3, 3), 777.0, device='cuda') if cell_out is None else cell_out)
    for k in ('mu', 'inv_mu', 'ke', 'pressure', 'volume', 'deps'):
        out[k] = torch.full((B,), 777.0, device='cuda')
    hip.npt_barostat(t['v'], t['m'], t['ptr'], t['cell'], t['W'], t['a'] if a is None else a, t['p0'], out['cell_out'], out['mu'],
                     out['inv_mu'], out['ke'], out['pressure'], out['volume'], out['deps'],
                     force=t['F'] if with_force else None, hk=t['hk'] if with_force else None,
                     s2=t['s2'] if with_noise else None, noise=t['xi'] if with_noise else None)
    return out


@pytest.mark.parametrize('with_noise', [False, True])
@pytest.mark.parametrize('with_force', [False, True])
@pytest.mark.parametrize('triclinic', [False, True])
def test_barostat_against_fp64_on_the_same_inputs(triclinic, with_force, with_noise):
    d = _barostat_inputs(triclinic, 40 + triclinic)
    t = {k: torch.from_numpy(x).cuda() for k, x in d.items()}
    keep = {k: x.clone() for k, x in t.items()}
    got = _launch_barostat(t, with_force, with_noise)
    again = _launch_barostat(t, with_force, with_noise)
    for k in got:
        assert torch.equal(got[k], again[k]), f'{k}: two launches differ'              # bitwise repeatable
    assert all(torch.equal(t[k], keep[k]) for k in t)                                   # inputs (the velocities too) intact
    ref = nr.barostat(d['v'], d['m'], d['ptr'], d['cell'], d['W'], d['a'], d['p0'], F=d['F'] if with_force else None,
                      hk=d['hk'] if with_force else None, s2=d['s2'] if with_noise else None, xi=d['xi'] if with_noise else None)
    worst = {}
    for k in ('ke', 'volume', 'pressure', 'deps', 'mu', 'inv_mu', 'cell_out'):
        _within(_np(got[k]), ref[k], ref['b' + k], k, worst)
    assert float(got['ke'][0]) == 0.0                                                    # the empty system
    assert np.all(np.abs(ref['deps']) > 1e-5), 'the set-up leaves the rescale at rounding level'
    print(f'npt_barostat triclinic {triclinic}, force {with_force}, noise {with_noise}: worst err / bound '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f'; |deps| {np.abs(ref["deps"]).min():.1e} .. {np.abs(ref["deps"]).max():.1e}')
    if not with_noise:
        # a = 0 without noise: mu = inv_mu = 1 exactly, deps = +0, the cell bit for bit; K, P and V are still recorded
        off = _launch_barostat(t, with_force, False, a=torch.zeros_like(t['a']))
        assert torch.all(off['mu'] == 1.0) and torch.all(off['inv_mu'] == 1.0) and not off['deps'].any()
        assert torch.equal(off['cell_out'].view(torch.int32), t['cell'].view(torch.int32))
        for k in ('ke', 'pressure', 'volume'):
            assert torch.equal(off[k], got[k])


@pytest.mark.parametrize('with_force', [False, True])
def test_barostat_kinetic_energy_is_the_step_kernels(with_force):
    """Five systems of one atom each: the barostat's tree sum is 0 + ke_i plus zeros, exact, so ke[b] must carry the bits of
    nnhip_md_step's ke_out[b] on the same vel, hk, force and mass (no pending force = a zero force in md_step: fma(hk, 0, v) = v)."""
    from newtonnet_amd import hip
    rng = np.random.default_rng(77)
    f32, B = np.float32, 5
    m = np.array([1.008, 12.011, 14.007, 15.999, 32.06], dtype=f32)
    v = (rng.standard_normal((B, 3)) * np.sqrt(K_B * 300.0 / m.astype(np.float64))[:, None]).astype(f32)
    d = dict(ptr=np.arange(B + 1, dtype=np.int32), m=m, v=v, F=rng.uniform(-5, 5, (B, 3)).astype(f32),
             hk=(0.5 * DT / m.astype(np.float64)).astype(f32), cell=np.tile(np.diag([10.0, 11.0, 12.0]).astype(f32), (B, 1, 1)),
             W=rng.normal(0, 4.0, (B, 3, 3)).astype(f32), a=np.full(B, 0.2, dtype=f32), p0=np.zeros(B, dtype=f32),
             s2=np.zeros(B, dtype=f32), xi=np.zeros(B, dtype=f32))
    t = {k: torch.from_numpy(x).cuda() for k, x in d.items()}
    ke = _launch_barostat(t, with_force, False)['ke']
    vel, ke_out = t['v'].clone(), torch.full((B,), 777.0, device='cuda')
    hip.md_step(None, vel, t['F'] if with_force else torch.zeros_like(t['F']), t['hk'], 0.5 * DT, 1.0, hip.MD_FINISH, mass=t['m'],
                ke_out=ke_out)
    assert torch.equal(vel, t['v']) != with_force and torch.all(ke_out > 0)            # the kick was applied iff a force is pending
    assert torch.equal(ke.view(torch.int32), ke_out.view(torch.int32)), f'ke {ke.tolist()} is not md_step ke_out {ke_out.tolist()}'


# ---- 2. the step kernel against fp64, and against md_step's bits ---------------------------------------------------------------

def _step_inputs(N, seed, n_mol=5):
    rng = np.random.default_rng(seed)
    f32 = np.float32
    x, v, F = (rng.uniform(-8, 8, (N, 3)).astype(f32), rng.uniform(-0.2, 0.2, (N, 3)).astype(f32), rng.uniform(-5, 5, (N, 3)).astype(f32))
    m = rng.choice(np.array([1.008, 12.011, 14.007, 15.999], dtype=f32), N)
    hk, sigma = (0.5 * DT / m.astype(np.float64)).astype(f32), np.sqrt(0.02 * K_B * 300.0 / m.astype(np.float64)).astype(f32)
    xi = rng.standard_normal((N, 3)).astype(f32)
    mol = np.sort(rng.integers(0, n_mol, N)).astype(np.int32)                 # atoms spread over systems with different mu
    e = rng.uniform(-1e-3, 1e-3, n_mol)
    mu, inv_mu = np.exp(e).astype(f32), np.exp(-e).astype(f32)
    return dict(x=x, v=v, F=F, m=m, hk=hk, sigma=sigma, xi=xi, mol=mol, mu=mu, inv_mu=inv_mu, dth=float(f32(0.5 * DT)),
                c1=float(f32(np.exp(-0.01))))


STRIDE = 2048 * 256                 # atoms one pass of the step kernel's grid covers


@pytest.mark.parametrize('with_noise', [False, True])
@pytest.mark.parametrize('flags', [mr.BEGIN, mr.FINISH, mr.BEGIN | mr.FINISH])
@pytest.mark.parametrize('N', [1, 255, 257, STRIDE + 300])
def test_npt_step_against_fp64_and_md_step_bits(N, flags, with_noise):
    from newtonnet_amd import hip
    d = _step_inputs(N, 200 + N % 1000)
    t = {k: torch.from_numpy(d[k]).cuda() for k in ('x', 'v', 'F', 'm', 'hk', 'sigma', 'xi', 'mol', 'mu', 'inv_mu')}
    SENT = 777.0
    begin, finish = bool(flags & mr.BEGIN), bool(flags & mr.FINISH)

    def launch(step, **kw):
        pos_out, ke, vel = torch.full((N, 3), SENT, device='cuda'), torch.full((N,), SENT, device='cuda'), t['v'].clone()
        step(t['x'] if begin else None, vel, t['F'], t['hk'], d['dth'], d['c1'], flags, pos_out=pos_out if begin else None,
             mass=t['m'], sigma=t['sigma'] if with_noise else None, noise=t['xi'] if with_noise else None,
             ke_out=ke if finish else None, **kw)
        return pos_out, vel, ke
    pos_out, vel, ke = launch(hip.npt_step, mu=t['mu'], inv_mu=t['inv_mu'], mol_of_atom=t['mol'])
    ref = nr.npt_step(flags, d['x'], d['v'], d['F'], d['hk'], d['mu'], d['inv_mu'], d['mol'], d['m'], d['sigma'] if with_noise else None,
                      d['xi'] if with_noise else None, d['c1'], d['dth'])
    assert torch.equal(t['x'], torch.from_numpy(d['x']).cuda()) and torch.equal(t['F'], torch.from_numpy(d['F']).cuda())   # inputs intact
    worst = {}
    _within(_np(vel), ref['v'], ref['bv'], 'v', worst)
    if begin:
        _within(_np(pos_out), ref['x'], ref['bx'], 'x', worst)
        # the rescale is far above the bound: without it the positions would miss by |mu - 1| |x|
        moved = np.abs((d['mu'].astype(np.float64)[d['mol']] - 1.0)[:, None] * d['x'])
        assert (moved > 10.0 * (ref['bx'] + mr.half_ulp32(ref['x']))).mean() > 0.5
    else:
        assert torch.all(pos_out == SENT)
    if finish:
        _within(_np(ke), ref['ke'], ref['bke'], 'ke', worst)
    else:
        assert torch.all(ke == SENT)
    print(f'npt_step N = {N}, flags = {flags}, noise {with_noise}: worst err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    # every mu = inv_mu = 1: nnhip_md_step's bits
    ones = torch.ones(5, device='cuda')
    a = launch(hip.npt_step, mu=ones, inv_mu=ones, mol_of_atom=t['mol'])
    b = launch(hip.md_step)
    for name, p, q in zip(('pos_out', 'vel', 'ke'), a, b):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), f'{name}: not the bits of nnhip_md_step'


# ---- 3. refusals, with nothing written -------------------------------------------------------------------------------------------

def test_refusals_write_nothing():
    from newtonnet_amd import hip
    d = _step_inputs(65, 5)
    t = {k: torch.from_numpy(d[k]).cuda() for k in ('x', 'v', 'F', 'm', 'hk', 'sigma', 'xi', 'mol', 'mu', 'inv_mu')}
    x0, v0 = t['x'].clone(), t['v'].clone()
    out = torch.full((65, 3), 777.0, device='cuda')
    base = dict(mu=t['mu'], inv_mu=t['inv_mu'], mol_of_atom=t['mol'])
    with pytest.raises(hip.HipLibraryError, match='alias'):
        hip.npt_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 1.0, mr.BEGIN, pos_out=t['x'], **base)
    with pytest.raises(hip.HipLibraryError, match='alias'):          # an overlapping view is an alias too
        flat = torch.zeros(3 * 65 + 3, device='cuda')
        hip.npt_step(flat[:195].view(65, 3), t['v'], t['F'], t['hk'], d['dth'], 1.0, mr.BEGIN, pos_out=flat[3:].view(65, 3), **base)
    with pytest.raises(hip.HipLibraryError, match='sigma and noise'):
        hip.npt_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 0.99, mr.BEGIN, pos_out=out, sigma=t['sigma'], **base)
    with pytest.raises(hip.HipLibraryError, match='sigma and noise'):
        hip.npt_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 0.99, mr.BEGIN, pos_out=out, noise=t['xi'], **base)
    with pytest.raises(hip.HipLibraryError, match='flags'):
        hip.npt_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 1.0, 0, pos_out=out, **base)
    with pytest.raises(hip.HipLibraryError):                         # begin without an output
        hip.npt_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 1.0, mr.BEGIN, **base)
    with pytest.raises(hip.HipLibraryError, match='mu'):             # begin without the scale factors / the atom -> system map
        hip.npt_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 1.0, mr.BEGIN, pos_out=out)
    with pytest.raises(hip.HipLibraryError, match='mol_of_atom'):
        hip.npt_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 1.0, mr.BEGIN, pos_out=out, mu=t['mu'], inv_mu=t['inv_mu'])
    with pytest.raises(hip.HipLibraryError, match='ke_out'):         # kinetic energies without finish
        hip.npt_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 1.0, mr.BEGIN, pos_out=out, mass=t['m'],
                     ke_out=torch.zeros(65, device='cuda'), **base)
    torch.cuda.synchronize()
    assert torch.equal(t['x'], x0) and torch.equal(t['v'], v0) and torch.all(out == 777.0)
    empty = torch.zeros(0, 3, device='cuda')
    hip.npt_step(empty, empty.clone(), empty, torch.zeros(0, device='cuda'), d['dth'], 1.0, mr.BEGIN, pos_out=empty.clone(),
                 mu=t['mu'], inv_mu=t['inv_mu'], mol_of_atom=torch.zeros(0, dtype=torch.int32, device='cuda'))      # no-op
    # the barostat
    b = _barostat_inputs(True, 9)
    tb = {k: torch.from_numpy(x).cuda() for k, x in b.items()}
    keep = tb['cell'].clone()
    B = keep.shape[0]
    with pytest.raises(hip.HipLibraryError, match='alias'):
        _launch_barostat(tb, True, True, cell_out=tb['cell'])
    flat = torch.cat([tb['cell'].reshape(-1), torch.zeros(9, device='cuda')])
    tb2 = dict(tb, cell=flat[:9 * B].view(B, 3, 3))
    with pytest.raises(hip.HipLibraryError, match='alias'):          # an overlapping view
        _launch_barostat(tb2, True, True, cell_out=flat[9:].view(B, 3, 3))
    recs = [torch.full((B,), 777.0, device='cuda') for _ in range(6)]
    cell_out = torch.full((B, 3, 3), 777.0, device='cuda')
    with pytest.raises(hip.HipLibraryError, match='s2 and noise'):
        hip.npt_barostat(tb['v'], tb['m'], tb['ptr'], tb['cell'], tb['W'], tb['a'], tb['p0'], cell_out, *recs, s2=tb['s2'])
    with pytest.raises(hip.HipLibraryError, match='s2 and noise'):
        hip.npt_barostat(tb['v'], tb['m'], tb['ptr'], tb['cell'], tb['W'], tb['a'], tb['p0'], cell_out, *recs, noise=tb['xi'])
    with pytest.raises(hip.HipLibraryError, match='hk'):             # a pending force without its hk
        hip.npt_barostat(tb['v'], tb['m'], tb['ptr'], tb['cell'], tb['W'], tb['a'], tb['p0'], cell_out, *recs, force=tb['F'])
    lib = hip.lib()
    null_virial = lib.nnhip_npt_barostat(hip._ptr(tb['v']), None, None, hip._ptr(tb['m']), hip._ptr(tb['ptr']), B, tb['v'].shape[0],
                                         hip._ptr(tb['cell']), None, hip._ptr(tb['a']), hip._ptr(tb['p0']), None, None,
                                         hip._ptr(cell_out), *[hip._ptr(r) for r in recs], hip._stream(cell_out.device))
    assert null_virial != 0 and b'nnhip_npt_barostat' in lib.nnhip_last_error()
    torch.cuda.synchronize()
    assert torch.equal(tb['cell'], keep) and torch.all(cell_out == 777.0) and all(torch.all(r == 777.0) for r in recs)
    # wrappers: outputs that a copy would take away
    with pytest.raises(ValueError, match='cell_out'):
        hip.npt_barostat(tb['v'], tb['m'], tb['ptr'], tb['cell'], tb['W'], tb['a'], tb['p0'], cell_out.double(), *recs)
    with pytest.raises(ValueError, match='mol_of_atom'):
        hip.npt_step(t['x'], t['v'], t['F'], t['hk'], d['dth'], 1.0, mr.BEGIN, pos_out=out, mu=t['mu'], inv_mu=t['inv_mu'],
                     mol_of_atom=t['mol'].long())


# ---- 4. stepwise consistency of the driver ------------------------------------------------------------------------------------

VIRIAL_TOL = 2e-5          # x max(1, |W|): the tolerance tests/test_hip_parity.py::test_virial_and_stress holds the virial head to


def _periodic_case(name):
    if name == 'triclinic64':
        c = util.load_npz('case_virial_triclinic64.npz')
        z, batch = torch.from_numpy(c['z']).long(), torch.from_numpy(c['batch']).long()
        pos, cell = torch.from_numpy(c['pos']).float(), torch.from_numpy(c['cell']).float()
    else:
        z, pos, cell, batch, _ = util.case_inputs(name, torch.float32)
    return cuda(z, pos, cell, batch)


def _evaluate(model, z, pos, cell, batch):
    out = model(z, pos, cell, batch)
    W = out.virial if 'virial' in model.output_properties else -out.displacement_grad
    return _np(out.gradient_force.clone()), _np(W.clone())


# a = beta_T dt / tau_p = 0.18 A^3 / eV; at 100 K in these ~1400-2100 A^3 cells |d eps| per step is 1e-4 .. a few 1e-3: the
# deterministic part a |P0 - P| ~ 3e-4 (|P| ~ 2e-3 eV / A^3 with the seeded weights), the noise sqrt(2 k_B T a / V) ~ 1.2e-3
NPT_KW = dict(pressure=1.0, temperature=100.0, compressibility=4.5e-5, barostat_time=200.0, timestep=0.5)


@pytest.mark.parametrize('thermostat', ['none', 'langevin'])
@pytest.mark.parametrize('case,head', [('pbc_batch2_rand', 'virial'), ('triclinic64', 'stress')])
def test_every_recorded_step_follows_from_the_one_before(case, head, thermostat):
    n_steps, seed = 40, 7
    z, pos, cell, batch = _periodic_case(case)
    model = make_model(util.load_state('rand'), props=('energy', 'gradient_force', head))
    N, B = pos.shape[0], cell.shape[0]
    kw = dict(NPT_KW, friction=0.02 if thermostat == 'langevin' else 0.0)
    if B > 1:
        kw.update(pressure=torch.tensor([1.0, 500.0]).cuda(), temperature=torch.tensor([100.0, 150.0]).cuda())
    gen = torch.Generator(device='cuda').manual_seed(seed)
    dyn = model.constant_pressure(z, pos, cell, batch, generator=gen, **kw)
    p0, v0, c0 = dyn.positions, dyn.velocities, dyn.cell
    assert torch.equal(c0, cell)
    before = model.deferred_stats()
    traj = dyn.run(n_steps, record_every=1)
    after = model.deferred_stats()
    assert traj.step.tolist() == list(range(1, n_steps + 1)) and traj.cell.shape == (n_steps, B, 3, 3)
    assert after['repeats_needed'] == before['repeats_needed']
    # the random numbers of the run, regenerated: Maxwell-Boltzmann, then per step [B] for the barostat and [N,3] for the thermostat
    regen = torch.Generator(device='cuda').manual_seed(seed)
    torch.randn((N, 3), generator=regen, device='cuda')
    xi_b, xi_n = [], []
    for _ in range(n_steps):
        xi_b.append(_np(torch.randn((B,), generator=regen, device='cuda')))
        xi_n.append(_np(torch.randn((N, 3), generator=regen, device='cuda')) if thermostat == 'langevin' else None)
    frames = [(p0, v0, c0)] + [(traj.pos[k], traj.vel[k], traj.cell[k]) for k in range(n_steps)]
    FW = [_evaluate(model, z, p, c, batch) for p, _, c in frames]
    hk, m, ptr, mol = _np(dyn._hk), _np(dyn.masses), _np(dyn._mol_ptr), _np(batch)
    a, p0_, s2 = _np(dyn._a), _np(dyn._p0), _np(dyn._s2)
    sigma = None if dyn._sigma is None else _np(dyn._sigma)
    worst, deps = {}, []
    for k in range(n_steps):
        x, v, c = (_np(t) for t in frames[k])
        dw = VIRIAL_TOL * max(1.0, float(np.abs(FW[k][1]).max()))
        ref = nr.full_step(x, v, FW[k][0], FW[k + 1][0], FW[k][1], c, hk, m, ptr, mol, a, p0_, s2=s2, xi_b=xi_b[k], sigma=sigma,
                           xi=xi_n[k], c1=dyn._c1, dth=dyn._dth, dw_in=dw)
        deps.append(ref['baro']['deps'])
        _within(_np(frames[k + 1][0]), ref['x'], ref['bx'], 'positions', worst)
        _within(_np(frames[k + 1][1]), ref['v'], ref['bv'] + hk.astype(np.float64)[:, None] * util.FORCE_MAX_TOL, 'velocities', worst)
        _within(_np(frames[k + 1][2]), ref['cell'], ref['bcell'], 'cell', worst)
        if k > 0:        # the records of frame k are the barostat's own figures of that state; in bar: a product with fl32(1 / BAR),
            # two more roundings (the constant's and the product's)
            _within(_np(traj.volume[k - 1]), ref['baro']['volume'], ref['baro']['bvolume'], 'volume', worst)
            P = ref['baro']['pressure'] / nr.BAR
            _within(_np(traj.pressure[k - 1]), P, ref['baro']['bpressure'] / nr.BAR + 2.0 * nr.EPS32 * np.abs(P), 'pressure', worst)
    deps = np.abs(np.asarray(deps))
    print(f'{case} ({head} head) {thermostat}: {n_steps} steps, worst err / bound ' + ', '.join(f'{k} {v:.4f}' for k, v in worst.items())
          + f'; |d eps| per step median {np.median(deps):.1e}, max {deps.max():.1e}')
    assert 1e-4 <= np.median(deps) <= 5e-3, 'the rescale is not where the test wants it (far above rounding, far below the cell)'
    assert (dyn._sigma is None) == (thermostat == 'none')
    assert torch.isfinite(traj.total_energy).all() and bool((traj.volume > 0).all())
    np.testing.assert_allclose(_np(traj.density), _np(dyn._total_mass)[None, :] / _np(traj.volume) * 1.66053906660, rtol=1e-6)


# ---- 5. bitwise properties --------------------------------------------------------------------------------------------------------

FIELDS = ('pos', 'vel', 'potential_energy', 'kinetic_energy')
NPT_FIELDS = FIELDS + ('cell', 'volume', 'pressure')


def test_bitwise_properties():
    z, pos, cell, batch = _periodic_case('pbc_batch2_rand')
    keep = [t.clone() for t in (z, pos, cell, batch)]
    model = make_model(util.load_state('rand'), props=('energy', 'gradient_force', 'virial'))
    # no coupling, no thermostat, given velocities: Dynamics on the same inputs, bit for bit, and the cell untouched
    gen = torch.Generator(device='cuda').manual_seed(3)
    d0 = model.dynamics(z, pos, cell, batch, temperature=300.0, generator=gen)
    v0 = d0.velocities
    t0 = d0.run(20, 1)
    gen = torch.Generator(device='cuda').manual_seed(5)
    state = gen.get_state()
    d1 = model.constant_pressure(z, pos, cell, batch, 1.0, 300.0, compressibility=0.0, velocities=v0, generator=gen)
    t1 = d1.run(20, 1)
    assert torch.equal(gen.get_state(), state)                                             # no random number was drawn
    for name in FIELDS:
        assert torch.equal(getattr(t0, name), getattr(t1, name)), name
    assert torch.equal(t1.cell.view(torch.int32), cell[None].expand(20, -1, -1, -1).contiguous().view(torch.int32))
    assert torch.equal(d1.cell, cell) and torch.equal(d1.forces, d0.forces)

    def npt(seed, friction=0.02):
        gen = torch.Generator(device='cuda').manual_seed(seed)
        return model.constant_pressure(z, pos, cell, batch, generator=gen, friction=friction, **NPT_KW)
    a, b, c = npt(7).run(20, 1), npt(7).run(20, 1), npt(8).run(20, 1)
    for name in NPT_FIELDS + ('step',):
        assert torch.equal(getattr(a, name), getattr(b, name)), name                       # the same seed twice
    assert not torch.equal(a.pos, c.pos) and not torch.equal(a.cell, c.cell)
    assert not torch.equal(a.cell[-1], cell)                                               # and the cell does move
    e5 = npt(7).run(20, 5)
    assert e5.step.tolist() == [5, 10, 15, 20]
    for name in NPT_FIELDS:
        assert torch.equal(getattr(e5, name), getattr(a, name)[4::5]), name                 # record_every changes no bit
    last = npt(7).run(20, 0)
    for name in NPT_FIELDS:
        assert torch.equal(getattr(last, name)[0], getattr(a, name)[-1]), name
    # run(11); run(9) leaves the bits of run(20), whatever was recorded on the way; so without a thermostat
    for friction in (0.02, 0.0):
        whole = npt(7, friction).run(20, 0)
        d3 = npt(7, friction)
        d3.run(11, 4)
        t3 = d3.run(9, 0)
        assert t3.step.tolist() == [20] and d3.step_count == 20
        for name in NPT_FIELDS:
            assert torch.equal(getattr(t3, name), getattr(whole, name)), (friction, name)
        assert torch.equal(d3.run(0).cell[0], d3.cell) and torch.equal(d3.volume, t3.volume[0])
    for t, k in zip((z, pos, cell, batch), keep):                                          # the caller's tensors are never modified
        assert torch.equal(t, k)


# ---- 6. the shape of the cell -------------------------------------------------------------------------------------------------------

def test_the_cell_keeps_its_shape_and_fractional_coordinates_follow():
    """An isotropic rescale multiplies every entry of the cell by the same mu, one rounding per entry and step: after n steps
    cell_n = lambda cell_0 with one lambda for all nine entries within n x 4 x 2^-24 relative (2 per step would be first order for
    the ratio of two entries; 4 is the 'few'), zeros staying zeros.  Model run: 200 steps of the triclinic fixture.  Fractional
    coordinates: atoms at rest that feel no force keep them, x_n = lambda x_0 with the same lambda (the two kernels driven directly
    with a constant virial and the barostat's noise, zero forces and velocities), within the same figure."""
    from newtonnet_amd import hip
    n_steps = 200
    tol = n_steps * 4.0 * nr.EPS32
    z, pos, cell, batch = _periodic_case('triclinic64')
    model = make_model(util.load_state('rand'), props=('energy', 'gradient_force', 'virial'))
    gen = torch.Generator(device='cuda').manual_seed(1)
    dyn = model.constant_pressure(z, pos, cell, batch, generator=gen, friction=0.02, **NPT_KW)
    traj = dyn.run(n_steps, 50)
    c0 = _np(cell).astype(np.float64)[0]
    for r in range(traj.cell.shape[0]):
        c = _np(traj.cell[r]).astype(np.float64)[0]
        lam = c[0, 0] / c0[0, 0]
        assert np.all(np.abs(c - lam * c0) <= tol * np.abs(lam * c0)), f'record {r}: the cell changed its shape'
        assert abs(np.linalg.det(c) / np.linalg.det(c0) - lam ** 3) <= 3.0 * tol * lam ** 3
    assert torch.isfinite(traj.volume).all() and bool((traj.volume > 0).all()) and torch.isfinite(traj.pressure).all()
    lam = float(traj.volume[-1, 0] / traj.volume[0, 0]) ** (1.0 / 3.0)
    print(f'triclinic64, {n_steps} steps: volume {float(traj.volume[0, 0]):.1f} -> {float(traj.volume[-1, 0]):.1f} A^3')
    assert abs(lam - 1.0) > 1e-4, 'the cell did not move: the test shows nothing'
    # atoms at rest without forces: positions and cell scale together
    d = _barostat_inputs(True, 12)
    t = {k: torch.from_numpy(x).cuda() for k, x in d.items()}
    B, N = t['cell'].shape[0], t['v'].shape[0]
    mol = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), torch.tensor(SIZES)).cuda()
    x0 = torch.from_numpy(np.random.default_rng(2).uniform(-20, 20, (N, 3)).astype(np.float32)).cuda()
    xs, cells = [x0.clone(), torch.empty_like(x0)], [t['cell'].clone(), torch.empty_like(t['cell'])]
    vel, zero = torch.zeros(N, 3, device='cuda'), torch.zeros(N, 3, device='cuda')
    recs = [torch.zeros(B, device='cuda') for _ in range(6)]
    gen = torch.Generator(device='cuda').manual_seed(4)
    for k in range(n_steps):
        i, o = k % 2, 1 - k % 2
        xi = torch.randn((B,), generator=gen, device='cuda')
        hip.npt_barostat(vel, t['m'], t['ptr'], cells[i], t['W'], t['a'], t['p0'], cells[o], *recs, s2=t['s2'], noise=xi)
        hip.npt_step(xs[i], vel, zero, t['hk'], float(np.float32(0.5 * DT)), 1.0, mr.BEGIN, mu=recs[0], inv_mu=recs[1], mol_of_atom=mol,
                     pos_out=xs[o])
    assert not vel.any()
    cn, xn = _np(cells[n_steps % 2]).astype(np.float64), _np(xs[n_steps % 2]).astype(np.float64)
    c0, x0 = d['cell'].astype(np.float64), _np(x0).astype(np.float64)
    lam = cn[:, 0, 0] / c0[:, 0, 0]
    assert np.median(np.abs(lam - 1.0)) > 1e-3, 'the cells did not move: the test shows nothing'
    assert np.all(np.abs(cn - lam[:, None, None] * c0) <= tol * np.abs(lam[:, None, None] * c0))
    la = lam[_np(mol)][:, None]
    worst = float((np.abs(xn - la * x0) / (tol * np.abs(la * x0))).max())
    print(f'atoms at rest, {n_steps} steps: lambda {lam.min():.4f} .. {lam.max():.4f}; worst |x_n - lambda x_0| / ({n_steps} x 4 x 2^-24 |x|) {worst:.3f}')
    assert worst <= 1.0          # so the fractional coordinates x cell^-1 are those of the start


# ---- 7. the ideal-gas ensemble on the device ----------------------------------------------------------------------------------------

def test_ideal_gas_volume_on_the_device():
    """1024 systems x 4 atoms, zero forces and virial, the two kernels driven directly with the host test's parameters (kT = P0 = 1,
    a P0 = 0.02, Langevin, burn-in 1000 steps, ten snapshots 100 steps apart).  The mean volume is within 5 combined standard errors
    of the fp64 loop's mean (tests/npt_ref.host_loop, 4096 systems: the reference), and, separately, within the host test's margin
    (5 standard errors + a P0 <V>) of (N + 1) kT / P0 = 5."""
    from newtonnet_amd import hip
    n_sys, n = 1024, GAS['n_atoms']
    N = n_sys * n
    dev = 'cuda'
    gen = torch.Generator(device=dev).manual_seed(11)
    ptr = torch.arange(0, N + 1, n, dtype=torch.int32, device=dev)
    mol = torch.repeat_interleave(torch.arange(n_sys, dtype=torch.int32, device=dev), n)
    mass, hk = torch.ones(N, device=dev), torch.zeros(N, device=dev)
    a, p0 = torch.full((n_sys,), GAS['a'], device=dev), torch.full((n_sys,), GAS['p0'], device=dev)
    s2 = torch.full((n_sys,), 2.0 * GAS['kT'] * GAS['a'], device=dev)
    sigma = torch.full((N,), float(np.sqrt((1.0 - GAS['c1'] ** 2) * GAS['kT'])), device=dev)
    W, zero = torch.zeros(n_sys, 3, 3, device=dev), torch.zeros(N, 3, device=dev)
    L = GAS_EXACT ** (1.0 / 3.0)
    cells = [(L * torch.eye(3, device=dev)).repeat(n_sys, 1, 1).contiguous(), torch.empty(n_sys, 3, 3, device=dev)]
    xs = [L * torch.rand((N, 3), generator=gen, device=dev), torch.empty(N, 3, device=dev)]
    vel = (torch.randn((N, 3), generator=gen, device=dev) * float(np.sqrt(GAS['kT']))).contiguous()
    mu, inv_mu, ke, pressure, volume, deps = (torch.zeros(n_sys, device=dev) for _ in range(6))
    snaps = []
    n_total = GAS['n_burn'] + GAS['n_snap'] * GAS['every']
    for k in range(n_total + 1):
        i, o = k % 2, 1 - k % 2
        xi = torch.randn((n_sys,), generator=gen, device=dev)
        hip.npt_barostat(vel, mass, ptr, cells[i], W, a, p0, cells[o], mu, inv_mu, ke, pressure, volume, deps, s2=s2, noise=xi)
        if k > GAS['n_burn'] and (k - GAS['n_burn']) % GAS['every'] == 0:
            snaps.append(volume.clone())            # (the volume of the state after k steps, as the barostat of step k + 1 forms it)
        noise = torch.randn((N, 3), generator=gen, device=dev)
        hip.npt_step(xs[i], vel, zero, hk, 0.005, GAS['c1'], mr.BEGIN, mu=mu, inv_mu=inv_mu, mol_of_atom=mol, pos_out=xs[o],
                     sigma=sigma, noise=noise)
    snaps = _np(torch.stack(snaps)).astype(np.float64)
    assert snaps.shape == (GAS['n_snap'], n_sys) and np.all(np.isfinite(snaps)) and np.all(snaps > 0)
    mean_d, se_d = nr.mean_and_standard_error(snaps)
    mean_h, se_h = nr.mean_and_standard_error(host_gas())
    combined = float(np.hypot(se_d, se_h))
    print(f'ideal gas on the device: <V> = {mean_d:.4f} +- {se_d:.4f}; fp64 loop {mean_h:.4f} +- {se_h:.4f}; difference / combined '
          f'standard error {abs(mean_d - mean_h) / combined:.2f}; exact {GAS_EXACT}, margin {gas_margin(mean_d, se_d):.4f}')
    assert abs(mean_d - mean_h) <= 5.0 * combined
    assert abs(mean_d - GAS_EXACT) <= gas_margin(mean_d, se_d)


# ---- 8. interfaces ----------------------------------------------------------------------------------------------------------------

class PeriodicAtoms:
    """The accessors format_data() and run_npt() use"""
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


def test_interfaces():
    from newtonnet_amd.npt import BAR, ConstantPressure, NPTTrajectory
    from newtonnet_amd.utils import MLAseCalculator
    z, pos, cell, batch = _periodic_case('pbc_batch2_rand')
    N, B = pos.shape[0], 2
    model = make_model(util.load_state('rand'), props=('energy', 'gradient_force', 'stress'))
    P, T = torch.tensor([1.0, 2000.0]).cuda(), torch.tensor([100.0, 300.0]).cuda()
    dyn = model.constant_pressure(z, pos, cell, batch, P, T, friction=0.02, compressibility=4.5e-5, barostat_time=200.0)
    assert isinstance(dyn, ConstantPressure)
    assert np.array_equal(_np(dyn._p0), (np.array([1.0, 2000.0]) * BAR).astype(np.float32))            # one target per system
    assert float(dyn._s2[1] / dyn._s2[0]) == pytest.approx(3.0, rel=1e-6)                              # and one temperature
    traj = dyn.run(5, record_every=2)
    assert isinstance(traj, NPTTrajectory) and traj.step.tolist() == [2, 4, 5]
    assert traj.pos.shape == traj.vel.shape == (3, N, 3) and traj.cell.shape == (3, B, 3, 3)
    for name in ('potential_energy', 'kinetic_energy', 'total_energy', 'temperature', 'volume', 'pressure', 'density'):
        t = getattr(traj, name)
        assert t.shape == (3, B) and t.dtype == torch.float32 and t.is_cuda and torch.isfinite(t).all(), name
    np.testing.assert_allclose(_np(traj.volume), np.linalg.det(_np(traj.cell).astype(np.float64)), rtol=1e-6)
    assert torch.equal(dyn.cell, traj.cell[-1]) and torch.equal(dyn.positions, traj.pos[-1]) and dyn.step_count == 5
    assert torch.equal(dyn.volume, traj.volume[-1]) and torch.equal(dyn.internal_pressure, traj.pressure[-1])
    assert dyn.run(0).step.tolist() == [5]
    for bad in (dict(n_steps=-1), dict(n_steps=2.5), dict(n_steps=3, record_every=-1)):
        with pytest.raises(ValueError):
            dyn.run(**bad)
    # refusals that need the device: a cell without volume, a left-handed cell, tensors elsewhere
    with pytest.raises(ValueError, match='det'):
        model.constant_pressure(z, pos, torch.zeros_like(cell), batch, 1.0, 300.0)
    flipped = cell.clone()
    flipped[1, 0] *= -1.0
    with pytest.raises(ValueError, match='det'):
        model.constant_pressure(z, pos, flipped, batch, 1.0, 300.0)
    with pytest.raises(ValueError, match='pressure'):
        model.constant_pressure(z, pos, cell, batch, torch.tensor([1.0, 2.0]), 300.0)
    plain = make_model(util.load_state('rand'))
    with pytest.raises(ValueError, match='virial'):
        plain.constant_pressure(z, pos, cell, batch, 1.0, 300.0)
    # the calculator: two frames of the 125-atom box
    sel = _np(batch) == 1
    frames = [PeriodicAtoms(_np(z)[sel], _np(pos)[sel] + 0.01 * k, _np(cell)[1]) for k in range(2)]
    keep = [f.positions.copy() for f in frames]
    calc = MLAseCalculator(model, properties=['energy', 'forces', 'stress'], device='cuda')
    kw = dict(friction=0.01, barostat_time=200.0, record_every=4, seed=5)
    out = calc.run_npt(frames, 6, [1.0, 500.0], 150.0, **kw)
    n = int(sel.sum())
    assert out['step'].tolist() == [4, 6] and out['positions'].shape == out['velocities'].shape == (2, 2, n, 3)
    assert out['cell'].shape == (2, 2, 3, 3) and out['cell'].dtype == np.float32
    for k in ('energy', 'kinetic_energy', 'volume', 'pressure', 'density'):
        assert out[k].shape == (2, 2) and out[k].dtype == np.float32 and np.all(np.isfinite(out[k])), k
    again, other = calc.run_npt(frames, 6, [1.0, 500.0], 150.0, **kw), calc.run_npt(frames, 6, [1.0, 500.0], 150.0, **dict(kw, seed=6))
    assert all(np.array_equal(out[k], again[k]) for k in out) and not np.array_equal(out['cell'], other['cell'])
    assert all(np.array_equal(f.positions, k) for f, k in zip(frames, keep))
    one = calc.run_npt(frames[0], 3, 1.0, 150.0)
    assert one['positions'].shape == (1, n, 3) and one['cell'].shape == (1, 3, 3) and one['volume'].shape == (1,)
    with pytest.raises(ValueError, match='temperature'):
        calc.run_npt(frames, 3, 1.0, None)
    with pytest.raises(ValueError):
        calc.run_npt(frames, -1, 1.0, 150.0)
