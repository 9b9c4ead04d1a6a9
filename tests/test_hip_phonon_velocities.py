"""Phonon group velocities on the device (csrc/phonon_velocity.hip, Phonons.frequencies(velocities=True)) against the fp64 yardstick
of tests/phonon_velocity_ref.py: the kernel alone on exact eigenpairs, an analytic lattice with its crossings, flat bands, the
group cap, Gamma, bitwise independence of the launch, and the whole chain from the model's force constants to the transport tensor.

Bounds.  Kernel alone, per mode and component: (n_terms + 2 d + 16) eps32 sum |e_i| |term| |e_j| (phonon_velocity_ref.running_bound).
With device eigenvectors: BOUND_C eps32 max_a ||G_a||_F (1 + ||D||_F / gap) (phonon_velocity_ref.error_bound); BOUND_C is four
times the largest constant measured over the analytic, flat-band and end-to-end cases, rounded up to a power of two.  Every test
prints the fraction of its bound it used."""
import numpy as np
import pytest
import torch

from newtonnet_amd import hip
from newtonnet_amd import phonons as ph
from tests import phonon_ref as pr
from tests import phonon_velocity_ref as pv
from tests import util
from tests import vib_ref as vr
from tests.test_hip_hessian import make_model

pytestmark = pytest.mark.gpu

EPS32 = pr.EPS32


def make(case, **kw):
    fc, pos, cell, S, m = case
    return ph.Phonons.from_force_constants(np.asarray(fc, dtype=np.float32), np.ones(len(pos), dtype=np.int64), pos, cell, S,
                                           masses=np.asarray(m, dtype=np.float32), device='cuda', **kw)


def as_device(case):
    """the case with the force constants and masses as the device holds them (fp32), in fp64"""
    fc, pos, cell, S, m = case
    return np.asarray(fc, dtype=np.float32).astype(np.float64), pos, cell, S, np.asarray(m, dtype=np.float32).astype(np.float64)


def references(case, q, direction=None, deg_rel=None):
    """[problem()] per q with the tolerances referred to max |lambda| over the call, as the library refers them"""
    case = as_device(case)
    table = pr.image_table_fast(*case[1:4])
    scale = max(np.abs(np.linalg.eigvalsh(pr.dynamical_matrix(*case, x, table))).max() for x in q)
    n = None if direction is None else np.broadcast_to(np.asarray(direction, dtype=np.float64), (len(q), 3))
    return [pv.problem(*case, x, direction=None if n is None else n[k], deg_rel=deg_rel, scale=scale, table=table) for k, x in enumerate(q)]


def kernel_alone(p, q, evals, modes, deg_tol, zero_tol, direction=None):
    """nnhip_phonon_velocities on the one-crystal Phonons p with the eigenpairs given: (vel, dlam, group, defined, status) as numpy"""
    dev, Q, d = p.fc.device, len(q), p._dims[0]
    q_dev = torch.tensor(np.asarray(q, dtype=np.float64)).to(dev)
    ev = torch.tensor(np.asarray(evals, dtype=np.float32).reshape(-1)).to(dev)
    md = torch.view_as_real(torch.tensor(np.asarray(modes, dtype=np.complex64).reshape(-1)).to(dev)).contiguous()
    cells = torch.tensor(np.asarray(p._cells, dtype=np.float64)).to(dev)
    n_dev = None if direction is None else torch.tensor(np.asarray(direction, dtype=np.float64)).to(dev)
    tol = [torch.tensor([x], dtype=torch.float32, device=dev) for x in (deg_tol, zero_tol)]
    vel, dlam = (torch.zeros(Q * d, 3, dtype=torch.float32, device=dev) for _ in range(2))
    group = torch.zeros(Q * d, dtype=torch.int32, device=dev)
    defined = torch.zeros(Q * d, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, Q, dtype=torch.int32, device=dev)
    hip._check(hip.lib().nnhip_phonon_velocities(
        hip._ptr(p.fc), hip._ptr(p.fc_ptr), hip._ptr(p.cry_ptr), p._cry_host.data_ptr(), hip._ptr(p.sc_atoms), hip._ptr(p.img_ptr),
        hip._ptr(p.img_start), hip._ptr(p.img_off), hip._ptr(p.masses), hip._ptr(p.out_ptr), 1, hip._ptr(cells), hip._ptr(q_dev), Q,
        hip._ptr(n_dev), hip._ptr(ev), hip._ptr(md), hip._ptr(tol[0]), hip._ptr(tol[1]), hip._ptr(vel), hip._ptr(dlam), hip._ptr(group),
        hip._ptr(defined), hip._ptr(status), hip._stream(dev)), 'nnhip_phonon_velocities')
    torch.cuda.synchronize()
    return (vel.cpu().numpy().reshape(Q, d, 3), dlam.cpu().numpy().reshape(Q, d, 3), group.cpu().numpy().reshape(Q, d),
            defined.cpu().numpy().reshape(Q, d).astype(bool), status.cpu().numpy()[0])


def gradients(bands, b=0):
    Q, d, o = len(bands.q), bands._dims[b], bands._offsets[b]
    return bands.eigenvalue_gradients[Q * o:Q * (o + d)].view(Q, d, 3).cpu().numpy().astype(np.float64)


def group_of(bands, b=0):
    Q, d, o = len(bands.q), bands._dims[b], bands._offsets[b]
    return bands.degenerate_group[Q * o:Q * (o + d)].view(Q, d).cpu().numpy()


def check_against(refs, bands, b=0, what='', expect_status=0):
    """every mode of every q against its reference within error_bound(BOUND_C); nothing is left out besides what the result flags
    (velocity_defined False, status bit 3), and the reference must flag exactly the same modes.  Returns the largest C used."""
    dl, grp = gradients(bands, b), group_of(bands, b)
    v, ok = (x.cpu().numpy() for x in bands.velocities(b))
    ev = bands.crystal(b)[0].cpu().numpy().astype(np.float64)
    worst = 0.0
    for k, p in enumerate(refs):          # the measurement first, whatever the assertions below make of it
        err = np.abs(dl[k] - p['dlam']).max(axis=1)[~p['capped']]
        worst = max(worst, float((err / pv.error_bound(1.0, p)[~p['capped']]).max())) if err.size else worst
    print(f'{what}: largest C = {worst:.3e} (bound constant {pv.BOUND_C})')
    for k, p in enumerate(refs):
        assert int(bands.status[b, k]) == (ph.STATUS_GROUP if p['capped'].any() else 0) | expect_status, (what, k)
        assert np.array_equal(ok[k], p['defined']), f'{what} q {k}: the device flags {np.flatnonzero(~ok[k])}, the reference {np.flatnonzero(~p["defined"])}'
        assert np.array_equal(grp[k], p['first']), f'{what} q {k}: groups {grp[k]} against {p["first"]}'
        keep = ~p['capped']
        err = np.abs(dl[k] - p['dlam']).max(axis=1)
        one = pv.error_bound(1.0, p)
        assert np.all(err[keep] <= pv.BOUND_C * one[keep]), f'{what} q {k}: C = {(err[keep] / one[keep]).max():.3e} above {pv.BOUND_C}'
        assert np.all(dl[k][~keep] == 0.0) and np.all(v[k][~ok[k]] == 0.0)
        # the velocity is that of the signed frequency, from the device's own eigenvalue
        want = dl[k][ok[k]] / (2.0 * np.sqrt(np.abs(ev[k][ok[k]])))[:, None] * pv.ANGSTROM_PER_PS_PER_SQRT_EV_AMU
        assert np.all(np.abs(v[k][ok[k]] - want) <= 8 * EPS32 * np.abs(want)), f'{what} q {k}: velocity'
    return worst


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['d3x8', 'd6x27', 'd24x8', 'd24x27', 'd96x8', 'd99x8', 'tie'])
def test_stage_kernel_on_exact_eigenpairs(name):
    """the reference's fp64 eigenpairs rounded to fp32 go in; d lambda / d q per mode within the running-error bound (d = 99: one
    above the LDS solver's bound, two tiles of modes)"""
    if name == 'tie':
        case, n_copies = pr.tie_crystal(), 8
    else:
        d, n_copies = (int(x) for x in name[1:].split('x'))
        case = pr.stage_case(d, n_copies)
    p = make(case, solver='auto')
    case64 = as_device(case)
    table = pr.image_table_fast(*case64[1:4])
    q = pr.STAGE_Q
    refs, evals, modes = [], [], []
    for x in q:
        D = pr.dynamical_matrix(*case64, x, table)
        G, Gabs = pv.d_dynamical_matrix(*case64, x, table, with_abs=True)
        lam, V = np.linalg.eigh(D)
        refs.append((lam, V.T, G, Gabs))
        evals.append(lam)
        modes.append(V.T)
    # both tolerances zero: every mode a group of one (no two planted eigenvalues are equal), so that each is e^H G_a e of the
    # eigenvector given; the grouping has its own tests below
    assert all(np.diff(lam.astype(np.float32)).min() > 0 and np.abs(lam).min() > 0 for lam in evals)
    vel, dlam, group, defined, status = kernel_alone(p, q, evals, modes, 0.0, 0.0)
    assert not status.any() and defined.all() and np.array_equal(group, np.tile(np.arange(len(evals[0])), (len(q), 1)))
    worst = 0.0
    for k, (lam, E, G, Gabs) in enumerate(refs):
        E32 = E.astype(np.complex64).astype(np.complex128)          # what the kernel was given
        want = np.real(np.einsum('ki,aij,kj->ka', E32.conj(), G, E32))
        bound = pv.running_bound(E32, Gabs, n_copies)
        err = np.abs(dlam[k] - want)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), f'{name} q {k}: |d dlam| exceeds the running-error bound by {(err / bound).max():.3f} x'
    print(f'{name}: largest |d dlam| / bound = {worst:.3f}')


# ---- 2. the analytic lattice ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_fold', pv.ANALYTIC_FOLDS)
def test_analytic_lattice_and_its_crossings(n_fold):
    """d = 3, 6, 66 (one tile of modes holds all 66, so no group can straddle a tile here; the kernel-alone test above has two tiles at d = 99)"""
    case = pv.coupled_cubic_lattice(n_fold=n_fold)
    p = make(case)
    bands = p.frequencies(pv.ANALYTIC_Q, velocities=True)
    refs = references(case, pv.ANALYTIC_Q)
    for k, r in enumerate(refs):          # the yardstick is the formula here
        lam, dlam = pv.coupled_cubic_analytic(pv.ANALYTIC_Q[k], n_fold=n_fold)
        # (the reference works on the spring constants as the device holds them, rounded to fp32: the slopes are linear in them)
        assert np.abs(r['dlam'] - dlam).max() <= 2 * EPS32 * np.abs(dlam).max()
    check_against(refs, bands, what=f'analytic n_fold {n_fold}')
    # q_x = 1/2: every mode in a crossing pair (for n_fold >= 2), split along an explicit generic direction, in the reference's order
    q = pv.CROSSING_Q[None, :]
    bands = p.frequencies(q, velocities=True, direction=pv.CROSSING_DIRECTION)
    refs = references(case, q, direction=pv.CROSSING_DIRECTION)
    if n_fold > 1:
        assert refs[0]['first'].tolist() == [2 * (k // 2) for k in range(3 * n_fold)]
    check_against(refs, bands, what=f'crossing n_fold {n_fold}')


# ---- 3. flat bands ---------------------------------------------------------------------------------------------------------------

def test_flat_bands_have_no_velocity_and_name_their_groups():
    lam = np.concatenate([[-1.5, -1.5], [-0.7], [0.4] * 3, np.linspace(0.9, 2.6, 9), [3.1] * 5, np.linspace(3.6, 5.0, 10)])
    A64, A32 = vr.planted(lam, 4242)
    case = pr.gauge_case(A32)
    q = np.stack([pr.GAUGE_Q, [0.12, 0.4, -0.27]])
    bands = make(case).frequencies(q, velocities=True)
    refs = references(case, q)
    want = np.arange(30)
    want[0:2], want[3:6], want[15:20] = 0, 3, 15
    for r in refs:
        # (a planted group is split by the rounding of A to fp32, about 1e-7: rotated within the group the commutator that G is
        # here shows that splitting times the atoms' coordinates, not zero)
        assert np.array_equal(r['first'], want) and np.abs(r['dlam']).max() <= 1e-5
    check_against(refs, bands, what='flat bands')
    assert np.array_equal(group_of(bands), np.stack([want, want]))
    dl = gradients(bands)
    for k, r in enumerate(refs):
        assert np.all(np.abs(dl[k]).max(axis=1) <= pv.error_bound(pv.BOUND_C, r)), f'q {k}: a flat band has a slope'


# ---- 4. the cap ------------------------------------------------------------------------------------------------------------------

def test_groups_above_the_cap_are_flagged_and_the_rest_is_right():
    case = pv.folded_cubic_lattice(22)
    q = np.array([[0.3, 0.1, 0.2]])
    bands = make(case).frequencies(q, velocities=True)
    refs = references(case, q)
    assert refs[0]['capped'].sum() == 44 and int(bands.status[0, 0]) == ph.STATUS_GROUP
    check_against(refs, bands, what='cap')
    v, ok = bands.velocities(0)
    capped = torch.tensor(refs[0]['capped'], device=v.device)
    assert not ok[0][capped].any() and ok[0][~capped].all() and float(v[0][capped].abs().max()) == 0.0
    lam, dlam = pv.coupled_cubic_analytic(q[0], np.diag(pr.CUBIC_K), 22)          # the x branches against the formula
    x = np.abs(dlam[:, 0]) > 0
    assert np.abs(refs[0]['dlam'][~refs[0]['capped']] - dlam[x]).max() <= 2 * EPS32 * np.abs(dlam).max()          # (fp32 spring constants)


# ---- 5. Gamma ------------------------------------------------------------------------------------------------------------------

def test_gamma_and_negative_eigenvalues():
    H, fc = pr.random_crystal(2, pr.TRICLINIC_S, seed=5)
    plain = (fc.astype(np.float32), pr.TRICLINIC_POS, pr.TRICLINIC_CELL, pr.TRICLINIC_S, pr.TRICLINIC_MASSES.astype(np.float32))
    # springs obey the sum rule; it is imposed again on their fp32 values, as phonons() imposes it on a model's (the random
    # crystal's row sums are not symmetric 3 x 3 matrices, so acoustic_sum_rule, which symmetrises the block, cannot zero them)
    springs = pv.coupled_cubic_lattice(n_fold=2)
    asr = (ph.acoustic_sum_rule(torch.tensor(springs[0].astype(np.float32))).numpy(),) + springs[1:]
    q = np.array([[0.0, 0.0, 0.0], [0.31, -0.17, 0.44]])
    for name, case, n_zero in (('sum rule', asr, 3), ('no sum rule', plain, 0)):
        bands = make(case).frequencies(q, velocities=True)
        refs = references(case, q)
        ok = bands.velocities(0)[1].cpu().numpy()
        assert (~ok[0]).sum() == n_zero and ok[1].all(), name
        check_against(refs, bands, what=f'Gamma, {name}')
    # the spectrum without the sum rule is indefinite: v = d lambda / (2 sqrt|lambda|), the slope of -sqrt|lambda| x (-1)
    ev = bands.crystal(0)[0].cpu().numpy()
    v = bands.velocities(0)[0].cpu().numpy()
    neg = ev[1] < 0
    assert neg.any()
    want = gradients(bands)[1][neg] / (2.0 * np.sqrt(-ev[1][neg].astype(np.float64)))[:, None] * pv.ANGSTROM_PER_PS_PER_SQRT_EV_AMU
    assert np.all(np.abs(v[1][neg] - want) <= 8 * EPS32 * np.abs(want)) and np.abs(want).max() > 0


# ---- 6. bitwise ------------------------------------------------------------------------------------------------------------------

def planted_case(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3 * n, 3 * n))
    fc = (X + X.T).astype(np.float32).reshape(n, 3, n, 3)
    pos = rng.uniform(0.0, 9.0, (n, 3))
    m = rng.choice([1.008, 12.011, 15.999], n).astype(np.float32)
    return fc, pos, 9.0 * np.eye(3) + 0.3 * rng.standard_normal((3, 3)), (1, 1, 1), m


VFIELDS = ('group_velocities', 'velocity_defined', 'degenerate_group', 'eigenvalue_gradients')


def test_a_wave_vector_gives_the_same_bits_whatever_surrounds_it():
    _, fc = pr.random_crystal(2, pr.TRICLINIC_S, seed=5)
    a = (fc.astype(np.float32), pr.TRICLINIC_POS, pr.TRICLINIC_CELL, pr.TRICLINIC_S, pr.TRICLINIC_MASSES.astype(np.float32))
    b = planted_case(12, 7)
    both = ph.Phonons.from_force_constants([a[0], b[0]], np.ones(14, dtype=np.int64), np.concatenate([a[1], b[1]]), np.stack([a[2], b[2]]),
                                           np.array([a[3], b[3]]), masses=np.concatenate([a[4], b[4]]), batch=np.array([0] * 2 + [1] * 12),
                                           device='cuda')
    q = np.random.default_rng(17).uniform(-0.5, 0.5, (1000, 3))
    n = np.array([0.3, -0.5, 0.8])
    # (the tolerances refer to max |lambda| over the call, so a gap that lies between the tolerance of the 1000 and that of a q
    # alone could group differently: a chance of about 1e-6 for the seven q compared below)
    big =both.frequencies(q, velocities=True, direction=n)
    assert int(big.status.abs().max()) == 0
    again = both.frequencies(q, velocities=True, direction=n, dynamical_matrix=True, modes=True)
    plain = both.frequencies(q)
    for f in VFIELDS:
        assert torch.equal(getattr(big, f), getattr(again, f)), f
    assert big.modes is None and torch.equal(big.eigenvalues, plain.eigenvalues) and torch.equal(big.sweeps, plain.sweeps)
    assert torch.equal(big.status, plain.status) and torch.equal(big.frequencies, plain.frequencies)
    assert torch.equal(again.eigenvalues, plain.eigenvalues)
    alone = [make(a), make(b)]
    for k in (0, 1, 2, 3, 501, 998, 999):
        for c in (0, 1):
            one = alone[c].frequencies(q[k:k + 1], velocities=True, direction=n)
            assert torch.equal(one.velocities(0)[0][0], big.velocities(c)[0][k]), (k, c)
            assert np.array_equal(gradients(one)[0], gradients(big, c)[k]) and np.array_equal(group_of(one)[0], group_of(big, c)[k])
    # the same eigenpairs through tables built for the LDS solver and for the blocked one
    lds, blk = make(b, solver='lds'), make(b, solver='blocked')
    src = lds.frequencies(q[:4], modes=True)
    ev, md = src.crystal(0)[0].cpu().numpy(), src.crystal(0)[2].cpu().numpy()
    tol = pv.default_tol(36) * float(np.abs(ev).max())
    outs = [kernel_alone(p, q[:4], ev, md, tol, tol, direction=np.tile(n / np.linalg.norm(n), (4, 1))) for p in (lds, blk, lds)]
    for o in outs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(outs[0], o))
    # ... and the blocked solver's own modes serve as well as the LDS solver's
    refs = references(b, q[:4], direction=n)
    check_against(refs, blk.frequencies(q[:4], velocities=True, direction=n), what='blocked solver, d = 36')


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------

E2E_CELLS = np.array([[[4.2, 0.4, -0.3], [0.4, 4.1, 0.5], [-0.3, 0.5, 4.3]],
                      [[4.3, -0.2, 0.3], [-0.2, 4.2, -0.4], [0.3, -0.4, 4.1]]])
E2E_Z = np.array([6, 1, 8, 1, 1])
E2E_POS = np.array([[0.4, 0.5, 0.3], [1.3, 1.1, 1.0], [0.6, 0.4, 0.5], [1.4, 0.9, 0.8], [0.1, 1.2, 0.2]])
E2E_BATCH = np.array([0, 0, 1, 1, 1])
E2E_S = (3, 3, 3)


@pytest.fixture(scope='module')
def e2e():
    model = make_model(util.load_state('rand'))
    z, batch = torch.tensor(E2E_Z), torch.tensor(E2E_BATCH)
    pos, cell = torch.tensor(E2E_POS, dtype=torch.float32), torch.tensor(E2E_CELLS, dtype=torch.float32)
    p = model.phonons(*[t.cuda() for t in (z, pos, cell, batch)], supercell=E2E_S)
    cases = []
    for b, (lo, hi) in enumerate(((0, 2), (2, 5))):
        m = np.array([vr.MASSES[int(x)] for x in E2E_Z[lo:hi]], dtype=np.float32)
        cases.append((p.force_constants(b).cpu().numpy(), pos[lo:hi].double().numpy(), cell[b].double().numpy(), E2E_S, m))
    return dict(p=p, cases=cases)


def assert_bound_is_tight(refs, what):
    """the condition tests/test_phonon_velocity_host.py holds on the analytic inputs, on inputs that exist on the device only"""
    ratio = [(pv.error_bound(pv.BOUND_C, r)[r['defined']] / np.abs(r['dlam']).max()).max() for r in refs]
    print(f'{what}: bound / largest |dlam| = {max(ratio):.2e} at most')
    assert max(ratio) <= 0.01, (what, ratio)


def test_end_to_end_velocities_against_the_reference(e2e):
    p = e2e['p']
    # generic q and a generic path: at Gamma and on the zone boundary the slopes vanish, and no bound is 1 % of nothing
    # (test_gamma_and_negative_eigenvalues has Gamma; the mesh of the transport tensor below holds both)
    q = np.random.default_rng(23).uniform(-0.5, 0.5, (6, 3))
    bands = p.frequencies(q, velocities=True)
    for b in range(2):
        refs = references(e2e['cases'][b], q)
        assert_bound_is_tight(refs, f'crystal {b}')
        check_against(refs, bands, b, what=f'end to end, crystal {b}')
    points = [[0.15, 0.1, 0.05], [0.35, 0.2, 0.15], [0.25, 0.4, 0.3]]
    path = p.band_structure(points, 3, velocities=True)
    for b in range(2):
        n = ph.segment_directions(points, 3, e2e['cases'][b][2])
        refs = references(e2e['cases'][b], path.q, direction=n)
        assert_bound_is_tight(refs, f'path, crystal {b}')
        check_against(refs, path, b, what=f'band structure, crystal {b}')


def test_transport_tensor_against_the_reference(e2e):
    """Every term C_v v_a v_b carries the relative error 2 dv / |v| + |dC_v / d lambda| d lambda / C_v of fp32 eigenpairs, both of the order
    d eps32 lambda_max / lambda <= 1e-5 on the modes a 4^3 mesh keeps: 1e-4 of the largest element."""
    p = e2e['p']
    mesh = p.mesh(4, 4, 4, velocities=True)
    kappa = mesh.transport_tensor(300.0)
    assert tuple(kappa.shape) == (2, 3, 3) and kappa.dtype == torch.float32 and torch.equal(kappa, kappa.transpose(1, 2))
    thr = mesh.threshold().cpu().numpy()
    for b in range(2):
        refs = references(e2e['cases'][b], mesh.bands.q)
        want = pv.transport_tensor(np.stack([r['lam'] for r in refs]), np.stack([r['v'] for r in refs]), np.stack([r['defined'] for r in refs]),
                                   300.0, float(thr[b]), abs(np.linalg.det(e2e['cases'][b][2])))
        got = kappa[b].cpu().numpy().astype(np.float64)
        print(f'crystal {b}: kappa / tau = {np.diag(want)} W/(m K)/ps, largest difference {np.abs(got - want).max() / np.abs(want).max():.2e}')
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
        assert np.all(np.linalg.eigvalsh(want) > 0)
    assert float(mesh.transport_tensor(0.0).abs().max()) == 0.0
    with pytest.raises(ValueError, match='velocities=True'):
        p.mesh(2, 2, 2).transport_tensor(300.0)
    # the cubic lattice: every branch moves along its own axis
    fc, pos, cell = pr.cubic_lattice()
    cub = make((fc, pos, cell, pr.CUBIC_S, [pr.CUBIC_MASS])).mesh(4, 4, 4, velocities=True).transport_tensor(300.0)[0].cpu().numpy()
    assert np.all(np.diag(cub) > 0) and np.abs(cub - np.diag(np.diag(cub))).max() <= 1e-6 * np.diag(cub).max()


@pytest.mark.parametrize('kind', ['pair', 'cap'])
def test_a_crystal_above_the_lds_bound_through_auto(kind):
    """d = 99 (33 atoms, phonon_velocity_ref.planted_levels_crystal) through solver='auto': the blocked solver's modes, two tiles of
    modes in the velocity kernel, direction=None on a triclinic cell.  'pair': modes 63 and 64 -- the last of the first tile and
    the first of the second -- belong to different atoms and cross at this q with different slopes, so the group straddles the
    tiles and its order comes from the kernel's own default direction.  'cap': modes 55 .. 72 coincide, a group above the cap that
    spans the tiles."""
    case = pv.planted_levels_crystal(pv.straddle_levels(kind))
    q = pv.STRADDLE_Q[None, :]
    bands = make(case, solver='auto').frequencies(q, velocities=True)
    refs = references(case, q)
    r = refs[0]
    want = np.arange(99)
    if kind == 'pair':
        want[64] = 63
        assert_bound_is_tight(refs, 'd = 99')
        split = (r['dlam'][64] - r['dlam'][63]) @ r['n']
        # (each eigenvalue of M_n is known within the bound: twice the bound decides the order, four times leaves a margin)
        assert split > 4 * pv.error_bound(pv.BOUND_C, r)[63:65].max(), 'the pair must be told apart by its slopes along n'
    else:
        want[55:73] = 55
        assert r['capped'].sum() == 18 and r['capped'][55:73].all()
    assert np.array_equal(r['first'], want)
    assert np.abs(r['n']).min() > 0.2          # the default direction is no axis of the cell
    check_against(refs, bands, what=f'd = 99 through auto, {kind}')
    if kind == 'cap':
        v, ok = (x.cpu().numpy() for x in bands.velocities(0))
        assert not ok[0][55:73].any() and ok[0][:55].all() and ok[0][73:].all() and np.all(v[0][55:73] == 0.0)
