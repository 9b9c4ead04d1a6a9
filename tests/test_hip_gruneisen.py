"""Mode Grueneisen parameters on the device (csrc/phonon_gruneisen.hip, newtonnet_amd/gruneisen.py) against the fp64 yardstick of
tests/gruneisen_ref.py: the kernel alone on exact eigenpairs, the Rayleigh identity, an analytic lattice, the group cap, a crystal
above the LDS solver, bitwise independence of the launch, and the whole chain from the model's force constants to the thermal
expansion.

Bounds.  Kernel alone, per mode and plane: (n_terms + 2 d + 16) eps32 sum |e_i| |term| |e_j| (gruneisen_ref.running_bound; derived, no
constant).  With device eigenvectors: BOUND_C eps32 max_k ||dD_k||_F (1 + ||D||_F / gap) (gruneisen_ref.error_bound).  Every test
prints the fraction of its bound it used.

Measured on the MI355X.  Kernel alone, largest error / running bound: 0.030, 0.007, 0.005, 0.007, 0.003, 0.002, 0.007 (d3x8 .. tie).
Constant C of error_bound: analytic lattice 0.12 / 0.32 / 0.26 (n_fold 1 / 2 / 22), its crossings 0.34 / 0.05 / 0.48, the cap case
0.26, d = 99 through 'auto' 8.5e-4 (pair) and 1.2e-3 (cap), the blocked solver's modes at d = 36 0.29, end to end 7.5 and 11.4
('volume', crystals 0 and 1), 6.0 and 12.4 ('voigt').  BOUND_C = 16, the velocity kernel's, holds on all of them.  Four times the
largest, rounded up to a power of two, would be 64; that rule is not met, because 64 breaks the 1 % condition of
tests/test_gruneisen_host.py at d = 66 (3.7 %): the margin over other seeds and q is 1.3.
Rayleigh identity on exact eigenpairs (dfc = fc): |gamma + 1/2| at most 1 eps32 on the sum-rule lattice and 7 and 8 eps32 on the random
crystal's smallest eigenvalue (0.038 and 0.067 in spectra reaching 5.7 and 8.4), against the 8 eps32 allowed: that mode sits at the
bound.  With the solver's own eigenpairs the same quantity reaches 17 eps32 (the solver's eigenvalue carries a few eps32 of ||D||,
not of lambda), which is why the identity is held where the specification puts it, on exact eigenpairs."""
import numpy as np
import pytest
import torch

from newtonnet_amd import gruneisen as gn
from newtonnet_amd import hip
from newtonnet_amd import phonons as ph
from tests import gruneisen_ref as gr
from tests import hessian_ref as hr
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


def make_g(case, planes, weights=None, **kw):
    """a Gruneisen over the one-crystal case with the planes given ([K, n, 3, N, 3])"""
    p = make(case, **kw)
    dfc = torch.tensor(np.asarray(planes, dtype=np.float32).reshape(len(planes), -1)).cuda()
    return gn.Gruneisen(p, dfc, None, None, 'custom', weights)


def as_device(case):
    """the case with the force constants and masses as the device holds them (fp32), in fp64"""
    fc, pos, cell, S, m = case
    return np.asarray(fc, dtype=np.float32).astype(np.float64), pos, cell, S, np.asarray(m, dtype=np.float32).astype(np.float64)


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def references(case, planes, q, weights=None, deg_rel=None):
    """[problem()] per q with the tolerances referred to max |lambda| over the call, as the library refers them"""
    fc, pos, cell, S, m = as_device(case)
    table = pr.image_table_fast(pos, cell, S)
    scale = max(np.abs(np.linalg.eigvalsh(pr.dynamical_matrix(fc, pos, cell, S, m, x, table))).max() for x in q)
    return [gr.problem(fc, f32(planes), pos, cell, S, m, x, weights=weights, deg_rel=deg_rel, scale=scale, table=table) for x in q]


def kernel_alone(p, dfc, split, q, evals, modes, deg_tol, zero_tol):
    """nnhip_phonon_strain_slopes on the one-crystal Phonons p with the eigenpairs given; dfc a device tensor [K, n_fc], split a device
    tensor [n_fc] (or None: plane 0 itself).  (dlam [Q, d, K], gamma, group, defined, status) as numpy"""
    dev, Q, d, K = p.fc.device, len(q), p._dims[0], dfc.shape[0]
    q_dev = torch.tensor(np.asarray(q, dtype=np.float64)).to(dev)
    ev = torch.tensor(np.asarray(evals, dtype=np.float32).reshape(-1)).to(dev)
    md = torch.view_as_real(torch.tensor(np.asarray(modes, dtype=np.complex64).reshape(-1)).to(dev)).contiguous()
    tol = [torch.tensor([x], dtype=torch.float32, device=dev) for x in (deg_tol, zero_tol)]
    dlam, gam = (torch.zeros(Q * d, K, dtype=torch.float32, device=dev) for _ in range(2))
    group = torch.zeros(Q * d, dtype=torch.int32, device=dev)
    defined = torch.zeros(Q * d, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, Q, dtype=torch.int32, device=dev)
    sp = dfc[0] if split is None else split
    hip._check(hip.lib().nnhip_phonon_strain_slopes(
        hip._ptr(dfc), K, dfc.stride(0), hip._ptr(sp), hip._ptr(p.fc_ptr), hip._ptr(p.cry_ptr), p._cry_host.data_ptr(),
        hip._ptr(p.sc_atoms), hip._ptr(p.img_ptr), hip._ptr(p.img_start), hip._ptr(p.img_off), hip._ptr(p.masses), hip._ptr(p.out_ptr),
        1, hip._ptr(q_dev), Q, hip._ptr(ev), hip._ptr(md), hip._ptr(tol[0]), hip._ptr(tol[1]), hip._ptr(dlam), hip._ptr(gam),
        hip._ptr(group), hip._ptr(defined), hip._ptr(status), hip._stream(dev)), 'nnhip_phonon_strain_slopes')
    torch.cuda.synchronize()
    return (dlam.cpu().numpy().reshape(Q, d, K), gam.cpu().numpy().reshape(Q, d, K), group.cpu().numpy().reshape(Q, d),
            defined.cpu().numpy().reshape(Q, d).astype(bool), status.cpu().numpy()[0])


def slopes(bands, b=0):
    return bands.strain_gradients(b).cpu().numpy().astype(np.float64)


def group_of(bands, b=0):
    Q, d, o = len(bands.q), bands._dims[b], bands._offsets[b]
    return bands.degenerate_group[Q * o:Q * (o + d)].view(Q, d).cpu().numpy()


def check_against(refs, bands, b=0, what='', expect_status=0):
    """every mode of every q and every plane against its reference within error_bound(BOUND_C); nothing is left out besides what the
    result flags, and the reference must flag exactly the same modes.  Returns the largest C used."""
    dl, grp = slopes(bands, b), group_of(bands, b)
    g, ok = (x.cpu().numpy() for x in bands.gruneisen_parameters(b))
    ev = bands.crystal(b)[0].cpu().numpy().astype(np.float64)
    worst = 0.0
    for k, p in enumerate(refs):          # the measurement first, whatever the assertions below make of it
        err = np.abs(dl[k] - p['dlam']).max(axis=1)[~p['capped']]
        worst = max(worst, float((err / gr.error_bound(1.0, p)[~p['capped']]).max())) if err.size else worst
    print(f'{what}: largest C = {worst:.3e} (bound constant {gr.BOUND_C})')
    for k, p in enumerate(refs):
        assert int(bands.status[b, k]) == (ph.STATUS_GROUP if p['capped'].any() else 0) | expect_status, (what, k)
        assert np.array_equal(ok[k], p['defined']), f'{what} q {k}: the device flags {np.flatnonzero(~ok[k])}, the reference {np.flatnonzero(~p["defined"])}'
        assert np.array_equal(grp[k], p['first']), f'{what} q {k}: groups {grp[k]} against {p["first"]}'
        keep = ~p['capped']
        err = np.abs(dl[k] - p['dlam']).max(axis=1)
        one = gr.error_bound(1.0, p)
        assert np.all(err[keep] <= gr.BOUND_C * one[keep]), f'{what} q {k}: C = {(err[keep] / one[keep]).max():.3e} above {gr.BOUND_C}'
        assert np.all(dl[k][~keep] == 0.0) and np.all(g[k][~ok[k]] == 0.0)
        # gamma is -dlam / (2 lambda) of the device's own eigenvalue
        want = -dl[k][ok[k]] / (2.0 * ev[k][ok[k]])[:, None]
        assert np.all(np.abs(g[k][ok[k]] - want) <= 8 * EPS32 * np.abs(want)), f'{what} q {k}: gamma'
    return worst


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['d3x8', 'd6x27', 'd24x8', 'd24x27', 'd96x8', 'd99x8', 'tie'])
def test_stage_kernel_on_exact_eigenpairs(name):
    """the reference's fp64 eigenpairs rounded to fp32 go in with six random planes (K = 6, split along plane 0) and with plane 0
    alone (K = 1); d lambda / d eta per mode and plane within the running-error bound, no mode left out; plane 0 gives the same bits
    either way"""
    if name == 'tie':
        case, n_copies = pr.tie_crystal(), 8
    else:
        d, n_copies = (int(x) for x in name[1:].split('x'))
        case = pr.stage_case(d, n_copies)
    p = make(case, solver='auto')
    fc, pos, cell, S, m = as_device(case)
    table = pr.image_table_fast(pos, cell, S)
    planes = np.random.default_rng(len(name) + fc.shape[0]).standard_normal((6,) + fc.shape).astype(np.float32)
    q = pr.STAGE_Q
    refs, evals, modes = [], [], []
    for x in q:
        D = gr.d_dynamical(fc[None], pos, cell, S, m, x, table)[0]
        dD, dDabs = gr.d_dynamical(planes.astype(np.float64), pos, cell, S, m, x, table, with_abs=True)
        lam, V = np.linalg.eigh(D)
        refs.append((V.T, dD, dDabs))
        evals.append(lam)
        modes.append(V.T)
    # both tolerances zero: every mode a group of one (no two planted eigenvalues are equal)
    assert all(np.diff(lam.astype(np.float32)).min() > 0 and np.abs(lam).min() > 0 for lam in evals)
    dfc = torch.tensor(planes.reshape(6, -1)).cuda()
    dlam, gam, group, defined, status = kernel_alone(p, dfc, None, q, evals, modes, 0.0, 0.0)
    one = kernel_alone(p, dfc[:1].clone(), None, q, evals, modes, 0.0, 0.0)
    assert not status.any() and defined.all() and np.array_equal(group, np.tile(np.arange(len(evals[0])), (len(q), 1)))
    assert np.array_equal(one[0][..., 0], dlam[..., 0]) and np.array_equal(one[1][..., 0], gam[..., 0])
    assert np.array_equal(one[2], group) and np.array_equal(one[3], defined) and not one[4].any()
    worst = 0.0
    for k, (E, dD, dDabs) in enumerate(refs):
        E32 = E.astype(np.complex64).astype(np.complex128)          # what the kernel was given
        want = np.real(np.einsum('ki,aij,kj->ka', E32.conj(), dD, E32))
        bound = gr.running_bound(E32, dDabs, n_copies)
        err = np.abs(dlam[k] - want)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), f'{name} q {k}: |d dlam| exceeds the running-error bound by {(err / bound).max():.3f} x'
        lam32 = evals[k].astype(np.float32).astype(np.float64)
        want_g = -dlam[k].astype(np.float64) / (2.0 * lam32)[:, None]
        assert np.all(np.abs(gam[k] - want_g) <= 8 * EPS32 * np.abs(want_g))
    print(f'{name}: largest |d dlam| / bound = {worst:.3f}')


# ---- 2. the Rayleigh identity --------------------------------------------------------------------------------------------------

def rayleigh_cases():
    H, fc = pr.random_crystal(2, pr.TRICLINIC_S, seed=5)
    plain = (fc.astype(np.float32), pr.TRICLINIC_POS, pr.TRICLINIC_CELL, pr.TRICLINIC_S, pr.TRICLINIC_MASSES.astype(np.float32))
    # springs obey the sum rule; it is imposed again on their fp32 values, as phonons() imposes it on a model's
    springs = pv.coupled_cubic_lattice(n_fold=2)
    asr = (ph.acoustic_sum_rule(torch.tensor(springs[0].astype(np.float32))).numpy(),) + springs[1:]
    return (('sum rule', asr, 3), ('no sum rule', plain, 0))


RAYLEIGH_Q = np.array([[0.0, 0.0, 0.0], [0.31, -0.17, 0.44]])


def test_rayleigh_identity_and_negative_eigenvalues():
    """dfc = dfc_split = fc: dlam = e^H D e of the device's own mode within the running bound; at Gamma with the sum rule exactly three
    modes are undefined; an indefinite spectrum has defined gamma for negative lambda"""
    q = RAYLEIGH_Q
    for name, case, n_zero in rayleigh_cases():
        g = make_g(case, [case[0]])
        assert g.dfc_split.data_ptr() == g.dfc.data_ptr()
        bands = g.frequencies(q, modes=True)
        gam, ok = (x.cpu().numpy() for x in bands.gruneisen_parameters(0))
        ok = ok.astype(bool)
        assert (~ok[0]).sum() == n_zero and ok[1].all(), name
        f64, pos, cell, S, m = as_device(case)
        table = pr.image_table_fast(pos, cell, S)
        dl, ev = slopes(bands), bands.crystal(0)[0].cpu().numpy().astype(np.float64)
        E = bands.crystal(0)[2].cpu().numpy().astype(np.complex128)
        for k in range(len(q)):
            D, Dabs = gr.d_dynamical(f64[None], pos, cell, S, m, q[k], table, with_abs=True)
            ray = np.real(np.einsum('ki,ij,kj->k', E[k].conj(), D[0], E[k]))
            bound = gr.running_bound(E[k], Dabs, f64.shape[2] // f64.shape[0])[:, 0]
            # where a group was rotated the kernel's vector is a combination of the group's: compare the group's sums
            first = group_of(bands)[k]
            for s in np.unique(first):
                sel = first == s
                assert abs(dl[k][sel, 0].sum() - ray[sel].sum()) <= bound[sel].sum(), (name, k, s)
            print(f'{name} q {k}: largest |dlam - e^H D e| / bound = {(np.abs(dl[k][:, 0] - ray) / bound).max():.3f}')
            assert np.all(gam[k][~ok[k]] == 0.0)
            # gamma is -dlam / (2 lambda) of the device's own numbers, and -1/2 within what the bound of dlam leaves of it
            want = -dl[k][ok[k], 0] / (2.0 * ev[k][ok[k]])
            assert np.all(np.abs(gam[k][ok[k], 0] - want) <= 8 * EPS32 * np.abs(want))
    neg = ev[1] < 0          # the spectrum without the sum rule is indefinite: gamma is defined for negative lambda
    assert neg.any() and ok[1][neg].all() and np.all(gam[1][neg, 0] < 0)


def test_rayleigh_identity_gamma_is_minus_one_half():
    """dfc = dfc_split = fc on the reference's fp64 eigenpairs rounded to fp32 (the kernel alone, as in test 1: the running-error bound
    of these two tests is that of exact eigenvectors): dlam = e^H D e within the running bound of lambda, and gamma = -1/2 to
    8 eps32 wherever defined, the bound the feature's specification sets.  The tolerances are the library's defaults, so that the
    three acoustic modes at Gamma are undefined."""
    worst = []
    for name, case, n_zero in rayleigh_cases():
        p = make(case)
        fc, pos, cell, S, m = as_device(case)
        table = pr.image_table_fast(pos, cell, S)
        evals, modes, refs = [], [], []
        for x in RAYLEIGH_Q:
            D, Dabs = gr.d_dynamical(fc[None], pos, cell, S, m, x, table, with_abs=True)
            lam, V = np.linalg.eigh(D[0])
            evals.append(lam)
            modes.append(V.T)
            refs.append((D[0], Dabs))
        tol = pv.default_tol(len(evals[0])) * max(np.abs(lam).max() for lam in evals)
        dlam, gam, group, defined, status = kernel_alone(p, p.fc[None], None, RAYLEIGH_Q, evals, modes, tol, tol)
        assert not status.any() and (~defined[0]).sum() == n_zero and defined[1].all(), name
        for k, (D, Dabs) in enumerate(refs):
            E32 = modes[k].astype(np.complex64).astype(np.complex128)
            ray = np.real(np.einsum('ki,ij,kj->k', E32.conj(), D, E32))
            bound = gr.running_bound(E32, Dabs, fc.shape[2] // fc.shape[0])[:, 0]
            ok = defined[k]
            for s0 in np.unique(group[k]):          # a rotated group (the acoustic modes at Gamma): its sum
                sel = group[k] == s0
                assert abs(dlam[k][sel, 0].sum() - ray[sel].sum()) <= bound[sel].sum(), (name, k, s0)
            dev = np.abs(gam[k][ok, 0].astype(np.float64) + 0.5) / EPS32
            print(f'{name} q {k}: |gamma + 1/2| / eps32 = {dev}, lambda = {evals[k][ok]}, |dlam - e^H D e| / bound = '
                  f'{(np.abs(dlam[k][:, 0] - ray) / bound)[ok].max():.3f}')
            assert np.all(gam[k][~ok] == 0.0)
            worst.append((float(dev.max()), name, k))
    assert max(worst)[0] <= 8, f'largest |gamma + 1/2| = {max(worst)[0]:.2f} eps32 ({max(worst)[1]}, q {max(worst)[2]})'


# ---- 3. the analytic lattice ---------------------------------------------------------------------------------------------------

def analytic_case(n_fold):
    return pv.coupled_cubic_lattice(n_fold=n_fold), pv.coupled_cubic_lattice(gr.ANALYTIC_DK, n_fold=n_fold)[0][None]


@pytest.mark.parametrize('n_fold', pv.ANALYTIC_FOLDS)
def test_analytic_lattice_and_its_crossings(n_fold):
    case, planes = analytic_case(n_fold)
    g = make_g(case, planes)
    bands = g.frequencies(pv.ANALYTIC_Q)
    refs = references(case, planes, pv.ANALYTIC_Q)
    for k, r in enumerate(refs):          # the yardstick is the formula here
        lam, dlam = gr.coupled_cubic_slopes(pv.ANALYTIC_Q[k], n_fold=n_fold)
        assert np.abs(r['dlam'][:, 0] - dlam).max() <= 2 * EPS32 * np.abs(dlam).max()
    check_against(refs, bands, what=f'analytic n_fold {n_fold}')
    # q_x = 1/2: every mode in a crossing pair (for n_fold >= 2); the pair keeps one slope under this plane (gruneisen_ref)
    q = pv.CROSSING_Q[None, :]
    bands = g.frequencies(q)
    refs = references(case, planes, q)
    if n_fold > 1:
        assert refs[0]['first'].tolist() == [2 * (k // 2) for k in range(3 * n_fold)]
    lam, dlam = gr.coupled_cubic_slopes(q[0], n_fold=n_fold)
    assert np.abs(refs[0]['dlam'][:, 0] - dlam).max() <= 2 * EPS32 * np.abs(dlam).max()
    check_against(refs, bands, what=f'crossing n_fold {n_fold}')


# ---- 4. the cap ------------------------------------------------------------------------------------------------------------------

def test_groups_above_the_cap_are_flagged_and_the_rest_is_right():
    case = pv.folded_cubic_lattice(22)
    planes = pv.coupled_cubic_lattice(np.diag([0.5, 1.25, -0.75]), 22)[0][None]
    q = np.array([[0.3, 0.1, 0.2]])
    bands = make_g(case, planes).frequencies(q)
    refs = references(case, planes, q)
    assert refs[0]['capped'].sum() == 44 and int(bands.status[0, 0]) == ph.STATUS_GROUP
    check_against(refs, bands, what='cap')
    gam, ok = bands.gruneisen_parameters(0)
    capped = torch.tensor(refs[0]['capped'], device=gam.device)
    assert not ok[0][capped].any() and ok[0][~capped].all() and float(gam[0][capped].abs().max()) == 0.0
    assert float(bands.strain_gradients(0)[0][capped].abs().max()) == 0.0


# ---- 5. above the LDS solver -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['pair', 'cap'])
def test_a_crystal_above_the_lds_bound_through_auto(kind):
    """d = 99 through solver='auto': the blocked solver's modes, two tiles of modes in the kernel.  'pair': modes 63 and 64 -- the last
    of the first tile and the first of the second -- live on different atoms and cross; the plane scales every atom's force constants
    by its own factor (gruneisen_ref.atom_scaled_plane), so the group straddles the tiles and is split by the plane.  'cap': modes
    55 .. 72 coincide, a group above the cap that spans the tiles."""
    case = pv.planted_levels_crystal(pv.straddle_levels(kind))
    planes = gr.atom_scaled_plane(f32(case[0]))[0][None]
    q = pv.STRADDLE_Q[None, :]
    bands = make_g(case, planes, solver='auto').frequencies(q)
    refs = references(case, planes, q)
    r = refs[0]
    want = np.arange(99)
    if kind == 'pair':
        want[64] = 63
        split = r['dlam'][64, 0] - r['dlam'][63, 0]
        assert split > 4 * gr.error_bound(gr.BOUND_C, r)[63:65].max(), 'the pair must be told apart by its slopes along the plane'
    else:
        want[55:73] = 55
        assert r['capped'].sum() == 18 and r['capped'][55:73].all()
    assert np.array_equal(r['first'], want)
    check_against(refs, bands, what=f'd = 99 through auto, {kind}')
    if kind == 'cap':
        gam, ok = (x.cpu().numpy() for x in bands.gruneisen_parameters(0))
        assert not ok[0][55:73].any() and ok[0][:55].all() and ok[0][73:].all() and np.all(gam[0][55:73] == 0.0)


# ---- 6. bitwise ------------------------------------------------------------------------------------------------------------------

def planted_case(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3 * n, 3 * n))
    fc = (X + X.T).astype(np.float32).reshape(n, 3, n, 3)
    pos = rng.uniform(0.0, 9.0, (n, 3))
    m = rng.choice([1.008, 12.011, 15.999], n).astype(np.float32)
    return fc, pos, 9.0 * np.eye(3) + 0.3 * rng.standard_normal((3, 3)), (1, 1, 1), m


GFIELDS = ('gruneisen', 'eigenvalue_strain_gradients', 'gruneisen_defined', 'degenerate_group')


def test_a_problem_gives_the_same_bits_whatever_surrounds_it():
    _, fc = pr.random_crystal(2, pr.TRICLINIC_S, seed=5)
    a = (fc.astype(np.float32), pr.TRICLINIC_POS, pr.TRICLINIC_CELL, pr.TRICLINIC_S, pr.TRICLINIC_MASSES.astype(np.float32))
    b = planted_case(12, 7)
    both = ph.Phonons.from_force_constants([a[0], b[0]], np.ones(14, dtype=np.int64), np.concatenate([a[1], b[1]]), np.stack([a[2], b[2]]),
                                           np.array([a[3], b[3]]), masses=np.concatenate([a[4], b[4]]), batch=np.array([0] * 2 + [1] * 12),
                                           device='cuda')
    rng = np.random.default_rng(29)
    pa, pb = (rng.standard_normal((6, x[0].size)).astype(np.float32) for x in (a, b))
    w = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]          # the split plane is plane 0 in every object below (0 x a finite value adds nothing)
    G = gn.Gruneisen(both, torch.tensor(np.concatenate([pa, pb], axis=1)).cuda(), None, None, 'custom', w)
    q = np.random.default_rng(17).uniform(-0.5, 0.5, (1000, 3))
    big = G.frequencies(q)
    assert int(big.status.abs().max()) == 0
    again = G.frequencies(q, modes=True)
    plain = both.frequencies(q)
    for f in GFIELDS:
        assert torch.equal(getattr(big, f), getattr(again, f)), f
    assert big.modes is None and again.modes is not None
    assert torch.equal(big.eigenvalues, plain.eigenvalues) and torch.equal(big.sweeps, plain.sweeps)
    assert torch.equal(big.status, plain.status) and torch.equal(big.frequencies, plain.frequencies)
    # alone (the pointers of crystal 1 moved to the front), with six planes and with plane 0 only (K = 1: one plane streamed)
    alone6 = [gn.Gruneisen(make(c), torch.tensor(pl).cuda(), None, None, 'custom', w) for c, pl in ((a, pa), (b, pb))]
    alone1 = [gn.Gruneisen(make(c), torch.tensor(pl[:1]).cuda(), None, None, 'custom') for c, pl in ((a, pa), (b, pb))]
    assert all(g.dfc_split.data_ptr() == g.dfc.data_ptr() for g in alone1) and all(g.dfc_split.data_ptr() != g.dfc.data_ptr() for g in alone6)
    for k in (0, 1, 2, 3, 501, 998, 999):
        for c in (0, 1):
            six = alone6[c].frequencies(q[k:k + 1])
            one = alone1[c].frequencies(q[k:k + 1])
            assert torch.equal(six.gruneisen_parameters(0)[0][0], big.gruneisen_parameters(c)[0][k]), (k, c)
            assert torch.equal(six.strain_gradients(0)[0], big.strain_gradients(c)[k]) and np.array_equal(group_of(six)[0], group_of(big, c)[k])
            assert torch.equal(six.gruneisen_parameters(0)[1][0], big.gruneisen_parameters(c)[1][k])
            assert torch.equal(one.strain_gradients(0)[0][:, 0], six.strain_gradients(0)[0][:, 0]), (k, c)
            assert torch.equal(one.gruneisen_parameters(0)[0][0][:, 0], six.gruneisen_parameters(0)[0][0][:, 0])
            assert np.array_equal(group_of(one), group_of(six))
    # the same eigenpairs through tables built for the LDS solver and for the blocked one
    lds, blk = make(b, solver='lds'), make(b, solver='blocked')
    src = lds.frequencies(q[:4], modes=True)
    ev, md = src.crystal(0)[0].cpu().numpy(), src.crystal(0)[2].cpu().numpy()
    tol = pv.default_tol(36) * float(np.abs(ev).max())
    dfc = torch.tensor(pb).cuda()
    outs = [kernel_alone(p, dfc, None, q[:4], ev, md, tol, tol) for p in (lds, blk, lds)]
    for o in outs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(outs[0], o))
    # ... and the blocked solver's own modes serve as well as the LDS solver's
    refs = references(b, pb.reshape((6,) + b[0].shape), q[:4], weights=w)
    check_against(refs, gn.Gruneisen(blk, dfc, None, None, 'custom', w).frequencies(q[:4]), what='blocked solver, d = 36')


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------

E2E_CELLS = np.array([[[4.2, 0.4, -0.3], [0.4, 4.1, 0.5], [-0.3, 0.5, 4.3]],
                      [[4.3, -0.2, 0.3], [-0.2, 4.2, -0.4], [0.3, -0.4, 4.1]]])
E2E_Z = np.array([6, 1, 8, 1, 1])
E2E_POS = np.array([[0.4, 0.5, 0.3], [1.3, 1.1, 1.0], [0.6, 0.4, 0.5], [1.4, 0.9, 0.8], [0.1, 1.2, 0.2]])
E2E_BATCH = np.array([0, 0, 1, 1, 1])
E2E_S = (3, 3, 3)
E2E_DELTA = 0.01
E2E_RANGES = ((0, 2), (2, 5))


@pytest.fixture(scope='module')
def e2e():
    model = make_model(util.load_state('rand'))
    z, batch = torch.tensor(E2E_Z), torch.tensor(E2E_BATCH)
    pos, cell = torch.tensor(E2E_POS, dtype=torch.float32), torch.tensor(E2E_CELLS, dtype=torch.float32)
    args = [t.cuda() for t in (z, pos, cell, batch)]
    p = model.phonons(*args, supercell=E2E_S)
    g = {form: model.gruneisen(*args, supercell=E2E_S, strain=form, delta=E2E_DELTA, phonons=p) for form in ('volume', 'voigt')}
    cases, planes = [], {form: [] for form in g}
    for b, (lo, hi) in enumerate(E2E_RANGES):
        m = np.array([vr.MASSES[int(x)] for x in E2E_Z[lo:hi]], dtype=np.float32)
        cases.append((p.force_constants(b).cpu().numpy(), pos[lo:hi].double().numpy(), cell[b].double().numpy(), E2E_S, m))
        o, n, N = p._fc_offsets[b], p.counts[b], p.sc_counts[b]
        for form in g:
            planes[form].append(g[form].dfc[:, o:o + 9 * n * N].cpu().numpy().reshape(-1, n, 3, N, 3))
    return dict(model=model, args=args, p=p, g=g, cases=cases, planes=planes)


def test_end_to_end_planes_are_the_central_difference_of_the_strained_force_constants(e2e):
    model, (z, pos, cell, batch), p = e2e['model'], e2e['args'], e2e['p']
    assert e2e['g']['volume'].phonons is p and tuple(e2e['g']['volume'].dfc.shape) == (1, p.fc.numel())
    assert tuple(e2e['g']['voigt'].dfc.shape) == (6, p.fc.numel()) and e2e['g']['voigt'].form == 'voigt'
    _, copies = gn.strained_crystals(pos, cell, batch, 'volume', E2E_DELTA)
    fm, fp = (model.phonons(z, c[0], c[1], batch, supercell=E2E_S).fc for c in copies[0])
    want = ((fp.double() - fm.double()) / (2.0 * E2E_DELTA)).float()
    assert torch.equal(e2e['g']['volume'].dfc[0], want)
    # the sum rule holds on the plane as on the force constants: each of Phi+- obeys it to the rounding of its self block, eps32 / 2
    # of |Phi|, and the plane's own rounding to fp32 adds eps32 / 2 of |plane| per term
    for b in range(2):
        pl = e2e['planes']['volume'][b][0].astype(np.float64)
        allowed = 2 * EPS32 * float(p.fc.abs().max()) / E2E_DELTA + pl.shape[2] * EPS32 * np.abs(pl).max()
        assert np.abs(pl.sum(axis=2)).max() <= allowed
    # 'voigt': the strained crystals are rotated; the force constants go back per block in fp64 before the difference
    eps, copies = gn.strained_crystals(pos, cell, batch, 'voigt', E2E_DELTA)
    scale = float(p.fc.abs().max())
    for J in (0, 3, 5):
        back = []
        for pc, cc, Q in copies[J]:
            one = model.phonons(z, pc, cc, batch, supercell=E2E_S)
            back.append(np.concatenate([gr.rotate_back(one.force_constants(b).cpu().numpy(), Q[b]).ravel() for b in range(2)]))
        want = (back[1] - back[0]) / (2.0 * E2E_DELTA)
        err = np.abs(e2e['g']['voigt'].dfc[J].cpu().numpy().astype(np.float64) - want).max()
        print(f'voigt plane {J}: |dfc - reference| = {err:.3e}, allowed {4 * EPS32 * scale / E2E_DELTA:.3e}')
        assert err <= 4 * EPS32 * scale / E2E_DELTA


def assert_bound_is_tight(refs, what):
    """the condition tests/test_gruneisen_host.py holds on the analytic inputs, on inputs that exist on the device only"""
    ratio = [(gr.error_bound(gr.BOUND_C, r)[r['defined']] / np.abs(r['dlam']).max()).max() for r in refs]
    print(f'{what}: bound / largest |dlam| = {max(ratio):.2e} at most')
    assert max(ratio) <= 0.01, (what, ratio)


@pytest.mark.parametrize('form', ['volume', 'voigt'])
def test_end_to_end_slopes_against_the_reference(e2e, form):
    q = np.random.default_rng(23).uniform(-0.5, 0.5, (6, 3))
    bands = e2e['g'][form].frequencies(q)
    for b in range(2):
        refs = references(e2e['cases'][b], e2e['planes'][form][b], q)
        assert_bound_is_tight(refs, f'{form}, crystal {b}')
        check_against(refs, bands, b, what=f'end to end {form}, crystal {b}')


def test_central_difference_is_second_order_in_the_reference():
    """Reference against reference in fp64 (the oracle's Hessian columns on the CPU), nothing from the kernel: the perturbative gamma
    from dfc = (Phi+ - Phi-) / (2 delta) against -(lambda+ - lambda-) / (4 delta lambda0) from the eigenvalues of D built from
    Phi+-.  Both are central differences, so their difference falls by four (asserted: by three at least) from delta = 0.04 to 0.02.
    'volume', modes whose gap to their neighbours exceeds 1 % of max |lambda| (six of nine at each q).

    Crystal 1 at three q chosen with the oracle on the CPU.  The random model's crystals are no minima: their spectra are indefinite
    with eigenvalues down to 1e-3 of the largest and |gamma| up to several hundred there, so such a lambda changes by its own size
    within delta = 0.04 and the expansion in delta has not reached its asymptotic regime.  Those modes are the ones the gap rule
    removes at these q; crystal 0 has five of its six eigenvalues below a quarter of the largest and |gamma| up to 23, and its
    differences fall by 0.9 .. 3.6 only.  Measured here (per kept mode, delta 0.04 against 0.02): 3.25 .. 4.42, 3.41 .. 4.25 and
    3.51 .. 6.29."""
    sd = util.load_state('rand')
    lo, hi = E2E_RANGES[1]
    z, pos0, cell0 = E2E_Z[lo:hi], f32(E2E_POS[lo:hi]), f32(E2E_CELLS[1])
    m = np.array([vr.MASSES[int(x)] for x in z], dtype=np.float64)

    def phi(pos, cell):
        zs, ps, cs = pr.build_supercell(z, pos, cell, E2E_S)
        cols = hr.oracle_hessian_columns(sd, torch.tensor(zs), torch.tensor(ps), torch.tensor(cs)[None], torch.zeros(len(zs), dtype=torch.long),
                                         range(3 * (hi - lo)))
        return cols.numpy().reshape(hi - lo, 3, len(zs), 3)

    table = pr.image_table_fast(pos0, cell0, E2E_S)
    fc0 = phi(pos0, cell0)
    q = np.array([[0.21, -0.13, 0.37], [0.19, 0.14, -0.37], [-0.39, 0.15, 0.35]])
    diff = {}
    for delta in (0.04, 0.02):
        (pm, cm, _), (pp, cp, _) = gr.strained_crystal(pos0, cell0, 'volume', delta)[0]
        fm, fp = phi(pm, cm), phi(pp, cp)
        out = []
        for x in q:
            r = gr.problem(fc0, ((fp - fm) / (2.0 * delta))[None], pos0, cell0, E2E_S, m, x, table=table)
            lam_m, lam_p = (np.linalg.eigvalsh(pr.dynamical_matrix(f, pos0, cell0, E2E_S, m, x, table)) for f in (fm, fp))
            fd = -(lam_p - lam_m) / (4.0 * delta * r['lam'])
            gap = np.minimum(np.diff(r['lam'], prepend=-np.inf), np.diff(r['lam'], append=np.inf))
            keep = (gap > 0.01 * np.abs(r['lam']).max()) & r['defined']
            assert keep.sum() * 2 >= len(keep), f'q {x}: only {keep.sum()} of {len(keep)} modes are isolated'
            out.append(np.where(keep, np.abs(r['gamma'][:, 0] - fd), np.nan))
        diff[delta] = np.array(out)
    for k in range(len(q)):
        big, small = np.nanmax(diff[0.04][k]), np.nanmax(diff[0.02][k])
        print(f'q {q[k]}: |gamma_pert - gamma_fd| = {big:.3e} at delta = 0.04, {small:.3e} at 0.02, ratio {big / small:.2f}; per mode '
              f'{diff[0.04][k] / diff[0.02][k]}')
        assert small * 3.0 <= big
        assert np.all((diff[0.02][k] * 3.0 <= diff[0.04][k]) | np.isnan(diff[0.02][k]))


def test_mean_and_thermal_expansion_against_the_reference(e2e):
    """Every term c_v gamma carries the relative error of fp32 eigenpairs, of the order d eps32 lambda_max / lambda <= 1e-5 on the modes a
    4^3 mesh keeps (the argument of the transport-tensor test): 1e-4 of the largest element."""
    model, args = e2e['model'], e2e['args']
    el = model.elastic_constants(*args, supercell=E2E_S, phonons=e2e['p'])
    C = el.C.double().cpu().numpy()
    alpha = {}
    for form in ('volume', 'voigt'):
        mesh = e2e['g'][form].mesh(4, 4, 4)
        mean, a = mesh.mean(300.0), mesh.thermal_expansion(300.0, elastic=el)
        K = 1 if form == 'volume' else 6
        assert tuple(mean.shape) == (2, K) and mean.dtype == torch.float32
        assert tuple(a.shape) == ((2,) if form == 'volume' else (2, 6)) and a.dtype == torch.float32
        assert torch.equal(a, mesh.thermal_expansion(300.0, elastic=el.C))
        thr = mesh.threshold().cpu().numpy()
        for b in range(2):
            refs = references(e2e['cases'][b], e2e['planes'][form][b], mesh.bands.q)
            ev, gam, ok = (np.stack([r[k] for r in refs]) for k in ('lam', 'gamma', 'defined'))
            vol = abs(np.linalg.det(e2e['cases'][b][2]))
            want_m = gr.mean(ev, gam, ok, 300.0, float(thr[b]))
            want_a = np.atleast_1d(gr.thermal_expansion(ev, gam, ok, 300.0, float(thr[b]), vol, C[b], form))
            got_m, got_a = mean[b].cpu().numpy().astype(np.float64), np.atleast_1d(a[b].cpu().numpy().astype(np.float64))
            print(f'{form}, crystal {b}: mean gamma {want_m}, alpha {want_a} 1/K; largest differences '
                  f'{np.abs(got_m - want_m).max() / np.abs(want_m).max():.2e}, {np.abs(got_a - want_a).max() / np.abs(want_a).max():.2e}')
            assert np.abs(got_m - want_m).max() <= 1e-4 * np.abs(want_m).max()
            assert np.abs(got_a - want_a).max() <= 1e-4 * np.abs(want_a).max()
        alpha[form] = a.cpu().numpy()
    # the two forms differ by O(delta^2) and by B_Voigt against S: printed, not asserted
    print(f'alpha_V: volume form {alpha["volume"]}, voigt form alpha_1 + alpha_2 + alpha_3 = {alpha["voigt"][:, :3].sum(axis=1)}')
    with pytest.raises(ValueError, match='temperature'):
        mesh.mean(0.0)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_come_from_the_host_checks_without_a_launch():
    import ctypes
    lib = hip.lib()
    one = ctypes.c_void_p(8)            # never dereferenced: every refusal below comes before any launch
    ok = (ctypes.c_int32 * 2)(0, 2)

    def call(n_planes=1, cry=ok, n_cry=1, **null):
        a = dict(dfc=one, n_planes=n_planes, stride=0, split=one, fc_ptr=one, cry_ptr=one, cry_host=cry, sc=one, img_ptr=one, img_start=one,
                 img_off=one, masses=None, out_ptr=one, n_cry=n_cry, q=one, n_q=1, evals=one, modes=one, deg=one, zero=one, dlam=one,
                 gamma=one, group=None, defined=one, status=one, stream=None)
        a.update(null)
        return lib.nnhip_phonon_strain_slopes(*a.values()), lib.nnhip_last_error().decode()

    rc, msg = call(n_planes=7)
    assert rc == 1 and '7' in msg and '1 .. 6' in msg
    assert call(n_planes=0)[0] == 1
    big = (ctypes.c_int32 * 2)(0, ph.max_dim_large() // 3 + 1)
    rc, msg = call(cry=big)
    assert rc == 2 and str(ph.max_dim_large()) in msg and 'crystal 0' in msg
    many = (ctypes.c_int32 * 65537)()
    rc, msg = call(cry=many, n_cry=65536)
    assert rc == 2 and '65535' in msg and '65536' in msg
    down = (ctypes.c_int32 * 3)(0, 2, 1)
    rc, msg = call(cry=down, n_cry=2)
    assert rc == 1 and 'decreases at crystal 1' in msg
    for k in ('dfc', 'split', 'evals', 'modes', 'dlam', 'gamma', 'defined', 'status'):
        assert call(**{k: None})[0] == 1, k
    assert call(n_cry=0)[0] == 0          # no crystals: nothing to do
