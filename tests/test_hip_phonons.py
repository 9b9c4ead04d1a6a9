"""Batched phonons on the device (newtonnet_amd/phonons.py, csrc/phonon.hip) against the fp64 yardstick of tests/phonon_ref.py:
the assembly of D(q) and the complex Hermitian solver one stage at a time on planted force constants, every dimension class of
the kernel, the analytic lattice, the symmetries and the packing, and the whole chain from the model's force constants (against
the oracle's double backward, tests/hessian_ref.py) to the density of states and the thermochemistry of a mesh.

Bounds.  Assembly, per element: (n_terms + 8) eps32 sum |terms| (phonon_ref.dynamical_matrix).  Eigenvalues of a d x d problem:
vib_ref.solver_bound(2 d, ||D||_2) -- a complex rotation is the real one of the 2 d embedding -- plus the Frobenius norm of the
assembly bound (Weyl)."""
import numpy as np
import pytest
import torch

from newtonnet_amd import phonons as ph
from tests import hessian_ref as hr
from tests import phonon_ref as pr
from tests import util
from tests import vib_ref as vr
from tests.test_hip_hessian import make_model

pytestmark = pytest.mark.gpu

EPS32 = vr.EPS32
M32 = pr.TRICLINIC_MASSES.astype(np.float32)


def stage_q():
    """16 wave vectors: Gamma, a zone-boundary point, generic ones (some outside the first zone)"""
    rng = np.random.default_rng(11)
    return np.concatenate([[[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], rng.uniform(-1.0, 1.0, (14, 3))])


def triclinic_case():
    _, fc = pr.random_crystal(2, pr.TRICLINIC_S, seed=5)
    return fc.astype(np.float32), pr.TRICLINIC_POS, pr.TRICLINIC_CELL, pr.TRICLINIC_S, M32


def cubic_case():
    fc, pos, cell = pr.cubic_lattice()
    return fc.astype(np.float32), pos, cell, pr.CUBIC_S, np.array([pr.CUBIC_MASS], dtype=np.float32)


def make(case, **kw):
    fc, pos, cell, S, m = case
    return ph.Phonons.from_force_constants(fc, np.ones(len(pos), dtype=np.int64), pos, cell, S, masses=m, device='cuda', **kw)


def reference(case, q):
    """[(D fp64, assembly bound)] per q, from the force constants and masses as the device holds them (fp32)"""
    fc, pos, cell, S, m = case
    table = pr.image_table(pos, cell, S)
    return [pr.dynamical_matrix(fc.astype(np.float64), pos, cell, S, m.astype(np.float64), x, table, with_bound=True) for x in q]


def eig_bound(D, B):
    return vr.solver_bound(2 * D.shape[0], np.linalg.norm(D, 2)) + np.linalg.norm(B)


def check_spectrum(D, B, ev, modes=None, what=''):
    """device eigenvalues (and modes, rows) of one problem against the fp64 D they belong to"""
    d = D.shape[0]
    bound = eig_bound(D, B)
    err = np.abs(np.asarray(ev, dtype=np.float64) - np.linalg.eigvalsh(D)).max()
    assert np.all(np.diff(ev) >= 0), f'{what}: eigenvalues not ascending'
    assert err <= bound, f'{what}: eigenvalue error {err:.3e} above the bound {bound:.3e}'
    if modes is not None:
        V = np.asarray(modes, dtype=np.complex128)
        res = np.linalg.norm(D @ V.T - V.T * np.asarray(ev, dtype=np.float64)[None, :], axis=0).max()
        orth = np.abs(V @ V.conj().T - np.eye(d)).max()
        assert res <= bound, f'{what}: residual {res:.3e} above the bound {bound:.3e}'
        assert orth <= 2 * d * EPS32 * 8, f'{what}: ||V V^H - I||_max = {orth:.3e} above {2 * d * EPS32 * 8:.3e}'
        for row in V:   # the largest component is real and positive (the device ranks |v|^2 in fp32: any of the near-largest may be it)
            top = row[np.abs(row) >= np.abs(row).max() * (1.0 - 1e-5)]
            assert np.any((top.real > 0) & (np.abs(top.imag) <= 4 * EPS32)), f'{what}: phase convention'
    return err, bound


@pytest.mark.parametrize('name', ['triclinic', 'cubic'])
def test_stage_assembly_and_solver(name):
    case = triclinic_case() if name == 'triclinic' else cubic_case()
    q = stage_q()
    p = make(case)
    bands = p.frequencies(q, modes=True, dynamical_matrix=True)
    assert int(bands.status.abs().max()) == 0
    ev, fr, modes = (x.cpu().numpy() for x in bands.crystal(0))
    Dd = bands.dynamical(0).cpu().numpy()
    ref = reference(case, q)
    worst = 0.0
    for k, (D, B) in enumerate(ref):
        diff = np.abs(Dd[k].astype(np.complex128) - D)
        assert np.all(diff <= B), f'{name} q {k}: |dD| exceeds the assembly bound by {np.max(diff - B):.3e}'
        assert np.array_equal(Dd[k], Dd[k].conj().T), 'D(q) on the device is not exactly Hermitian'
        worst = max(worst, float(np.max(diff / np.where(B > 0, B, 1.0))))
        check_spectrum(D, B, ev[k], modes[k], f'{name} q {k}')
    print(f'{name}: max |dD| / bound = {worst:.3f}')
    np.testing.assert_allclose(fr, np.sign(ev) * np.sqrt(np.abs(ev)) * vr.WAVENUMBER, rtol=1e-6)


def planted_case(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3 * n, 3 * n))
    fc = (X + X.T).astype(np.float32).reshape(n, 3, n, 3)
    pos = rng.uniform(0.0, 9.0, (n, 3))
    m = rng.choice([1.008, 12.011, 15.999], n).astype(np.float32)
    return fc, pos, 9.0 * np.eye(3) + 0.3 * rng.standard_normal((3, 3)), (1, 1, 1), m


@pytest.mark.parametrize('d', [3, 6, 9, 24, 72, 'max'])
def test_every_dimension_class(d):
    """one wave per problem up to d = 32, a workgroup above; an odd d pads; d = max_dim() fills the LDS"""
    d = ph.max_dim() if d == 'max' else d
    case = planted_case(d // 3, 100 + d)
    q = np.array([[0.0, 0.0, 0.0], [0.31, -0.17, 0.44], [-0.5, 0.25, 0.125]])
    bands = make(case).frequencies(q, modes=True)
    assert int(bands.status.abs().max()) == 0 and int(bands.sweeps.min()) >= 1
    ev, _, modes = (x.cpu().numpy() for x in bands.crystal(0))
    for k, (D, B) in enumerate(reference(case, q)):
        err, bound = check_spectrum(D, B, ev[k], modes[k], f'd = {d} q {k}')
    print(f'd = {d}: sweeps {bands.sweeps.cpu().tolist()}, last error {err:.2e} of {bound:.2e}')


def test_one_above_the_bound_is_refused_before_any_kernel():
    n = ph.max_dim() // 3 + 1
    with pytest.raises(NotImplementedError, match=r'phonons\.max_dim\(\)'):
        make(planted_case(n, 1))


def test_analytic_dispersion_on_the_device():
    case = cubic_case()
    fc = ph.acoustic_sum_rule(torch.tensor(case[0], device='cuda'))
    p = ph.Phonons.from_force_constants(fc, [1], case[1], case[2], case[3], masses=case[4])
    q = np.concatenate([[[0.0, 0.0, 0.0]], np.random.default_rng(3).uniform(-1.0, 1.0, (20, 3))])
    ev = p.frequencies(q).crystal(0)[0].cpu().numpy().astype(np.float64)
    ref = reference(case, q)
    for k, (D, B) in enumerate(ref):
        bound = eig_bound(D, B)
        assert np.abs(ev[k] - pr.cubic_omega2(q[k])).max() <= bound + 1e-12, (k, ev[k], pr.cubic_omega2(q[k]), bound)
    assert np.abs(ev[0]).max() <= eig_bound(*ref[0]), f'Gamma: {ev[0]}'


def two_crystals():
    """the triclinic d = 6 crystal (one wave per problem) and a planted d = 36 one (a workgroup per problem) as one batch"""
    a, b = triclinic_case(), planted_case(12, 7)
    p = ph.Phonons.from_force_constants([a[0], b[0]], np.ones(14, dtype=np.int64), np.concatenate([a[1], b[1]]), np.stack([a[2], b[2]]),
                                        np.array([a[3], b[3]]), masses=np.concatenate([a[4], b[4]]),
                                        batch=np.array([0] * 2 + [1] * 12), device='cuda')
    return p, a, b


def test_symmetries_packing_and_repeatability():
    p, a, b = two_crystals()
    rng = np.random.default_rng(17)
    q = rng.uniform(-0.5, 0.5, (1000, 3))
    big = p.frequencies(q, modes=True)
    assert int(big.status.abs().max()) == 0
    again = p.frequencies(q, modes=True)
    assert torch.equal(big.eigenvalues, again.eigenvalues) and torch.equal(torch.view_as_real(big.modes), torch.view_as_real(again.modes))
    plain = p.frequencies(q)
    assert plain.modes is None and torch.equal(plain.eigenvalues, big.eigenvalues) and torch.equal(plain.sweeps, big.sweeps)
    # each q alone, each crystal alone: the same bits as in the launch of 2 x 1000
    # (every q for the packed crystal, whose neighbours in the workgroup change; a few for the one that owns its workgroup)
    alone = [make(a), make(b)]
    for k in range(1000):
        for c in ((0, 1) if k in (0, 1, 2, 3, 501, 998, 999) else (0,)):
            one = alone[c].frequencies(q[k:k + 1], modes=True)
            assert torch.equal(one.crystal(0)[0][0], big.crystal(c)[0][k]), (k, c)
            assert torch.equal(torch.view_as_real(one.crystal(0)[2][0]), torch.view_as_real(big.crystal(c)[2][k])), (k, c)
            assert int(one.sweeps[0, 0]) == int(big.sweeps[c, k])
    # q, -q and q + G
    qs = q[:8]
    G = np.array([1.0, -2.0, 1.0])
    e0, e1, e2 = (p.frequencies(x).crystal(0)[0].cpu().numpy().astype(np.float64) for x in (qs, -qs, qs + G))
    for k, (D, B) in enumerate(reference(a, qs)):
        bound = eig_bound(D, B)
        assert np.abs(e0[k] - e1[k]).max() <= 2 * bound and np.abs(e0[k] - e2[k]).max() <= 2 * bound, (k, e0[k], e1[k], e2[k], bound)


def test_band_structure_path():
    p = make(triclinic_case())
    points = [[0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0], [0, 0, 0]]
    bands = p.band_structure(points, 5)
    q, length, ticks = pr.band_path(points, 5, pr.TRICLINIC_CELL)
    assert bands.ticks == ticks and np.allclose(bands.q, q, atol=1e-15) and np.allclose(bands.path[0], length, rtol=1e-13)
    assert torch.equal(bands.eigenvalues, p.frequencies(q).eigenvalues)
    ev = bands.crystal(0)[0]
    assert tuple(ev.shape) == (16, 6) and torch.equal(ev[0], ev[15])            # the path returns to Gamma


def test_dos_and_thermochemistry_of_a_mesh():
    p, a, b = two_crystals()
    mesh = p.mesh(4, 4, 4)
    Q, dims = 64, (6, 36)
    ev = [mesh.bands.crystal(c)[0].cpu().numpy() for c in range(2)]
    fr = [mesh.bands.crystal(c)[1].cpu().numpy().astype(np.float64) for c in range(2)]
    # histogram: integer counts, every mode once
    hist = mesh.dos(50)
    assert hist.counts.dtype == torch.int32 and hist.counts.sum(dim=1).tolist() == [Q * d for d in dims]
    np.testing.assert_allclose((hist.dos.double().sum(dim=1) * hist.bin_width).cpu().numpy(), dims, rtol=1e-6)
    edges = hist.lo + hist.bin_width * np.arange(51)
    for c in range(2):
        want, _ = np.histogram(fr[c], bins=edges)
        got = hist.counts[c].cpu().numpy()
        assert np.abs(got - want).sum() <= 2 * 2, 'more than two values moved to a neighbouring bin (fp32 against fp64 bin edges)'
    assert torch.equal(mesh.dos(50).counts, hist.counts)
    # Gaussian smearing
    width = float(max(f.max() for f in fr) - min(f.min() for f in fr)) / 20.0
    g = mesh.dos(400, width=width)
    np.testing.assert_allclose((g.dos.double().sum(dim=1) * g.bin_width).cpu().numpy(), dims, rtol=1e-4)
    centres = g.frequencies.cpu().numpy().astype(np.float64)
    for c in range(2):
        want = np.exp(-0.5 * ((centres[:, None] - fr[c].reshape(-1)[None, :]) / width) ** 2).sum(axis=1) / (width * np.sqrt(2 * np.pi) * Q)
        np.testing.assert_allclose(g.dos[c].cpu().numpy(), want, rtol=1e-4, atol=1e-6 * want.max())
    # thermochemistry: the yardstick's formulas on the device's eigenvalues
    thr = mesh.threshold().cpu().numpy()
    for T in (300.0, 0.0):
        t = mesh.thermochemistry(T)
        for c in range(2):
            np.testing.assert_allclose(thr[c], 8 * EPS32 * 2 * dims[c] * np.abs(ev[c]).max(), rtol=1e-6)
            want = pr.thermochemistry(ev[c], T, float(thr[c]))
            for key in ('ZPE', 'U', 'S', 'F', 'Cv'):
                np.testing.assert_allclose(float(getattr(t, key)[c]), want[key], rtol=1e-5, atol=0, err_msg=f'{key} crystal {c} T {T}')
            assert int(t.n_skipped_imaginary[c]) == want['n_imag'] > 0 and int(t.n_skipped_zero[c]) == want['n_zero']
    # the cubic lattice: a branch is zero wherever its q component is, 3 x 16 modes of the 4^3 mesh, and nothing is imaginary
    cub = make(cubic_case()).mesh(4, 4, 4).thermochemistry(300.0)
    assert int(cub.n_skipped_zero[0]) == 48 and int(cub.n_skipped_imaginary[0]) == 0


# ---- end to end with the model -----------------------------------------------------------------------------------------------

# triclinic, and SYMMETRIC as matrices: the model's minimum-image shift is a lattice vector for such a cell only (phonons.phonons)
E2E_CELLS = np.array([[[4.2, 0.4, -0.3], [0.4, 4.1, 0.5], [-0.3, 0.5, 4.3]],
                      [[4.3, -0.2, 0.3], [-0.2, 4.2, -0.4], [0.3, -0.4, 4.1]]])
E2E_Z = np.array([6, 1, 8, 1, 1])
E2E_POS = np.array([[0.4, 0.5, 0.3], [1.3, 1.1, 1.0], [0.6, 0.4, 0.5], [1.4, 0.9, 0.8], [0.1, 1.2, 0.2]])
E2E_BATCH = np.array([0, 0, 1, 1, 1])
E2E_S = (3, 3, 3)


@pytest.fixture(scope='module')
def e2e():
    sd = util.load_state('rand')
    model = make_model(sd)
    z, batch = torch.tensor(E2E_Z), torch.tensor(E2E_BATCH)
    pos, cell = torch.tensor(E2E_POS, dtype=torch.float32), torch.tensor(E2E_CELLS, dtype=torch.float32)
    args = [t.cuda() for t in (z, pos, cell, batch)]
    raw = model.phonons(*args, supercell=E2E_S, asr=False)
    asr = model.phonons(*args, supercell=E2E_S)
    # the oracle's columns of the home atoms, crystal by crystal (fp64 double backward on the supercell the device saw)
    oracle = []
    for b, (lo, hi) in enumerate(((0, 2), (2, 5))):
        zs, ps, cs = pr.build_supercell(E2E_Z[lo:hi], pos[lo:hi].double().numpy(), cell[b].double().numpy(), E2E_S)
        ps32 = torch.tensor(ps, dtype=torch.float32)
        cols = hr.oracle_hessian_columns(sd, torch.tensor(zs), ps32.double(), torch.tensor(cs, dtype=torch.float32).double()[None],
                                         torch.zeros(len(zs), dtype=torch.long), range(3 * (hi - lo)))
        oracle.append(cols.numpy().reshape(hi - lo, 3, len(zs), 3))
    return dict(sd=sd, model=model, args=args, raw=raw, asr=asr, oracle=oracle, pos=pos, cell=cell)


def e2e_case(e, b, fc):
    lo, hi = ((0, 2), (2, 5))[b]
    m = np.array([vr.MASSES[int(x)] for x in E2E_Z[lo:hi]], dtype=np.float32)
    return (np.asarray(fc), e['pos'][lo:hi].double().numpy(), e['cell'][b].double().numpy(), E2E_S, m)


def test_force_constants_against_the_oracle(e2e):
    assert e2e['raw'].counts == [2, 3] and e2e['raw'].sc_counts == [54, 81]
    for b in range(2):
        got = e2e['raw'].force_constants(b).cpu().double().numpy()
        want = e2e['oracle'][b]
        scale = np.abs(want).max()
        d = np.abs(got - want)
        print(f'crystal {b}: max |dPhi| {d.max():.3e}, mean {d.mean():.3e} of {scale:.3e}')
        assert d.max() <= 1e-4 * scale and d.mean() <= 1e-5 * scale
        # the acoustic sum rule changes the self blocks only, and as stated
        asr = e2e['asr'].force_constants(b)
        assert torch.allclose(asr, ph.acoustic_sum_rule(e2e['raw'].force_constants(b)), rtol=0, atol=0)
    assert torch.equal(e2e['model'].phonons(*e2e['args'], supercell=E2E_S, asr=False).fc, e2e['raw'].fc)


def asr64(phi):
    phi = np.array(phi, dtype=np.float64)
    for i in range(phi.shape[0]):
        blk = phi[i, :, i, :] - phi[i].sum(axis=1)
        phi[i, :, i, :] = 0.5 * (blk + blk.T)
    return phi


def test_end_to_end_eigenvalues_against_the_oracle(e2e):
    q = np.concatenate([[[0.0, 0.0, 0.0]], np.random.default_rng(23).uniform(-0.5, 0.5, (7, 3))])
    bands = e2e['asr'].frequencies(q)
    assert int(bands.status.abs().max()) == 0
    for b in range(2):
        ev = bands.crystal(b)[0].cpu().numpy().astype(np.float64)
        dev_case = e2e_case(e2e, b, e2e['asr'].force_constants(b).cpu().numpy())
        ora_case = e2e_case(e2e, b, asr64(e2e['oracle'][b]))
        table = pr.image_table(dev_case[1], dev_case[2], E2E_S)
        for k, x in enumerate(q):
            Dd, B = pr.dynamical_matrix(dev_case[0].astype(np.float64), dev_case[1], dev_case[2], E2E_S, dev_case[4].astype(np.float64), x,
                                        table, with_bound=True)
            Do = pr.dynamical_matrix(ora_case[0], ora_case[1], ora_case[2], E2E_S, ora_case[4].astype(np.float64), x, table)
            bound = eig_bound(Dd, B) + np.linalg.norm(Dd - Do, 2)
            err = np.abs(ev[k] - np.linalg.eigvalsh(Do)).max()
            assert err <= bound, f'crystal {b} q {k}: {err:.3e} above {bound:.3e}'
        # Gamma with the sum rule: three acoustic modes within the bound of zero
        D0, B0 = pr.dynamical_matrix(dev_case[0].astype(np.float64), dev_case[1], dev_case[2], E2E_S, dev_case[4].astype(np.float64), q[0],
                                     table, with_bound=True)
        assert np.sum(np.abs(ev[0]) <= eig_bound(D0, B0)) >= 3, ev[0]


def test_commensurate_union_against_the_supercell_hessian(e2e):
    """the 27 commensurate q of the 3 x 3 x 3 supercell carry the spectrum of the supercell's own mass-weighted Hessian"""
    model, (z, pos, cell, batch) = e2e['model'], e2e['args']
    ev = e2e['raw'].mesh(3, 3, 3).bands
    for b, (lo, hi) in enumerate(((0, 2), (2, 5))):
        zs, ps, cs = pr.build_supercell(E2E_Z[lo:hi], e2e['pos'][lo:hi].double().numpy(), e2e['cell'][b].double().numpy(), E2E_S)
        N = len(zs)
        H = model.hessian(torch.tensor(zs).cuda(), torch.tensor(ps, dtype=torch.float32).cuda(),
                          torch.tensor(cs, dtype=torch.float32).cuda()[None], torch.zeros(N, dtype=torch.long).cuda())
        A = vr.mass_weighted(H.cpu().double().numpy(), [vr.MASSES[int(x)] for x in zs])
        want = np.linalg.eigvalsh(A)
        got = np.sort(ev.crystal(b)[0].cpu().numpy().astype(np.float64).reshape(-1))
        bound = vr.solver_bound(3 * N, np.abs(want).max())
        err = np.abs(got - want).max()
        print(f'crystal {b}: union error {err:.3e}, bound {bound:.3e}')
        assert got.shape == want.shape == (3 * N,) and err <= bound


def test_width_check_on_the_device_model(e2e):
    with pytest.raises(ValueError, match='widths'):
        e2e['model'].phonons(*e2e['args'], supercell=(1, 1, 1))
    with pytest.raises(ValueError, match='widths'):
        e2e['model'].phonons(*e2e['args'], supercell=torch.tensor([[3, 3, 3], [3, 2, 3]]))


def test_calculator_phonons_agree_with_the_model():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    sd = util.load_state('rand', torch.float32)
    calc = MLAseCalculator(sd, properties=['energy', 'forces'], device='cuda')
    frames = [FakeAtoms(E2E_Z[lo:hi], E2E_POS[lo:hi], cell=E2E_CELLS[b], pbc=(True, True, True)) for b, (lo, hi) in enumerate(((0, 2), (2, 5)))]
    q = np.array([[0.0, 0.0, 0.0], [0.2, 0.1, -0.4]])
    both = calc.phonons(frames, E2E_S)
    z, pos, cell, batch = calc.format_data(frames)
    direct = calc.model.phonons(z, pos, cell, batch, E2E_S)
    assert torch.equal(both.fc, direct.fc) and torch.equal(both.frequencies(q).eigenvalues, direct.frequencies(q).eigenvalues)
    one = calc.phonons(frames[0], E2E_S)
    assert one.counts == [2] and tuple(one.frequencies(q).crystal(0)[0].shape) == (2, 6)
