"""CPU-side checks of the elastic-constant feature (newtonnet_amd/elastic.py, csrc/elastic.hip): the build plumbing, the fp64
yardstick of the GPU tests (tests/elastic_ref.py) against central differences of the oracle's energy and against its virial,
the condition of the test crystals, the host helpers, and every argument check before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from newtonnet_amd import elastic as el
from newtonnet_amd import hessian as nh
from oracle import newtonnet_ref as ref
from tests import elastic_ref as er
from tests import hessian_ref as hr
from tests import util
from tests.test_phonon_host import _FakeModel, _crystal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_symbols_are_declared_listed_and_exported():
    from newtonnet_amd import abi, hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for name in ('nnhip_strain_vp', 'nnhip_elastic_fold', 'nnhip_elastic_relax'):
        assert name in declared and name in abi.FUNCTIONS and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\belastic\b.*\)', f.read(), re.M)
    assert el.STATUS_ZERO == 1 and el.STATUS_NEGATIVE == 2 and el.max_dim() == 96 and abi.CONSTANTS['NNHIP_ELASTIC_STATUS_SIZE'] == 8
    # argument checks of the library itself, before any launch
    hip.abi.bind(lib, ('nnhip_strain_vp', 'nnhip_elastic_fold', 'nnhip_elastic_relax', 'nnhip_last_error'))
    one = ctypes.c_void_p(8)
    assert lib.nnhip_elastic_fold(None, one, one, one, one, 1, one, one, None) != 0 and b'nnhip_elastic_fold' in lib.nnhip_last_error()
    assert lib.nnhip_elastic_fold(one, one, one, one, one, 1, one, None, None) != 0          # the status array is not optional
    assert lib.nnhip_elastic_relax(one, one, one, one, one, None, 1, one, one, one, one, None) != 0
    assert b'nnhip_elastic_relax' in lib.nnhip_last_error()
    assert lib.nnhip_elastic_fold(None, None, None, None, None, 0, None, None, None) == 0
    assert lib.nnhip_strain_vp(None, None, None, one, one, one, None) != 0


@pytest.fixture(scope='module')
def cubic0():
    """crystal 0 in its cubic cell: the strained oracle and its second derivatives"""
    sd = util.load_state('rand')
    z, pos, cell, batch = er.supercell(0, cells=er.CUBIC_CELLS)
    o = er.StrainedOracle(sd, z, pos, cell, batch)
    return dict(sd=sd, args=(z, pos, cell, batch), oracle=o, second=o.second(range(2)))


def test_reference_born_matrix_is_symmetric_and_matches_energy_differences(cubic0):
    """d^2E/de de of tests/elastic_ref.py (edge list frozen, displacement vectors strained) against central differences of the
    oracle's OWN energy on the strained positions and cell (graph rebuilt at every point).  The h^2 term of the central
    difference is 6.6e2 h^2 of the largest entry here (it falls by 4.00 per halving of h from 1e-3 to 1e-4), so the steps
    h = 1e-3 and h / 2 are combined by Richardson extrapolation; what is left is the h^4 term, expected at (6.6e2 h^2)^2 = 4e-7
    relative, and the rounding error 8 x 2^-53 |E| / h^2.  Allowed: 1e-5 of the largest entry plus that rounding error."""
    sd, (z, pos, cell, batch) = cubic0['sd'], cubic0['args']
    bv = cubic0['second'][0][0].numpy()
    scale = np.abs(bv).max()
    assert np.abs(bv - bv.T).max() <= 1e-10 * scale
    sdd = {k: v.double() for k, v in sd.items()}

    def energy(e):
        m = torch.eye(3, dtype=torch.float64) + torch.tensor(el.voigt_matrices(e))
        return float(hr.oracle_energy(sdd, z, pos @ m, cell @ m, batch)[0])
    h, worst = 1e-3, 0.0
    e0 = energy(np.zeros(6))
    tol = 1e-5 * scale + 8.0 * 2.0 ** -53 * abs(e0) / h ** 2

    def fd(I, J, s):
        a, b = np.zeros(6), np.zeros(6)
        a[I], b[J] = s, s
        return (energy(a + b) - energy(a - b) - energy(b - a) + energy(-a - b)) / (4.0 * s * s)
    for I in range(6):
        for J in range(I, 6):
            worst = max(worst, abs((4.0 * fd(I, J, 0.5 * h) - fd(I, J, h)) / 3.0 - bv[I, J]))
    print(f'Born matrix against central differences: max {worst:.3e} of {scale:.3e} (tolerance {tol:.3e})')
    assert worst <= tol


def test_reference_matches_energy_differences_in_the_triclinic_test_cell():
    """The same check on E2E crystal 0 in its own (symmetric triclinic) cell, the cell the GPU tests use.  The oracle's energy on
    pos @ m, cell @ m is NOT the homogeneously strained crystal there: cell @ m is no symmetric matrix, so the image shift
    (cell m) n is no vector of the strained lattice m (cell n) -- its derivative is the oracle's virial (next test).  The strained
    crystal is therefore rotated rigidly back to a symmetric cell (phonons.symmetric_cell, the polar decomposition; the energy does
    not change under a rotation), where the oracle's shift is a lattice vector.  First derivative, all six components, and the
    second for six (I, J) pairs; steps and tolerances as above (the first derivative's h^2 term goes by Richardson as well)."""
    from newtonnet_amd import phonons as ph
    sd = util.load_state('rand')
    sdd = {k: v.double() for k, v in sd.items()}
    z, pos, cell, batch = er.supercell(0)
    o = er.StrainedOracle(sd, z, pos, cell, batch)
    ge = o.first()[0][0].numpy()
    bv = er.elastic_reference(sd, 0)['bornV']

    def energy(e):
        m = np.eye(3) + el.voigt_matrices(e)
        p, c = ph.symmetric_cell(pos.numpy() @ m, cell[0].numpy() @ m)
        return float(hr.oracle_energy(sdd, z, torch.tensor(p), torch.tensor(c)[None], batch)[0])
    h = 1e-3
    e0 = energy(np.zeros(6))

    def unit(I, s):
        a = np.zeros(6)
        a[I] = s
        return a

    def fd1(I, s):
        return (energy(unit(I, s)) - energy(unit(I, -s))) / (2.0 * s)

    def fd2(I, J, s):
        a, b = unit(I, s), unit(J, s)
        return (energy(a + b) - energy(a - b) - energy(b - a) + energy(-a - b)) / (4.0 * s * s)
    err1 = max(abs((4.0 * fd1(I, 0.5 * h) - fd1(I, h)) / 3.0 - ge[I]) for I in range(6))
    tol1 = 1e-5 * np.abs(ge).max() + 8.0 * 2.0 ** -53 * abs(e0) / h
    pairs = ((0, 0), (0, 1), (1, 2), (3, 3), (2, 4), (4, 5))
    err2 = max(abs((4.0 * fd2(I, J, 0.5 * h) - fd2(I, J, h)) / 3.0 - bv[I, J]) for I, J in pairs)
    tol2 = 1e-5 * np.abs(bv).max() + 8.0 * 2.0 ** -53 * abs(e0) / h ** 2
    print(f'triclinic cell: dE/de against differences {err1:.3e} of {np.abs(ge).max():.3e} (tolerance {tol1:.3e}); '
          f'd2E/de de {err2:.3e} of {np.abs(bv).max():.3e} (tolerance {tol2:.3e})')
    assert err1 <= tol1 and err2 <= tol2
    # ... and the plain pos @ m, cell @ m energy differs from it at first order in the strain
    m = np.eye(3) + el.voigt_matrices(unit(0, h))
    plain = float(hr.oracle_energy(sdd, z, pos @ torch.tensor(m), cell @ torch.tensor(m), batch)[0])
    assert abs(plain - energy(unit(0, h))) > 1e-3 * h * np.abs(ge).max()


def test_first_strain_derivative_is_minus_the_virial_in_cubic_cells():
    """dE/de_I = -virial (Voigt) of the oracle where the cell commutes with the strain.  The oracle (as the reference) strains the
    image shift as (cell S) n, which equals S (cell n) only for such cells: on the symmetric triclinic E2E cells the two first
    derivatives differ by a few per cent (printed), which is why this identity is checked on the cubic variants."""
    sd = util.load_state('rand')
    sdd = {k: v.double() for k, v in sd.items()}
    for cells, exact in ((er.CUBIC_CELLS, True), (er.E2E_CELLS, False)):
        for b in range(2):
            z, pos, cell, batch = er.supercell(b, cells=cells)
            ge, gu = er.StrainedOracle(sd, z, pos, cell, batch).first()
            out = ref.energy_forces(sdd, z, pos, cell, batch)
            want = -np.array([out['virial'][0][a, c].item() for a, c in er.VOIGT_PAIRS])
            err = np.abs(ge[0].numpy() - want).max() / np.abs(want).max()
            print(f'{"cubic" if exact else "E2E"} crystal {b}: |dE/de + virial| / max = {err:.3e}')
            assert (gu + out['forces']).abs().max().item() <= 1e-12
            if exact:
                assert err <= 1e-10


def test_test_crystals_are_well_conditioned_for_the_relaxed_term():
    """the end-to-end GPU test inverts Phi0 over its non-acoustic modes: the smallest of them is at least 1e-2 of the largest, and
    the three acoustic ones are far below (the sum rule)"""
    sd = util.load_state('rand')
    for b in range(2):
        r = er.elastic_reference(sd, b)
        w = np.sort(np.abs(r['evals']))
        print(f'crystal {b}: |lambda| {w}')
        assert w[3] >= 1e-2 * w[-1] and w[2] <= 1e-9 * w[-1]
        assert np.abs(r['C'] - r['C'].T).max() <= 1e-10 * np.abs(r['C']).max()
        # translation invariance: exact over the supercell; over the home atoms alone up to the fp32 rounding of the supercell's
        # positions (the copies of an atom sit 2^-24 x 12 A off the lattice), printed
        scale = np.abs(r['lam_sc']).max()
        assert np.abs(r['lam_sc'].sum(axis=0)).max() <= 1e-9 * scale
        print(f'crystal {b}: |sum of Lambda over the home atoms| = {np.abs(r["lam"].reshape(-1, 3, 6).sum(axis=0)).max():.3e} of {scale:.3e}')
        assert np.abs(r['lam'].reshape(-1, 3, 6).sum(axis=0)).max() <= 1e-4 * scale


def _result(C):
    C = torch.tensor(np.asarray(C), dtype=torch.float32).reshape(-1, 6, 6)
    return el.ElasticConstants(C=C, born=C, relaxation=torch.zeros_like(C))


def test_moduli_helpers_on_a_cubic_crystal():
    c11, c12, c44 = 1.05, 0.40, 0.50          # eV / A^3 (all three exact in fp32 to 1e-7)
    res = _result(er.cubic_matrix(c11, c12, c44))
    K, GV, GR = er.cubic_moduli(c11, c12, c44)
    kv, kr, kh = (float(x[0]) for x in res.bulk_modulus())
    gv, gr, gh = (float(x[0]) for x in res.shear_modulus())
    assert abs(kv - K) <= 1e-6 and abs(kr - K) <= 1e-6 and abs(kh - K) <= 1e-6
    assert abs(gv - GV) <= 1e-6 and abs(gr - GR) <= 1e-6 and abs(gh - 0.5 * (GV + GR)) <= 1e-6
    E, nu = 9 * K * gh / (3 * K + gh), (3 * K - 2 * gh) / (2 * (3 * K + gh))
    assert abs(float(res.youngs_modulus()[0]) - E) <= 1e-6 and abs(float(res.poisson_ratio()[0]) - nu) <= 1e-6
    assert torch.allclose(res.compliance()[0] @ res.C[0].double(), torch.eye(6, dtype=torch.float64), atol=1e-6)
    assert abs(float(res.stability()[0]) - min(c11 - c12, c44, c11 + 2 * c12)) <= 1e-6
    assert float(_result(er.cubic_matrix(0.3, 0.4, 0.5)).stability()[0]) < 0          # c11 < c12: unstable
    assert el.GPA_PER_EV_A3 == er.GPA_PER_EV_A3 == 160.21766
    assert torch.allclose(res.gpa(), res.C.double() * 160.21766, rtol=1e-15)


def test_voigt_packing():
    eps = np.array([[0.01, 0.02, -0.03], [0.02, 0.04, 0.05], [-0.03, 0.05, -0.06]])
    e = nh.voigt_strain(torch.tensor(eps)[None], 1)[0].numpy()
    assert np.allclose(e, [0.01, 0.04, -0.06, 0.10, -0.06, 0.04], atol=1e-15)
    assert np.array_equal(e, er.voigt_of(eps))
    assert np.allclose(el.voigt_matrices(e), eps, atol=1e-15)
    assert np.allclose(er.voigt_matrix(torch.tensor(e)).numpy(), eps, atol=1e-15)
    six = torch.arange(12.0).reshape(2, 6)
    assert nh.voigt_strain(six, 2) is not None and torch.equal(nh.voigt_strain(six, 2), six)
    assert el.VOIGT_PAIRS == er.VOIGT_PAIRS


def test_argument_errors_come_before_any_kernel():
    from newtonnet_amd.models.newtonnet import NewtonNet
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    assert callable(NewtonNet.elastic_constants) and callable(NewtonNet.strain_vector_product)
    assert callable(MLAseCalculator.elastic_constants)
    z, pos, cell, batch = _crystal()
    ok, train, no_energy = _FakeModel(), _FakeModel(), _FakeModel()
    train.training = True
    no_energy.output_properties = ['direct_force']
    eye = torch.eye(3)[None]
    # strain_vector_product
    with pytest.raises(NotImplementedError, match='eval'):
        nh.strain_vector_product(train, z, pos, cell, batch, eye)
    with pytest.raises(NotImplementedError, match='energy'):
        nh.strain_vector_product(no_energy, z, pos, cell, batch, eye)
    skew = eye.clone()
    skew[0, 0, 1] = 0.1
    with pytest.raises(ValueError, match='not symmetric'):
        nh.strain_vector_product(ok, z, pos, cell, batch, skew)
    for bad in (torch.zeros(2, 3, 3), torch.zeros(1, 5), torch.zeros(6), torch.zeros(1, 3, 2)):
        with pytest.raises(ValueError, match='strain'):
            nh.strain_vector_product(ok, z, pos, cell, batch, bad)
    with pytest.raises(ValueError, match='expected'):
        nh.strain_vector_product(ok, z[:1], pos, cell, batch, eye)
    with pytest.raises(ValueError, match='expected'):
        nh.strain_vector_product(ok, z, pos, cell[0], batch, eye)
    with pytest.raises(RuntimeError, match='MI355X'):
        nh.strain_vector_product(ok, z, pos, cell, batch, eye)
    with pytest.raises(RuntimeError, match='MI355X'):
        nh.strain_vector_product(ok, z, pos, cell, batch, torch.zeros(1, 6))
    # elastic_constants: the checks of phonons.phonons, in its words
    with pytest.raises(NotImplementedError, match='eval'):
        el.elastic_constants(train, z, pos, cell, batch, (3, 3, 3))
    with pytest.raises(NotImplementedError, match='energy'):
        el.elastic_constants(no_energy, z, pos, cell, batch, (3, 3, 3))
    with pytest.raises(ValueError, match='zero'):
        el.elastic_constants(ok, z, pos, torch.zeros(1, 3, 3), batch, (3, 3, 3))
    tilt = cell.clone()
    tilt[0, 0, 1] = 0.4
    with pytest.raises(ValueError, match='symmetric'):
        el.elastic_constants(ok, z, pos, tilt, batch, (3, 3, 3))
    with pytest.raises(ValueError, match='supercell'):
        el.elastic_constants(ok, z, pos, cell, batch, (3, 0, 3))
    with pytest.raises(ValueError, match=r'widths 4\.200, 4\.200, 4\.200 A.*2 x cutoff = 10\.000'):
        el.elastic_constants(ok, z, pos, cell, batch)                      # the default supercell (1, 1, 1) is too narrow here
    with pytest.raises(ValueError, match=r'widths 12\.600, 8\.400, 12\.600'):
        el.elastic_constants(ok, z, pos, cell, batch, (3, 2, 3))
    with pytest.raises(ValueError, match='expected'):
        el.elastic_constants(ok, z, pos[:1], cell, batch, (3, 3, 3))
    with pytest.raises(RuntimeError, match='MI355X'):
        el.elastic_constants(ok, z, pos, cell, batch, (3, 3, 3))
    # the size limit belongs to the relaxed term alone
    zb, pb, cb, bb = _crystal(n=el.max_dim() // 3 + 1, a=12.0)
    with pytest.raises(NotImplementedError, match=r'elastic\.max_dim\(\)'):
        el.elastic_constants(ok, zb, pb, cb, bb, (1, 1, 1))
    with pytest.raises(RuntimeError, match='MI355X'):
        el.elastic_constants(ok, zb, pb, cb, bb, (1, 1, 1), relaxed=False)
    # a Phonons of other crystals
    from newtonnet_amd import phonons as ph
    from tests import phonon_ref as pr
    fc, p1, c1 = pr.cubic_lattice()
    other = ph.Phonons.from_force_constants(fc, [1], p1, c1, pr.CUBIC_S, masses=[pr.CUBIC_MASS], device='cpu')
    with pytest.raises(ValueError, match='phonons'):
        el.elastic_constants(ok, z, pos, cell, batch, (3, 3, 3), phonons=other)
    with pytest.raises(RuntimeError, match='MI355X'):
        el.fold_force_constants(other)
    with pytest.raises(ValueError, match='Lambda'):
        el.relaxation_term(torch.zeros(9), torch.zeros(1, dtype=torch.long), [1], torch.zeros(3, 5))


def test_planted_inputs_of_the_stage_test():
    """tests/test_hip_elastic.py plants Phi0 = Q diag(lambda) Q^T: three exact null translations, condition number 100, Lambda with
    zero column sums; the copies of the force constants sum back to Phi0"""
    for n in (1, 2, 11, 32):
        phi0, lam = er.planted_phi0(n, seed=n)
        d = 3 * n
        w = np.linalg.eigvalsh(phi0)
        aw = np.sort(np.abs(w))
        assert np.abs(phi0 - phi0.T).max() == 0 and aw[:3].max() <= 1e-12 * max(aw[-1], 1.0)
        if d > 3:
            assert abs(aw[-1] / aw[3] - (100.0 if d > 4 else 1.0)) <= 1e-8 * 100.0
        for a in range(3):
            t = np.zeros(d)
            t[a::3] = 1.0
            assert np.abs(phi0 @ t).max() <= 1e-12 * max(aw[-1], 1.0)
        assert np.abs(lam.reshape(n, 3, 6).sum(axis=0)).max() <= 1e-12
        fc = er.spread_over_copies(phi0, n, 4, seed=n)
        assert fc.shape == (n, 3, 4 * n, 3)
        assert np.abs(fc.reshape(n, 3, 4, n, 3).sum(axis=2).reshape(d, d) - phi0).max() <= 1e-12
    phi0, lam = er.planted_phi0(2, seed=7, negative=True)
    R, nz, nn = er.relaxation_reference(phi0, lam, 1e-6)
    assert (nz, nn) == (3, 1)
    phi0, lam = er.planted_phi0(2, seed=7, n_null=4)
    assert er.relaxation_reference(phi0, lam, 1e-6)[1] == 4
    # the reference formula is the pseudo-inverse
    phi0, lam = er.planted_phi0(3, seed=1)
    R, nz, nn = er.relaxation_reference(phi0, lam, 1e-6)
    assert np.abs(R - lam.T @ np.linalg.pinv(phi0, rcond=1e-9, hermitian=True) @ lam).max() <= 1e-10 * np.abs(R).max() and nn == 0


def test_planted_eigenpairs_and_their_reference():
    """tests/test_hip_crystal_stages.py hands nnhip_elastic_relax eigenpairs it planted: the reference that takes them as given
    agrees with the one that diagonalises Q^T diag(lambda) Q (to the fp32 rounding of Q), counts what the kernel counts, and its
    bound is dominated by the rounding of R"""
    for d, kw in ((3, dict(n_zero=3)), (63, {}), (66, dict(negative=True)), (96, {})):
        ev, Q, lam = er.planted_eigenpairs(d, seed=d, **kw)
        assert ev.dtype == Q.dtype == lam.dtype == np.float32 and Q.shape == (d, d) and lam.shape == (d, 6)
        assert np.all(np.diff(ev) >= 0) and np.abs(Q.astype(np.float64) @ Q.astype(np.float64).T - np.eye(d)).max() <= 4 * d * er.EPS32
        R, nz, nn, bound = er.relaxation_from_eigenpairs(ev, Q, lam, 1e-3)
        assert nz == 3 and nn == (1 if kw.get('negative') else 0) and np.array_equal(R, R.T)
        assert np.all(bound >= er.EPS32 * np.abs(R)) and np.all(bound <= er.EPS32 * np.abs(R) + 1e-11 * max(np.abs(R).max(), 1e-300))
        if d > 3:
            phi0 = (Q.astype(np.float64).T * ev.astype(np.float64)[None, :]) @ Q.astype(np.float64)
            R2, nz2, nn2 = er.relaxation_reference(0.5 * (phi0 + phi0.T), lam, 1e-3)
            assert (nz2, nn2) == (nz, nn) and np.abs(R - R2).max() <= 100.0 * 8 * d * er.EPS32 * np.abs(R).max()
        else:
            assert np.count_nonzero(R) == 0
    ev, Q, lam = er.planted_eigenpairs(63, seed=63)
    base = er.relaxation_from_eigenpairs(ev, Q, lam, 1e-3)
    # a mode exactly at the threshold, and a NaN eigenvalue, are left out and counted as zero
    at = er.relaxation_from_eigenpairs(ev, Q, lam, float(ev[10]))
    assert at[1] == 11 and at[2] == 0
    bad = ev.copy()
    bad[20] = np.nan
    nan = er.relaxation_from_eigenpairs(bad, Q, lam, 1e-3)
    p = Q[20].astype(np.float64) @ lam.astype(np.float64)
    assert nan[1] == 4 and np.isfinite(nan[0]).all() and np.allclose(base[0] - nan[0], np.outer(p, p) / float(ev[20]), rtol=0, atol=1e-12)
    assert er.relaxation_from_eigenpairs(np.zeros(0), np.zeros((0, 0)), np.zeros((0, 6)), 0.0)[:3:1][1:] == (0, 0)
