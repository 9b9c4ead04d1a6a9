"""Host-side checks of the mode Grueneisen parameters: the fp64 yardstick (tests/gruneisen_ref.py) against an analytic lattice and a
designed crossing, the strained-crystal construction, the condition on the inputs of the device tests, the formulas of the mean
Grueneisen parameter and the thermal expansion, the argument checks and the ABI symbol (no device)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from newtonnet_amd import gruneisen as gn
from newtonnet_amd import phonons as ph
from tests import gruneisen_ref as gr
from tests import phonon_ref as pr
from tests import phonon_velocity_ref as pv
from tests.test_phonon_host import _FakeModel, _crystal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = pr.EPS32


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def analytic_problem(n_fold, q):
    """the coupled cubic lattice and the plane of ANALYTIC_DK, both as the device holds them (fp32)"""
    fc, pos, cell, S, m = pv.coupled_cubic_lattice(n_fold=n_fold)
    plane = pv.coupled_cubic_lattice(gr.ANALYTIC_DK, n_fold=n_fold)[0]
    return gr.problem(f32(fc), f32(plane)[None], pos, cell, S, f32(m), q)


# ---- the analytic lattice ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_fold', pv.ANALYTIC_FOLDS)
def test_yardstick_against_the_analytic_lattice(n_fold):
    """The lattice is linear in its spring constants: the plane built from dK has the slopes of the formula evaluated at dK.  dK holds
    binary fractions, so its fp32 rounding is exact.  At CROSSING_Q every mode of a folded cell sits in a pair (k, n_fold - 1 - k); the
    two have the same cosines, so NO dK of this form splits them: both take the same slope and the order inside the pair is the tie
    rule's (the designed crossing below is split by its plane)."""
    assert np.array_equal(f32(gr.ANALYTIC_DK), gr.ANALYTIC_DK)
    assert np.linalg.matrix_rank(np.stack([gr.ANALYTIC_DK.ravel(), pv.COUPLED_K.ravel()])) == 2          # not proportional to K
    for q in list(pv.ANALYTIC_Q) + [pv.CROSSING_Q]:
        p = analytic_problem(n_fold, q)
        lam, dlam = gr.coupled_cubic_slopes(q, n_fold=n_fold)
        assert np.abs(lam - pv.coupled_cubic_analytic(q, n_fold=n_fold)[0]).max() <= 1e-13 * np.abs(lam).max()
        assert not p['capped'].any()
        err = np.abs(p['dlam'][:, 0] - dlam).max()
        print(f'n_fold {n_fold} q {q}: |dlam - formula| = {err:.2e}, max |dlam| = {np.abs(dlam).max():.3f}')
        assert err <= 2 * EPS32 * np.abs(dlam).max()
        if q is pv.CROSSING_Q and n_fold > 1:
            assert p['first'].tolist() == [2 * (k // 2) for k in range(3 * n_fold)]
            assert np.abs(dlam[0::2] - dlam[1::2]).max() <= 1e-12 * np.abs(dlam).max()
        elif q is not pv.CROSSING_Q:
            assert len(set(p['first'])) == 3 * n_fold
        assert np.abs(p['gamma'][:, 0] + dlam / (2.0 * lam)).max() <= 1e-6 * np.abs(dlam / lam).max()


def test_a_crossing_pair_is_split_by_the_plane_in_the_order_of_its_slopes():
    """the d = 99 crystal of phonon_velocity_ref: modes 63 and 64 live on different atoms and cross; the plane scales every atom's force
    constants by its own factor c_i, so the two slopes are c_i lambda and c_j lambda, the smaller first"""
    fc, pos, cell, S, m = pv.planted_levels_crystal(pv.straddle_levels('pair'))
    plane, c = gr.atom_scaled_plane(f32(fc))
    p = gr.problem(f32(fc), f32(plane)[None], pos, cell, S, f32(m), pv.STRADDLE_Q)
    want = np.arange(99)
    want[64] = 63
    assert np.array_equal(p['first'], want) and not p['capped'].any()
    lam = p['lam'][63]
    owners = [int(np.argmax(np.abs(p['modes'][k]).reshape(33, 3).sum(axis=1))) for k in (63, 64)]
    assert owners[0] != owners[1]
    slopes = np.sort([c[owners[0]] * lam, c[owners[1]] * lam])
    assert np.abs(p['dlam'][63:65, 0] - slopes).max() <= 1e-5 * slopes.max()          # (fp32 rounding of the plane)
    split = p['dlam'][64, 0] - p['dlam'][63, 0]
    bound = gr.error_bound(gr.BOUND_C, p)[63:65].max()
    print(f'd = 99: split {split:.3f}, bound {bound:.3e}, bound / max |dlam| = {gr.error_bound(gr.BOUND_C, p).max() / np.abs(p["dlam"]).max():.2e}')
    assert split > 4 * bound
    cap = gr.problem(f32(pv.planted_levels_crystal(pv.straddle_levels('cap'))[0]), f32(plane)[None], pos, cell, S, f32(m), pv.STRADDLE_Q)
    assert cap['capped'].sum() == 18 and cap['capped'][55:73].all() and np.all(cap['dlam'][55:73] == 0.0)
    assert not cap['defined'][55:73].any() and np.all(cap['gamma'][55:73] == 0.0)


def test_the_rayleigh_identity_of_the_yardstick():
    """dfc = a fc: dlam = a lambda, gamma = -a / 2 for every mode, degenerate or not"""
    _, fc = pr.random_crystal(2, pr.TRICLINIC_S, 5)
    args = (pr.TRICLINIC_POS, pr.TRICLINIC_CELL, pr.TRICLINIC_S, pr.TRICLINIC_MASSES)
    for q in ([0.31, -0.17, 0.44], [0.0, 0.0, 0.0]):
        p = gr.problem(fc, 0.7 * fc[None], *args, np.array(q))
        assert p['defined'].all() and (p['lam'] < 0).any()
        assert np.abs(p['dlam'][:, 0] - 0.7 * p['lam']).max() <= 1e-12 * np.abs(p['lam']).max()
        assert np.abs(p['gamma'] + 0.35).max() <= 1e-10
    # six planes: each plane's slopes do not depend on the others, whatever the weights, where nothing is degenerate
    planes = np.random.default_rng(3).standard_normal((6,) + fc.shape)
    six = gr.problem(fc, planes, *args, np.array([0.31, -0.17, 0.44]), weights=[1, 2, 3, 4, 5, 6])
    for k in range(6):
        one = gr.problem(fc, planes[k:k + 1], *args, np.array([0.31, -0.17, 0.44]))
        assert np.abs(one['dlam'][:, 0] - six['dlam'][:, k]).max() <= 1e-12 * np.abs(six['dlam']).max()


def test_the_plane_sum_is_the_dynamical_matrix_of_the_plane():
    """gruneisen_ref.d_dynamical forms the weights once for all planes: element for element phonon_ref.dynamical_matrix of each plane,
    and its |terms| are those of that function's bound (the tie crystal: 2, 4 and 8 equally near images)"""
    fc, pos, cell, S, m = pr.tie_crystal()
    planes = np.random.default_rng(2).standard_normal((3,) + fc.shape)
    table = pr.image_table_fast(pos, cell, S)
    for q in pr.STAGE_Q[1:4]:
        dD, A = gr.d_dynamical(planes, pos, cell, S, m, q, table, with_abs=True)
        for k in range(3):
            D, bound = pr.dynamical_matrix(planes[k], pos, cell, S, m, q, table, with_bound=True)
            assert np.abs(dD[k] - D).max() <= 1e-13 * np.abs(D).max()
            terms = bound / ((fc.shape[2] // fc.shape[0] + 8) * EPS32)
            assert np.all(A[k] >= terms * (1 - 1e-12)) and np.all(A[k] <= terms * (1 + 1e-6))


# ---- strained crystals -----------------------------------------------------------------------------------------------------------

E2E_CELLS = np.array([[[4.2, 0.4, -0.3], [0.4, 4.1, 0.5], [-0.3, 0.5, 4.3]],
                      [[4.3, -0.2, 0.3], [-0.2, 4.2, -0.4], [0.3, -0.4, 4.1]]])
E2E_POS = np.array([[0.4, 0.5, 0.3], [1.3, 1.1, 1.0], [0.6, 0.4, 0.5], [1.4, 0.9, 0.8], [0.1, 1.2, 0.2]])
E2E_BATCH = np.array([0, 0, 1, 1, 1])


def test_strained_crystals_volume_and_voigt():
    delta = 0.01
    eps, copies = gn.strained_crystals(E2E_POS, E2E_CELLS, E2E_BATCH, 'volume', delta, dtype=torch.float64)
    assert eps.shape == (1, 3, 3) and len(copies) == 1
    for sign, (p, c, Q) in zip((-1.0, 1.0), copies[0]):
        p, c = p.numpy(), c.numpy()
        for b in range(2):
            assert abs(np.log(np.linalg.det(c[b]) / np.linalg.det(E2E_CELLS[b])) - sign * delta) <= 1e-12
            assert np.array_equal(c[b], c[b].T) and np.array_equal(Q[b], np.eye(3))
            want = gr.strained_crystal(E2E_POS[E2E_BATCH == b], E2E_CELLS[b], 'volume', delta)[0][0 if sign < 0 else 1]
            assert np.abs(p[E2E_BATCH == b] - want[0]).max() <= 1e-12 and np.abs(c[b] - want[1]).max() <= 1e-12
    # the default is what the model takes
    assert gn.strained_crystals(E2E_POS, E2E_CELLS, E2E_BATCH)[1][0][0][0].dtype == torch.float32
    eps, copies = gn.strained_crystals(torch.tensor(E2E_POS), torch.tensor(E2E_CELLS), torch.tensor(E2E_BATCH), 'voigt', delta,
                                       dtype=torch.float64)
    assert eps.shape == (6, 3, 3) and all(np.array_equal(eps[J], gr.voigt_matrix(J)) for J in range(6))
    rng = np.random.default_rng(11)
    for J in range(6):
        for s, (p, c, Q) in enumerate(copies[J]):
            p, c = p.numpy(), c.numpy()
            for b in range(2):
                sel = E2E_BATCH == b
                F = np.eye(3) + (2 * s - 1) * delta * eps[J]
                assert np.abs(c[b] - c[b].T).max() <= 1e-12 and np.abs(Q[b] @ Q[b].T - np.eye(3)).max() <= 1e-14
                assert np.linalg.det(Q[b]) > 0 and np.abs(c[b] @ Q[b] - E2E_CELLS[b] @ F).max() <= 1e-12
                assert np.abs(p[sel] @ Q[b] - E2E_POS[sel] @ F).max() <= 1e-12
                want = gr.strained_crystal(E2E_POS[sel], E2E_CELLS[b], 'voigt', delta)[J][s]
                assert np.abs(p[sel] - want[0]).max() <= 1e-12 and np.abs(c[b] - want[1]).max() <= 1e-12
                assert np.abs(Q[b] - want[2]).max() <= 1e-12
        # rotating back a synthetic rotated Phi recovers Phi to fp64 rounding
        Q = copies[J][1][2]
        counts, sc = [2, 3], [4, 6]
        phi = [rng.standard_normal((n, 3, N, 3)) for n, N in zip(counts, sc)]
        rot = torch.tensor(np.concatenate([gr.rotate_forward(phi[b], Q[b]).ravel() for b in range(2)]))
        back = gn.rotate_back(rot, Q, counts, sc).numpy()
        assert np.abs(back - np.concatenate([x.ravel() for x in phi])).max() <= 1e-14
    # explicit matrices are treated like 'voigt'
    one = gn.strained_crystals(E2E_POS, E2E_CELLS, E2E_BATCH, eps[3:5], delta, dtype=torch.float64)[1]
    assert len(one) == 2 and torch.equal(one[0][1][1], copies[3][1][1]) and torch.equal(one[1][0][0], copies[4][0][0])


# ---- the bound -----------------------------------------------------------------------------------------------------------------

def test_the_bound_of_the_device_tests_is_tight_on_their_inputs():
    """For every mode the analytic device test compares, error_bound(BOUND_C) is at most 1 % of the problem's largest |dlam|: the
    condition tests/test_phonon_velocity_host.py holds, so that the bound cannot hide a failure."""
    for n_fold in pv.ANALYTIC_FOLDS:
        for q in list(pv.ANALYTIC_Q) + [pv.CROSSING_Q]:
            p = analytic_problem(n_fold, q)
            keep = p['defined']
            ratio = (gr.error_bound(gr.BOUND_C, p)[keep] / np.abs(p['dlam']).max()).max()
            print(f'n_fold {n_fold} q {q}: bound / max |dlam| = {ratio:.2e}')
            assert ratio <= 0.01


# ---- formulas ---------------------------------------------------------------------------------------------------------------------

def _cv(lam, T):
    x = pr.EV_PER_SQRT_EIGENVALUE * np.sqrt(lam) / (pr.K_BOLTZMANN * T)
    return pr.K_BOLTZMANN * x * x * np.exp(-x) / (1.0 - np.exp(-x)) ** 2


def _mesh(evals, gam, defined, form):
    """a GruneisenMesh over one cubic one-atom crystal from values given by hand (CPU tensors)"""
    fc, pos, cell = pr.cubic_lattice()
    p = ph.Phonons.from_force_constants(fc, [1], pos, cell, pr.CUBIC_S, masses=[pr.CUBIC_MASS], device='cpu')
    ev = torch.tensor(np.asarray(evals, dtype=np.float32).reshape(-1))
    bands = gn.GruneisenBands(eigenvalues=ev, frequencies=ev, modes=None, dynamical_matrix=None, sweeps=None, status=None,
                              q=np.zeros((np.asarray(evals).shape[0], 3)), _dims=p._dims, _offsets=p._offsets, _sq_offsets=p._sq_offsets,
                              gruneisen=torch.tensor(np.asarray(gam, dtype=np.float32).reshape(ev.numel(), -1)),
                              eigenvalue_strain_gradients=None, gruneisen_defined=torch.tensor(np.asarray(defined).reshape(-1)),
                              degenerate_group=None)
    return gn.GruneisenMesh(bands, p, form), abs(np.linalg.det(cell))


def test_mean_and_thermal_expansion_against_hand_sums():
    T = 300.0
    ev = np.array([[0.0, 1.0, 4.0]])
    c1, c2 = _cv(1.0, T), _cv(4.0, T)
    C = np.diag([2.0, 2.0, 2.0, 0.5, 0.5, 0.5]) + 0.25 * (np.ones((6, 6)) - np.eye(6)) * (np.arange(6)[:, None] < 3) * (np.arange(6)[None, :] < 3)
    # volume form: one plane
    gam = np.array([[[9.0], [1.5], [0.5]]])
    ok = np.array([[False, True, True]])
    want = (c1 * 1.5 + c2 * 0.5) / (c1 + c2)
    assert abs(gr.mean(ev, gam, ok, T, 1e-6)[0] - want) <= 1e-14
    mesh, vol = _mesh(ev, gam, ok, 'volume')
    assert abs(float(mesh.mean(T)[0, 0]) - want) <= 2e-7 * want
    B = (3 * 2.0 + 6 * 0.25) / 9.0
    alpha = (c1 * 1.5 + c2 * 0.5) / (vol * B)
    assert abs(gr.thermal_expansion(ev, gam, ok, T, 1e-6, vol, C, 'volume') - alpha) <= 1e-14 * alpha
    got = mesh.thermal_expansion(T, elastic=torch.tensor(C)[None])
    assert tuple(got.shape) == (1,) and got.dtype == torch.float32 and abs(float(got[0]) - alpha) <= 2e-7 * alpha
    # a mode that is live but not defined is left out of both sums
    assert abs(gr.mean(ev, gam, np.array([[False, True, False]]), T, 1e-6)[0] - 1.5) <= 1e-14
    # Voigt form: six planes
    g6 = np.zeros((1, 3, 6))
    g6[0, 1], g6[0, 2] = [1.0, 2.0, 3.0, 0.1, 0.2, 0.3], [0.5, 0.4, 0.3, -0.1, 0.0, 0.2]
    s = c1 * g6[0, 1] + c2 * g6[0, 2]
    a6 = np.linalg.inv(C) @ s / vol
    assert np.abs(gr.thermal_expansion(ev, g6, ok, T, 1e-6, vol, C, 'voigt') - a6).max() <= 1e-14 * np.abs(a6).max()
    mesh6, _ = _mesh(ev, g6, ok, 'voigt')
    got = mesh6.thermal_expansion(T, elastic=torch.tensor(C)[None])
    assert tuple(got.shape) == (1, 6) and np.abs(got[0].numpy() - a6).max() <= 2e-7 * np.abs(a6).max()
    assert tuple(mesh6.mean(T).shape) == (1, 6) and float(mesh6.thermal_expansion(0.0, elastic=torch.tensor(C)[None]).abs().max()) == 0.0


def test_a_plane_proportional_to_the_force_constants():
    """dfc = a fc: gamma = -a / 2 for every mode, mean(T) = -a / 2 at any T, alpha_V = -a C_v / (2 V B)"""
    a, B = 0.6, 1.3
    fc, pos, cell = pr.cubic_lattice()
    q = pr.monkhorst_pack(2, 3, 2, shift=True)
    ps = [gr.problem(fc, a * fc[None], pos, cell, pr.CUBIC_S, [pr.CUBIC_MASS], x) for x in q]
    ev, gam, ok = (np.stack([p[k] for p in ps]) for k in ('lam', 'gamma', 'defined'))
    assert ok.all() and np.abs(gam + a / 2).max() <= 1e-12
    vol = abs(np.linalg.det(cell))
    C = np.diag([B] * 3 + [1.0] * 3) + B * (np.ones((6, 6)) - np.eye(6)) * (np.arange(6)[:, None] < 3) * (np.arange(6)[None, :] < 3)
    assert abs(gr.bulk_modulus_voigt(C) - B) <= 1e-15
    for T in (30.0, 300.0, 3000.0):
        assert abs(gr.mean(ev, gam, ok, T, 0.0)[0] + a / 2) <= 1e-12
        cv = sum(_cv(x, T) for x in ev.ravel()) / len(q)
        want = -a * cv / (2.0 * vol * B)
        assert abs(gr.thermal_expansion(ev, gam, ok, T, 0.0, vol, C, 'volume') - want) <= 1e-12 * abs(want)
        mesh, _ = _mesh(ev, gam, ok, 'volume')
        assert abs(float(mesh.mean(T)[0, 0]) + a / 2) <= 1e-6
        assert abs(float(mesh.thermal_expansion(T, elastic=torch.tensor(C)[None])[0]) - want) <= 1e-5 * abs(want)


# ---- arguments -------------------------------------------------------------------------------------------------------------------

def test_argument_errors_come_before_any_device_work():
    from newtonnet_amd.models.newtonnet import NewtonNet
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    assert callable(NewtonNet.gruneisen) and callable(MLAseCalculator.gruneisen)
    z, pos, cell, batch = _crystal()
    ok = _FakeModel()
    for bad in (0.0, -0.01, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='delta'):
            gn.gruneisen(ok, z, pos, cell, batch, (3, 3, 3), delta=bad)
        with pytest.raises(ValueError, match='delta'):
            gn.strained_crystals(pos, cell, batch, 'volume', bad)
    skew = np.eye(3)[None].copy()
    skew[0, 0, 1] = 0.1
    with pytest.raises(ValueError, match='strain.*not symmetric'):
        gn.gruneisen(ok, z, pos, cell, batch, (3, 3, 3), strain=skew)
    with pytest.raises(ValueError, match='strain: at most 6'):
        gn.gruneisen(ok, z, pos, cell, batch, (3, 3, 3), strain=np.tile(np.eye(3), (7, 1, 1)))
    for bad in ('shear', np.zeros((2, 3)), np.zeros((0, 3, 3))):
        with pytest.raises(ValueError, match='strain'):
            gn.gruneisen(ok, z, pos, cell, batch, (3, 3, 3), strain=bad)
    with pytest.raises(ValueError, match='split_weights'):
        gn.gruneisen(ok, z, pos, cell, batch, (3, 3, 3), strain='voigt', split_weights=[0.0] * 6)
    # the checks of phonons.phonons, in its words, at the central cell and at the strained ones
    train = _FakeModel()
    train.training = True
    with pytest.raises(NotImplementedError, match='eval'):
        gn.gruneisen(train, z, pos, cell, batch, (3, 3, 3))
    with pytest.raises(ValueError, match='2 x cutoff'):
        gn.gruneisen(ok, z, pos, cell, batch, (2, 3, 3))
    narrow = cell * (10.0 / 12.6) * 1.0001          # wide enough as it stands, too narrow once compressed
    with pytest.raises(ValueError, match='2 x cutoff'):
        gn.gruneisen(ok, z, pos, narrow, batch, (3, 3, 3), delta=0.01)
    with pytest.raises(RuntimeError, match='MI355X'):          # ... and a good set of arguments gets as far as the device check
        gn.gruneisen(ok, z, pos, cell, batch, (3, 3, 3), strain='voigt', delta=0.02)
    # queries
    fc, p1, c1 = pr.cubic_lattice()
    p = ph.Phonons.from_force_constants(fc, [1], p1, c1, pr.CUBIC_S, masses=[pr.CUBIC_MASS], device='cpu')
    g = gn.Gruneisen.from_phonons(p, p, p, 0.01)
    assert tuple(g.dfc.shape) == (1, p.fc.numel()) and g.dfc_split.data_ptr() == g.dfc.data_ptr() and g.form == 'volume'
    assert float(g.dfc.abs().max()) == 0.0 and np.array_equal(g.split_weights, [1.0])
    with pytest.raises(ValueError, match='degeneracy_tol'):
        g.frequencies([[0.1, 0.2, 0.3]], degeneracy_tol=-1.0)
    with pytest.raises(ValueError, match='finite'):
        g.frequencies([[0.1, float('nan'), 0.3]])
    with pytest.raises(RuntimeError, match='MI355X'):
        g.frequencies([[0.1, 0.2, 0.3]])
    with pytest.raises(ValueError, match='step|delta'):
        gn.Gruneisen.from_phonons(p, p, p, 0.0)
    fc2, p2, c2 = pr.cubic_lattice(S=(2, 2, 2))
    other = ph.Phonons.from_force_constants(fc2, [1], p2, c2, (2, 2, 2), masses=[pr.CUBIC_MASS], device='cpu')
    with pytest.raises(ValueError, match='ph_plus'):
        gn.Gruneisen.from_phonons(p, p, other, 0.01)
    # a mesh made without the option, a missing tensor, T = 0
    plain = ph.PhononBands(eigenvalues=torch.ones(3), q=np.zeros((1, 3)), _dims=p._dims, _offsets=p._offsets)
    with pytest.raises(ValueError, match='gruneisen'):
        gn.GruneisenMesh(plain, p, 'volume').mean(300.0)
    mesh, _ = _mesh([[0.0, 1.0, 4.0]], [[[9.0], [1.5], [0.5]]], [[False, True, True]], 'volume')
    with pytest.raises(ValueError, match='elastic'):
        mesh.thermal_expansion(300.0)
    with pytest.raises(ValueError, match='elastic'):
        mesh.thermal_expansion(300.0, elastic=torch.eye(6))
    with pytest.raises(ValueError, match='temperature'):
        mesh.mean(0.0)
    mesh.form = 'custom'
    with pytest.raises(ValueError, match='strain'):
        mesh.thermal_expansion(300.0, elastic=torch.eye(6)[None])
    with pytest.raises(ValueError, match='gruneisen'):
        gn.GruneisenBands(q=np.zeros((1, 3))).gruneisen_parameters(0)


def test_kernel_symbol_is_declared_listed_and_exported():
    from newtonnet_amd import abi, hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    name = 'nnhip_phonon_strain_slopes'
    assert name in declared and name in abi.FUNCTIONS and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bphonon_gruneisen\b.*\)', f.read(), re.M)
    assert gn.MAX_PLANES == 6
