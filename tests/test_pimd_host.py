"""CPU-side checks of path-integral molecular dynamics (newtonnet_amd/pimd.py, csrc/pimd.hip): the normal-mode transform is
orthonormal and diagonalises the ring's spring matrix, the free-ring-polymer step of the restatement the GPU tests compare against
(tests/pimd_ref.py) is the exact propagator built independently in bead space, the whole thermostatted step has the stationary
covariance of the quantum harmonic oscillator up to its second-order splitting error (and the three estimators agree on it),
arguments are refused before any device work, and the C ABI carries the new entry point."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import pimd_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the transform -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('P', [1, 2, 3, 4, 5, 8, 16, 33, 64])
def test_transform_is_orthonormal_and_diagonalises_the_spring_matrix(P):
    from newtonnet_amd import pimd
    C = pimd.transform_matrix(P)
    assert C.dtype == np.float64 and C.shape == (P, P)
    assert np.abs(C @ C.T - np.eye(P)).max() <= 1e-14
    S = np.roll(np.eye(P), 1, axis=1)                                      # the cyclic shift
    K = 2.0 * np.eye(P) - S - S.T
    T = 300.0
    om = pimd.mode_frequencies(P, [T])[0]
    omega_P = P * pimd.K_BOLTZMANN * T / pimd.HBAR
    assert np.abs(C @ K @ C.T - np.diag((om / omega_P) ** 2)).max() <= 1e-13
    assert abs(pimd.HBAR - 0.0646541513) < 1e-10


# ---- 2. the free ring polymer -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('P', [3, 8])
def test_free_step_of_the_restatement_is_the_exact_propagator_in_bead_space(P):
    from newtonnet_amd import pimd
    rng = np.random.default_rng(P)
    T, dt_fs = 300.0, 0.25
    h = 0.5 * dt_fs * pimd.FS
    omega_P = P * pimd.K_BOLTZMANN * T / pimd.HBAR
    x, v = rng.normal(0, 1.0, P), rng.normal(0, 1.0, P)
    # independently: exp(h [[0, I], [-omega_P^2 K, 0]]) from the eigenvectors of K
    S = np.roll(np.eye(P), 1, axis=1)
    lam, V = np.linalg.eigh(2.0 * np.eye(P) - S - S.T)
    om = omega_P * np.sqrt(np.clip(lam, 0.0, None))
    q, p = V.T @ x, V.T @ v
    soft = om < 1e-6 * omega_P
    sinc = np.where(soft, h, np.sin(om * h) / np.where(soft, 1.0, om))
    x_ref = V @ (np.cos(om * h) * q + sinc * p)
    v_ref = V @ (-om * np.sin(om * h) * q + np.cos(om * h) * p)
    # the restatement: to modes, A with the fp64 table, back
    C = pimd.transform_matrix(P)
    tab = pimd.mode_tables(P, [T], dt_fs, 0.0, 0.0, dtype=np.float64)[0][0]
    u, w = (C @ x)[:, None, None], (C @ v)[:, None, None]
    un, wn, _, _ = pr.free_half_step(u, w, 0.0, 0.0, tab[:, 0, None, None], tab[:, 1, None, None], tab[:, 2, None, None])
    x_new, v_new = C.T @ un[:, 0, 0], C.T @ wn[:, 0, 0]
    assert np.abs(x_new - x_ref).max() <= 1e-12 * np.abs(x_ref).max()
    assert np.abs(v_new - v_ref).max() <= 1e-12 * np.abs(v_ref).max()


# ---- 3. the stationary distribution of the whole step -----------------------------------------------------------------------------

M_H, WAVENUMBER, T_OSC = 1.008, 3000.0, 300.0


def _stationary(P, dt_fs, centroid_friction=0.01, mode_friction=1.0):
    """(Sigma [2P, 2P] of (u, w), omega, omega_k) of the restatement's own step on the 1-D oscillator"""
    from newtonnet_amd import pimd
    omega = 2.0 * math.pi * 2.99792458e10 * WAVENUMBER * 1e-15 / pimd.FS         # rad per internal time unit
    C = pimd.transform_matrix(P)
    tab, one_minus = pimd.mode_tables(P, [T_OSC], dt_fs, centroid_friction, mode_friction, dtype=np.float64)
    tab, one_minus = tab[0], one_minus[0]
    hk = np.full((P, 1), 0.5 * dt_fs * pimd.FS / M_H)
    sigma = np.sqrt(one_minus * pimd.K_BOLTZMANN * P * T_OSC / M_H)[:, None]

    def force(u):
        return -M_H * omega ** 2 * np.einsum('ks,kic->sic', C, u)

    def step(z, xi):
        u, w = np.zeros((P, 1, 3)), np.zeros((P, 1, 3))
        u[:, 0, 0], w[:, 0, 0] = z[:P], z[P:]
        noise = np.zeros((P, 1, 3))
        noise[:, 0, 0] = xi
        a = pr.pimd_step(pr.BEGIN, u, w, force(u), C, tab, hk, None, sigma, noise)
        b = pr.pimd_step(pr.FINISH, a['u'], a['w'], force(a['u']), C, tab, hk)
        return np.concatenate([a['u'][:, 0, 0], b['w'][:, 0, 0]])
    eye = np.eye(2 * P)
    M = np.stack([step(eye[j], np.zeros(P)) for j in range(2 * P)], axis=1)
    Nn = np.stack([step(np.zeros(2 * P), np.eye(P)[j]) for j in range(P)], axis=1)
    S, A = Nn @ Nn.T, M
    for _ in range(200):                              # Sigma = sum_j M^j Q M^jT by doubling, until M^(2^j) has died out
        S = S + A @ S @ A.T
        A = A @ A
        if np.abs(A).max() < 1e-30:
            break
    else:
        raise AssertionError('the step does not contract')
    return S, omega, pimd.mode_frequencies(P, [T_OSC])[0]


def _deviations(P, dt_fs):
    from newtonnet_amd import pimd
    S, omega, om = _stationary(P, dt_fs)
    kT = pimd.K_BOLTZMANN * T_OSC
    uu, ww = np.diag(S)[:P], np.diag(S)[P:]
    dev_u = np.abs(uu / (kT * P / (M_H * (omega ** 2 + om ** 2))) - 1.0).max()
    dev_w = np.abs(ww / (kT * P / M_H) - 1.0).max()
    exact = 0.5 * kT * (omega ** 2 / (omega ** 2 + om ** 2)).sum()
    potential = 0.5 * M_H * omega ** 2 * uu.sum() / P
    # u_k f_k with f_k = -m omega^2 u_k (the transform is orthogonal)
    virial = 0.5 * kT + 0.5 * M_H * omega ** 2 * uu[1:].sum() / P
    primitive = 0.5 * P * kT - (0.5 * M_H * om ** 2 * uu).sum() / P
    return dev_u, dev_w, [abs(e / exact - 1.0) for e in (potential, virial, primitive)]


def test_stationary_covariance_is_the_quantum_oscillators_up_to_the_splitting_error():
    dev1, _, est1 = _deviations(1, 0.25)
    print(f'P = 1: deviation of <u^2> {dev1:.2e}')
    assert dev1 <= 1e-9                                # BAOAB is configurationally exact for a harmonic well
    assert est1[0] <= 1e-9 and est1[1] <= 1e-9 and est1[2] <= 1e-9
    for P in (4, 8, 32):
        d25, w25, est = _deviations(P, 0.25)
        d50, _, _ = _deviations(P, 0.5)
        print(f'P = {P}: deviation of <u_k^2> at 0.25 fs {d25:.2e}, at 0.5 fs {d50:.2e} (ratio {d50 / d25:.2f}); of <w_k^2> {w25:.2e}; '
              f'estimators potential {est[0]:.2e}, centroid virial {est[1]:.2e}, primitive {est[2]:.2e}')
        assert 3.5 <= d50 / d25 <= 4.5                 # second order
        assert d25 <= 2.5e-3
        assert est[0] <= d25 and est[1] <= d25          # within the deviation of <u_k^2> at the same P
        assert est[2] <= d25 + w25                      # ... plus that of <w_k^2>


# ---- 4. arguments -----------------------------------------------------------------------------------------------------------------

class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force']

    def path_integral(self, *a, **kw):
        from newtonnet_amd.models import NewtonNet
        return NewtonNet.path_integral(self, *a, **kw)


def _inputs(n=3, g=2):
    return (torch.ones(n * g, dtype=torch.long), torch.zeros(n * g, 3), torch.zeros(g, 3, 3), torch.arange(g).repeat_interleave(n))


def test_path_integral_validates_before_any_device_work():
    from newtonnet_amd.dynamics import Dynamics
    from newtonnet_amd.pimd import PathIntegral
    z, pos, cell, batch = _inputs()
    ok = _FakeModel()
    for bad in (0, 65, 2.5, True, None, -1):
        with pytest.raises(ValueError, match='n_beads'):
            ok.path_integral(z, pos, cell, batch, bad, 300.0)
    for bad in (None, 0, 0.0, -5.0, float('nan'), [300.0], [300.0, 300.0, 300.0], torch.full((3,), 300.0), [300.0, -1.0]):
        with pytest.raises(ValueError, match='temperature'):
            ok.path_integral(z, pos, cell, batch, 4, bad)
    with pytest.raises(ValueError, match='centroid_friction'):
        ok.path_integral(z, pos, cell, batch, 4, 300.0, centroid_friction=-0.01)
    with pytest.raises(ValueError, match='mode_friction'):
        ok.path_integral(z, pos, cell, batch, 4, 300.0, mode_friction=-1.0)
    train = _FakeModel()
    train.training = True
    with pytest.raises(ValueError, match='eval'):
        train.path_integral(z, pos, cell, batch, 4, 300.0)
    energy_only = _FakeModel()
    energy_only.output_properties = ['energy']
    with pytest.raises(ValueError, match='gradient_force'):
        energy_only.path_integral(z, pos, cell, batch, 4, 300.0)
    for name in ('bead_positions', 'bead_velocities'):
        for bad in (torch.zeros(6, 3), torch.zeros(24, 2), torch.zeros(23, 3), np.zeros((24, 3))):
            with pytest.raises(ValueError, match=name):
                ok.path_integral(z, pos, cell, batch, 4, 300.0, **{name: bad})
    with pytest.raises(ValueError, match='timestep'):
        ok.path_integral(z, pos, cell, batch, 4, 300.0, timestep=0.0)
    with pytest.raises(TypeError):
        ok.path_integral(z, pos, cell, batch, 4, 300.0, fixed=torch.zeros(6, dtype=torch.bool))     # not offered
    for good in (300.0, [300.0, 250.0], torch.tensor([300.0, 250.0]), np.array([300.0, 250.0])):
        with pytest.raises(RuntimeError, match='MI355X'):                                          # CPU tensors: no CPU path
            ok.path_integral(z, pos, cell, batch, 4, good, bead_positions=torch.zeros(24, 3))
    assert PathIntegral._recorded_steps is Dynamics._recorded_steps and PathIntegral._evaluate is Dynamics._evaluate


def test_calculator_run_pimd_validates_before_any_device_work():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype = torch.device('cpu'), torch.float32
    calc.model = _FakeModel()
    a, b = FakeAtoms([8, 1, 1], np.zeros((3, 3))), FakeAtoms([6, 1], np.zeros((2, 3)))
    with pytest.raises(ValueError, match='at least one'):
        calc.run_pimd([], 4, 300.0, 10)
    with pytest.raises(ValueError, match='sizes'):
        calc.run_pimd([a, b], 4, 300.0, 10)
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match='n_beads'):
            calc.run_pimd(a, bad, 300.0, 10)
    for bad in (None, 0.0, -1.0, [300.0, 300.0]):
        with pytest.raises(ValueError, match='temperature'):
            calc.run_pimd(a, 4, bad, 10)
    with pytest.raises(ValueError, match='friction'):
        calc.run_pimd(a, 4, 300.0, 10, centroid_friction=-1.0)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match='n_steps'):
            calc.run_pimd(a, 4, 300.0, bad)
        with pytest.raises(ValueError, match='record_every'):
            calc.run_pimd(a, 4, 300.0, 10, record_every=bad)
    with pytest.raises(ValueError, match='timestep'):
        calc.run_pimd(a, 4, 300.0, 10, timestep=0.0)
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.run_pimd([a, a], 4, [300.0, 250.0], 10)


# ---- 5. the ABI -------------------------------------------------------------------------------------------------------------------

def test_kernel_symbol_is_declared_listed_and_exported_and_the_constants_agree():
    from newtonnet_amd import abi, hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert 'nnhip_pimd_step' in abi.FUNCTIONS and 'nnhip_pimd_step' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'nnhip_pimd_step')
    restype, argtypes = abi.FUNCTIONS['nnhip_pimd_step']
    assert restype is ctypes.c_int32 and len(argtypes) == 19 and argtypes[12:16] == [ctypes.c_int32] * 4
    for name, value in (('NNHIP_PIMD_FINISH', 1), ('NNHIP_PIMD_BEGIN', 2), ('NNHIP_PIMD_MAX_BEADS', 64), ('NNHIP_PIMD_THREADS', 256)):
        assert abi.CONSTANTS[name] == value
    assert (hip.PIMD_FINISH, hip.PIMD_BEGIN, hip.PIMD_MAX_BEADS) == (pr.FINISH, pr.BEGIN, 64)
    assert [hip.pimd_tile_atoms(P) for P in (1, 3, 8, 33, 64)] == [256, 85, 32, 7, 4]
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bpimd\b.*\)', f.read(), re.M)
