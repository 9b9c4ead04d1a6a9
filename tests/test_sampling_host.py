"""CPU-side checks of normal-mode sampling and harmonic thermochemistry (newtonnet_amd/vibrations.py, csrc/sample.hip): the fp64
reference formulas the GPU tests compare against (tests/sample_ref.py) have the limits and identities they must have, the
synthetic inputs are what their docstrings claim, the C ABI exports the kernel, and the arguments are validated before any
device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import sample_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = np.array([2.7e-3, 0.05, 0.5, 3.0, 30.0])          # 27 .. 2856 cm^-1


def test_kernel_symbol_is_declared_listed_and_exported():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    assert 'nnhip_mode_sample' in declared and 'nnhip_mode_sample' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'nnhip_mode_sample')
    assert lib.nnhip_version() >= 111


def test_constants():
    from newtonnet_amd import vibrations as vib
    assert vib.K_BOLTZMANN == 8.617333262e-5 == sr.K_BOLTZMANN
    assert abs(vib.K_BOLTZMANN - 1.380649e-23 / 1.602176634e-19) <= 1e-9 * vib.K_BOLTZMANN
    # hbar omega of lambda = 1 eV / (A^2 amu): hbar = 6.582119569e-16 eV s, omega = 9.822694e13 rad / s
    assert abs(sr.HBAR_UNIT - 6.582119569e-16 * 9.8226948e13) <= 1e-6 * sr.HBAR_UNIT
    assert abs(vib.EV_PER_SQRT_EIGENVALUE - sr.HBAR_UNIT) <= 1e-12 * sr.HBAR_UNIT
    # 2 x the zero-point energy per mode the package already reports (0.5 EV_PER_WAVENUMBER nu~)
    assert abs(sr.mode_energy(4.0) - 2 * 0.5 * vib.EV_PER_WAVENUMBER * vib.WAVENUMBER_PER_SQRT_EIGENVALUE * 2.0) <= 1e-15


def test_quantum_variance_has_the_classical_limit():
    """coth(x / 2) = 2 / x + x / 6 - x^3 / 360 + ...: sigma_q^2 / sigma_c^2 = 1 + x^2 / 12 - x^4 / 720 + O(x^6), x = eps / kT"""
    for T in (1e5, 1e6, 1e8):
        x = sr.mode_energy(LAM) / (sr.K_BOLTZMANN * T)
        ratio = sr.variance(LAM, 0.0, T, True) / sr.variance(LAM, 0.0, T, False)
        assert np.all(np.abs(ratio - (1.0 + x * x / 12.0 - x ** 4 / 720.0)) <= 1e-14 + x ** 6)
    np.testing.assert_allclose(sr.variance(LAM, 0.0, 300.0, False), sr.K_BOLTZMANN * 300.0 / LAM, rtol=1e-15)


def test_quantum_variance_at_low_temperature_is_the_ground_state():
    ground = sr.mode_energy(LAM) / (2.0 * LAM)
    np.testing.assert_array_equal(sr.variance(LAM, 0.0, 0.0, True), ground)
    np.testing.assert_allclose(sr.variance(LAM, 0.0, 1e-3, True), ground, rtol=1e-15)      # x >= 3.9e4: expm1 overflows, coth = 1
    v1 = sr.variance(LAM, 0.0, 1.0, True)
    x = sr.mode_energy(LAM) / sr.K_BOLTZMANN
    np.testing.assert_allclose(v1, ground * (1.0 + 2.0 * np.exp(-x) / (1.0 - np.exp(-x))), rtol=1e-13)
    assert np.all(sr.variance(LAM, 0.0, 0.0, False) == 0.0)
    # the live rule: lambda <= thr has no amplitude, whatever its sign
    v = sr.variance(np.array([-1.0, 0.0, 0.5, 0.5000001, 2.0]), 0.5, 300.0, True)
    assert np.all(v[:3] == 0.0) and np.all(v[3:] > 0.0)


@pytest.mark.parametrize('T', [10.0, 300.0, 2000.0])
def test_free_energy_identity(T):
    """U - T S = sum eps / 2 + kT sum ln(1 - e^-x)"""
    t = sr.thermochemistry(LAM, 0.0, T)
    x = sr.mode_energy(LAM) / (sr.K_BOLTZMANN * T)
    closed = 0.5 * sr.mode_energy(LAM).sum() + sr.K_BOLTZMANN * T * np.log1p(-np.exp(-x)).sum()
    assert abs(t['U'] - T * t['S'] - closed) <= 1e-13 * (t['U_abs'] + T * t['S_abs'])
    assert abs(t['F'] - closed) <= 1e-13 * t['F_abs']


def test_thermochemistry_limits():
    n = len(LAM)
    zpe = 0.5 * sr.mode_energy(LAM).sum()
    t0 = sr.thermochemistry(LAM, 0.0, 0.0)
    assert t0['U'] == zpe and t0['F'] == zpe and t0['S'] == 0.0 and t0['Cv'] == 0.0
    hot = sr.thermochemistry(LAM, 0.0, 1e7)                 # x <= 4e-4: C_v = k_B (1 - x^2 / 12) per mode, U = kT per mode
    assert abs(hot['Cv'] / (n * sr.K_BOLTZMANN) - 1.0) <= 2e-8
    assert abs(hot['U'] / (n * sr.K_BOLTZMANN * 1e7) - 1.0) <= 2e-8
    cold = sr.thermochemistry(LAM, 0.0, 1.0)                # x >= 39
    assert 0.0 < cold['Cv'] < 1e-12 * sr.K_BOLTZMANN and abs(cold['U'] - zpe) <= 1e-15
    # modes at or below the threshold carry nothing
    a, b = sr.thermochemistry(LAM, 0.05, 300.0), sr.thermochemistry(LAM[2:], 0.0, 300.0)
    assert a == b


def test_reference_sample_is_the_definition():
    rng = np.random.default_rng(3)
    L = np.linalg.qr(rng.standard_normal((9, 9)))[0].T
    lam = np.array([-0.5, 0, 0, 0, 0, 0, 0.3, 1.0, 2.0])
    m = np.array([1.008, 12.011, 15.999])
    pos, xi = rng.standard_normal((3, 3)), rng.standard_normal((4, 9))
    r = sr.sample(L, lam, 1e-6, m, pos, xi, 300.0, False)
    assert r['n_skipped'] == 1 and r['pos'].shape == (4, 3, 3) and np.all(r['q'][:, :6] == 0.0)
    # mass-weighted displacement back onto the modes gives q; the energy is kT / 2 sum xi^2 over the live modes
    mw = (r['dx'] * np.sqrt(m)[None, :, None]).reshape(4, 9)
    np.testing.assert_allclose(mw @ L.T, r['q'], atol=1e-13)
    np.testing.assert_allclose(r['energy'], 0.5 * sr.K_BOLTZMANN * 300.0 * (xi[:, 6:] ** 2).sum(1), rtol=1e-13)


def test_synthetic_inputs():
    for with_masses in (False, True):
        a, b = sr.synthetic_molecules(with_masses), sr.synthetic_molecules(with_masses)
        assert [m['n'] for m in a] == [1, 2, 0, 3, 9, 21, 42]
        for x, y in zip(a, b):
            M = 3 * x['n']
            assert all(np.array_equal(x[k], y[k]) for k in ('lam', 'modes', 'pos')) and (x['masses'] is None) == (not with_masses)
            assert x['lam'].dtype == np.float32 and x['modes'].shape == (M, M) and x['modes'].dtype == np.float32
            assert np.all(np.diff(x['lam']) >= 0)
            if M:
                L = x['modes'].astype(np.float64)
                assert np.abs(L @ L.T - np.eye(M)).max() <= 4 * sr.EPS32
            if x['n'] >= 3:
                lam = x['lam'].astype(np.float64)
                thr = float(sr.default_threshold(M, lam[-1]))
                sides = ((thr, 2 * thr), (0.25 * thr, thr), (-thr, -0.25 * thr), (-2 * thr, -thr)) if x['n'] > 3 else \
                    ((thr, 2 * thr), (0.25 * thr, thr), (-2 * thr, -thr))
                for lo, hi in sides:
                    assert np.count_nonzero((lam > lo) & (lam < hi)) >= 1, (x['n'], lo)
                assert np.count_nonzero(lam == 0.0) >= 3 and np.count_nonzero(lam < -thr) >= 1
            if x['n'] >= 9:
                assert np.float32(thr) in x['lam'] and np.float32(-thr) in x['lam']
    s1, s33 = sr.synthetic_draws(a, 1), sr.synthetic_draws(a, 33)
    assert all(np.array_equal(p, q[:1]) and q.shape == (33, 3 * m['n']) for p, q, m in zip(s1, s33, a))


def host_modes(modes=True):
    """a NormalModes of one water-sized molecule on the host: enough for the checks that come before any device work"""
    from newtonnet_amd import vibrations as vib
    lam = torch.tensor([0.0] * 6 + [0.5, 1.0, 2.0])
    return vib.NormalModes(eigenvalues=lam, frequencies=lam.sqrt() * vib.WAVENUMBER_PER_SQRT_EIGENVALUE,
                           modes=torch.eye(9).reshape(-1) if modes else None, ptr=torch.tensor([0, 9]), blk_ptr=torch.tensor([0]),
                           masses=None, threshold=torch.tensor([1e-5]), pos=torch.zeros(3, 3), cell=torch.zeros(1, 3, 3),
                           z=torch.tensor([8, 1, 1]), zero_point_energy=torch.tensor([0.1]), _counts=[3], _offsets=[0], _blk_offsets=[0])


def test_sample_validates_its_arguments_before_any_device_work():
    nm = host_modes()
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='n_samples'):
            nm.sample(bad, 300.0)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='temperature'):
            nm.sample(1, bad)
        with pytest.raises(ValueError, match='temperature'):
            nm.thermochemistry(bad)
    with pytest.raises(ValueError, match='modes=False'):
        host_modes(modes=False).sample(1, 300.0)
    with pytest.raises(ValueError, match='xi'):
        nm.sample(2, 300.0, xi=torch.zeros(9))
    with pytest.raises(ValueError, match='xi'):
        nm.sample(2, 300.0, xi=torch.zeros(2, 9))
    with pytest.raises(ValueError, match='float32'):
        nm.sample(2, 300.0, xi=torch.zeros(18, dtype=torch.float64))
    with pytest.raises(ValueError, match='pos'):
        nm.sample(1, 300.0, pos=torch.zeros(4, 3))
    with pytest.raises(ValueError, match='pos'):
        nm.sample(1, 300.0, cell=torch.zeros(2, 3, 3))
    with pytest.raises(ValueError, match='z:'):
        nm.sample(1, 300.0, z=torch.tensor([8, 1]))
    with pytest.raises(RuntimeError, match='cuda'):          # valid arguments: refused for the device, like eig_blocks
        nm.sample(2, 300.0, xi=torch.zeros(18))
    t = nm.thermochemistry(0.0)                              # T = 0 needs no kernel: U = F = the zero-point energy
    assert torch.equal(t.U, nm.zero_point_energy) and torch.equal(t.F, nm.zero_point_energy)
    assert torch.count_nonzero(t.S) == 0 and torch.count_nonzero(t.Cv) == 0
