"""CPU-side checks of constant-pressure dynamics (newtonnet_amd/npt.py, csrc/npt.hip): the C ABI exports the two kernels, the unit
constant and the barostat's coefficients have the values they must have, arguments are refused before any device work, the fp64
restatement the GPU tests compare against (tests/npt_ref.py) does what the header says, and the scheme itself -- the fp64 host loop
alone -- samples the ideal gas's volume distribution."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import md_ref as mr
from tests import npt_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the ideal-gas ensemble (shared with tests/test_hip_npt.py): N atoms, kT = P0 = 1, a P0 = 0.02, a burn-in of 20 / (a P0) steps, then
# snapshots one relaxation time 1 / (a P0) x 2 apart; the exact mean volume of the isothermal-isobaric ideal gas is (N + 1) kT / P0
GAS = dict(n_atoms=4, kT=1.0, p0=1.0, a=0.02, c1=float(np.exp(-0.5)), n_burn=1000, n_snap=10, every=100)
GAS_EXACT = (GAS['n_atoms'] + 1) * GAS['kT'] / GAS['p0']


def gas_margin(mean_volume, standard_error):
    """5 standard errors plus the first-order (Euler) bias a P0 <V> of the discretised barostat"""
    return 5.0 * standard_error + GAS['a'] * GAS['p0'] * mean_volume


_host_gas = {}


def host_gas(n_sys=4096, seed=1):
    """the fp64 loop's volumes [n_snap, n_sys], computed once per process"""
    if (n_sys, seed) not in _host_gas:
        _host_gas[(n_sys, seed)] = nr.host_loop(n_sys, seed=seed, **GAS)
    return _host_gas[(n_sys, seed)]


def test_kernel_symbols_are_declared_listed_and_exported():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for name in ('nnhip_npt_barostat', 'nnhip_npt_step'):
        assert name in declared and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bnpt\b.*\)', f.read(), re.M)
    assert callable(hip.npt_barostat) and callable(hip.npt_step)


def test_units_and_coefficients():
    from newtonnet_amd import npt
    from newtonnet_amd.vibrations import K_BOLTZMANN
    assert abs(npt.BAR - 6.241509e-7) <= 1e-6 * 6.241509e-7 and npt.BAR == nr.BAR          # 1 bar in eV / A^3
    assert abs(npt.AMU_PER_A3_IN_G_PER_CM3 - 1.660539) < 1e-6
    a, p0, s2 = npt.barostat_coefficients(0.5, 1000.0, 4.5e-5, 1.0, 300.0, 3)
    assert all(t.dtype == torch.float32 and tuple(t.shape) == (3,) for t in (a, p0, s2))
    a64 = (4.5e-5 / npt.BAR) * (0.5 / 1000.0)                                              # beta_T dt / tau_p, A^3 / eV
    assert np.array_equal(a.numpy(), np.full(3, a64).astype(np.float32)) and abs(a64 - 0.03605) < 1e-5
    assert np.array_equal(p0.numpy(), np.full(3, npt.BAR).astype(np.float32))
    assert np.array_equal(s2.numpy(), np.full(3, 2.0 * K_BOLTZMANN * 300.0 * a64).astype(np.float32))     # fp64, rounded once
    # one value per system, and the limits: no coupling without compressibility, no noise at T = 0
    P, T = torch.tensor([1.0, 1000.0, -50.0]), torch.tensor([100.0, 300.0, 0.0])
    a, p0, s2 = npt.barostat_coefficients(1.0, 500.0, 1e-4, P, T, 3)
    a64 = (1e-4 / npt.BAR) * (1.0 / 500.0)
    assert np.array_equal(p0.numpy(), (P.double().numpy() * npt.BAR).astype(np.float32))
    assert np.array_equal(s2.numpy(), (2.0 * K_BOLTZMANN * T.double().numpy() * a64).astype(np.float32)) and float(s2[2]) == 0.0
    a, _, s2 = npt.barostat_coefficients(0.5, 1000.0, 0.0, 1.0, 300.0, 2)
    assert not a.any() and not s2.any()
    for bad in (dict(timestep_fs=0.0), dict(barostat_time_fs=0.0), dict(barostat_time_fs=-1.0), dict(barostat_time_fs=float('inf')),
                dict(compressibility_per_bar=-1e-5), dict(compressibility_per_bar=float('nan')), dict(pressure_bar=float('inf')),
                dict(pressure_bar=torch.ones(2)), dict(temperature=torch.ones(4))):
        kw = dict(timestep_fs=0.5, barostat_time_fs=1000.0, compressibility_per_bar=4.5e-5, pressure_bar=1.0, temperature=300.0, n_mol=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            npt.barostat_coefficients(**kw)


class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force', 'virial']


def _inputs(n=3, b=1):
    return (torch.ones(n, dtype=torch.long), torch.zeros(n, 3), 10.0 * torch.eye(3).repeat(b, 1, 1), torch.zeros(n, dtype=torch.long))


def test_constant_pressure_validates_before_any_device_work():
    from newtonnet_amd.npt import ConstantPressure, NPTTrajectory
    from newtonnet_amd.dynamics import Dynamics, Trajectory
    assert issubclass(ConstantPressure, Dynamics) and issubclass(NPTTrajectory, Trajectory)
    z, pos, cell, batch = _inputs()
    ok = _FakeModel()
    no_virial = _FakeModel()
    no_virial.output_properties = ['energy', 'gradient_force']
    with pytest.raises(ValueError, match='virial'):
        ConstantPressure(no_virial, z, pos, cell, batch, 1.0, 300.0)
    train = _FakeModel()
    train.training = True
    with pytest.raises(ValueError, match='eval'):
        ConstantPressure(train, z, pos, cell, batch, 1.0, 300.0)
    with pytest.raises(ValueError, match='fixed'):
        ConstantPressure(ok, z, pos, cell, batch, 1.0, 300.0, fixed=torch.zeros(3, dtype=torch.bool))
    with pytest.raises(ValueError, match='constraints'):
        ConstantPressure(ok, z, pos, cell, batch, 1.0, 300.0, constraints='h-bonds')
    with pytest.raises(ValueError, match='temperature'):
        ConstantPressure(ok, z, pos, cell, batch, 1.0, None)
    with pytest.raises(ValueError, match='temperature'):
        ConstantPressure(ok, z, pos, cell, batch, 1.0, -5.0)
    for kw in (dict(compressibility=-1e-5), dict(compressibility=float('nan')), dict(compressibility=float('inf')),
               dict(barostat_time=-1.0), dict(barostat_time=float('nan')), dict(barostat_time=0.0), dict(timestep=0.0),
               dict(friction=-0.1)):
        with pytest.raises(ValueError):
            ConstantPressure(ok, z, pos, cell, batch, 1.0, 300.0, **kw)
    with pytest.raises(ValueError, match='pressure'):
        ConstantPressure(ok, z, pos, cell, batch, torch.ones(2), 300.0)
    with pytest.raises(ValueError, match='pressure'):
        ConstantPressure(ok, z, pos, cell, batch, float('nan'), 300.0)
    with pytest.raises(ValueError, match='pos'):
        ConstantPressure(ok, z, torch.zeros(3, 2), cell, batch, 1.0, 300.0)
    # a stress head serves as well; with sound arguments the first thing missing is the device
    stress = _FakeModel()
    stress.output_properties = ['energy', 'gradient_force', 'stress']
    for model in (ok, stress):
        with pytest.raises(RuntimeError, match='MI355X'):
            ConstantPressure(model, z, pos, cell, batch, 1.0, 300.0)


def test_fp64_restatement_of_the_barostat_does_what_the_header_says():
    rng = np.random.default_rng(3)
    sizes = [0, 1, 7]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    N, B = ptr[-1], 3
    v, m = rng.normal(0, 0.1, (N, 3)).astype(np.float32), rng.uniform(1, 16, N).astype(np.float32)
    cell = (np.eye(3) * [8.0, 9.0, 10.0] + rng.normal(0, 0.5, (B, 3, 3))).astype(np.float32)
    W = rng.normal(0, 1.0, (B, 3, 3)).astype(np.float32)
    a, p0 = np.array([0.0, 0.03, 0.03], dtype=np.float32), np.full(B, 6e-4, dtype=np.float32)
    out = nr.barostat(v, m, ptr, cell, W, a, p0)
    K = np.array([(0.5 * m[ptr[b]:ptr[b + 1], None].astype(np.float64) * v[ptr[b]:ptr[b + 1]].astype(np.float64) ** 2).sum() for b in range(B)])
    V = np.linalg.det(cell.astype(np.float64))
    P = (2.0 * K + np.trace(W.astype(np.float64), axis1=1, axis2=2)) / (3.0 * V)
    np.testing.assert_allclose(out['ke'], K, rtol=1e-12)
    np.testing.assert_allclose(out['volume'], V, rtol=1e-12)
    np.testing.assert_allclose(out['pressure'], P, rtol=1e-12)
    np.testing.assert_allclose(out['deps'], -a.astype(np.float64) * (p0 - P), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(out['mu'], np.exp(out['deps'] * nr.THIRD32), rtol=1e-12)
    np.testing.assert_allclose(out['mu'] * out['inv_mu'], 1.0, rtol=1e-12)
    np.testing.assert_allclose(out['cell_out'], out['mu'][:, None, None] * cell, rtol=1e-12)
    assert out['mu'][0] == 1.0 and out['deps'][0] == 0.0 and np.array_equal(out['cell_out'][0], cell[0].astype(np.float64))   # a = 0
    # the bounds are first order: a few 2^-24 of the values (not zero, not percent)
    for key in ('volume', 'pressure', 'mu'):
        rel = out['b' + key][1:] / np.abs(out[key][1:])
        assert np.all(rel > 0.5 * nr.EPS32) and np.all(rel < 1e-4), (key, rel)
    # with noise: deps gains sqrt(s2 / V) xi
    s2, xi = np.full(B, 2e-3, dtype=np.float32), rng.standard_normal(B).astype(np.float32)
    noisy = nr.barostat(v, m, ptr, cell, W, a, p0, s2=s2, xi=xi)
    np.testing.assert_allclose(noisy['deps'] - (-a.astype(np.float64) * (p0 - P)), np.sqrt(s2.astype(np.float64) / V) * xi, rtol=1e-9)
    # a pending kick enters the kinetic energy
    F, hk = rng.normal(0, 1, (N, 3)).astype(np.float32), (0.02 / m).astype(np.float32)
    kicked = nr.barostat(v, m, ptr, cell, W, a, p0, F=F, hk=hk)
    vk = v.astype(np.float64) + hk[:, None].astype(np.float64) * F
    np.testing.assert_allclose(kicked['ke'][2], (0.5 * m[1:, None] * vk[1:] ** 2).sum(), rtol=1e-12)


def test_fp64_restatement_of_the_step_reduces_to_md_step_and_rescales():
    rng = np.random.default_rng(4)
    N = 9
    x, v, F = rng.uniform(-5, 5, (N, 3)).astype(np.float32), rng.normal(0, 0.1, (N, 3)).astype(np.float32), rng.normal(0, 1, (N, 3)).astype(np.float32)
    m = rng.uniform(1, 16, N).astype(np.float32)
    hk, sigma, xi = (0.02 / m).astype(np.float32), (0.01 / np.sqrt(m)).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)
    mol = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2])
    ones = np.ones(3)
    for flags in (mr.BEGIN, mr.FINISH, mr.BEGIN | mr.FINISH):
        got = nr.npt_step(flags, x, v, F, hk, ones, ones, mol, m if flags & mr.FINISH else None, sigma, xi, 0.99, 0.05)
        want = mr.md_step(flags, x, v, F, hk, m if flags & mr.FINISH else None, sigma, xi, 0.99, 0.05)
        for key in ('x', 'v', 'ke', 'bx', 'bv', 'bke'):
            assert (got[key] is None) == (want[key] is None)
            if got[key] is not None:
                assert np.array_equal(got[key], want[key]), (flags, key)           # mu = 1: the same chain and the same bound
    mu = np.array([1.001, 0.999, 1.0])
    got = nr.npt_step(mr.BEGIN, x, v, F, hk, mu, 1.0 / mu, mol, dth=0.05)
    vk = (v.astype(np.float64) + hk[:, None].astype(np.float64) * F) / mu[mol][:, None]
    np.testing.assert_allclose(got['v'], vk, rtol=1e-12)
    np.testing.assert_allclose(got['x'], mu[mol][:, None] * x + 2 * 0.05 * vk, rtol=1e-12)


def test_ideal_gas_volume_of_the_fp64_loop():
    """N = 4 atoms, zero forces and virial, Langevin, a P0 = 0.02, 4096 systems, burn-in 20 / (a P0) = 1000 steps, ten snapshots 100
    steps apart: the mean volume is (N + 1) kT / P0 = 5 within 5 standard errors (across the independent systems) plus the Euler
    bias a P0 <V>.  A Jacobian term too few or too many in the barostat's drift gives N kT / P0 = 4 or (N + 2) kT / P0 = 6."""
    mean, se = nr.mean_and_standard_error(host_gas())
    print(f'ideal gas, fp64 loop: <V> = {mean:.4f} +- {se:.4f} (exact {GAS_EXACT}), margin {gas_margin(mean, se):.4f}')
    assert 0.0 < se < 0.05
    assert abs(mean - GAS_EXACT) <= gas_margin(mean, se)
    assert gas_margin(mean, se) < 0.5                       # the margin separates 5 from 4 and 6
