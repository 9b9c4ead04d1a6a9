"""CPU-side checks of the batched molecular dynamics (newtonnet_amd/dynamics.py, csrc/md.hip): the C ABI exports the kernels, the
unit constant and the Langevin coefficients have the values and limits they must have, the fp64 restatement the GPU tests compare
against (tests/md_ref.py) integrates the way BAOAB / velocity Verlet must, and arguments are refused before any device work."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import md_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_symbols_are_declared_listed_and_exported():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for name in ('nnhip_md_step', 'nnhip_md_kinetic'):
        assert name in declared and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.nnhip_version() == 113
    assert (hip.MD_FINISH, hip.MD_BEGIN) == (mr.FINISH, mr.BEGIN) == (1, 2)
    assert re.search(r'#define NNHIP_MD_FINISH 1\b', header) and re.search(r'#define NNHIP_MD_BEGIN 2\b', header)
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bmd\b.*\)', f.read(), re.M)


def test_femtosecond_in_internal_units():
    from newtonnet_amd import dynamics as dyn
    assert abs(dyn.FS - 1e-15 * 9.8226948e13) <= 1e-7 * dyn.FS
    assert abs(dyn.FS - 0.0982269) < 1e-6


def test_langevin_coefficients_limits_and_ladder():
    from newtonnet_amd import dynamics as dyn
    from newtonnet_amd.vibrations import K_BOLTZMANN
    m = torch.tensor([1.008, 12.011, 15.999, 1.008, 12.011], dtype=torch.float32)
    batch = torch.tensor([0, 0, 0, 1, 1])
    m64 = m.double().numpy()
    c1, sigma = dyn.langevin_coefficients(0.5, 0.0, 300.0, m, batch)
    assert c1 == 1.0 and sigma.dtype == torch.float32 and torch.all(sigma == 0)
    c1, sigma = dyn.langevin_coefficients(0.5, 1e4, 300.0, m, batch)          # gamma dt = 5000
    assert c1 == 0.0
    np.testing.assert_allclose(sigma.double().numpy() ** 2, K_BOLTZMANN * 300.0 / m64, rtol=2e-7)
    c1, sigma = dyn.langevin_coefficients(0.5, 0.02, 300.0, m, batch)
    assert c1 == float(np.float32(math.exp(-0.01)))
    want = np.sqrt((1.0 - math.exp(-0.02)) * K_BOLTZMANN * 300.0 / m64)
    assert np.array_equal(sigma.numpy(), want.astype(np.float32))             # fp64, rounded once
    ladder = torch.tensor([200.0, 400.0])
    _, s2 = dyn.langevin_coefficients(0.5, 0.02, ladder, m, batch)
    T = np.array([200.0, 200.0, 200.0, 400.0, 400.0])
    assert np.array_equal(s2.numpy(), np.sqrt((1.0 - math.exp(-0.02)) * K_BOLTZMANN * T / m64).astype(np.float32))
    with pytest.raises(ValueError):
        dyn.langevin_coefficients(0.5, -1.0, 300.0, m, batch)


def test_maxwell_boltzmann_is_one_draw_without_net_momentum():
    from newtonnet_amd import dynamics as dyn
    from newtonnet_amd.vibrations import K_BOLTZMANN
    m = torch.tensor([1.008, 12.011, 15.999] * 4, dtype=torch.float32)
    batch = torch.tensor([0] * 5 + [1] * 7)
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    v = dyn.maxwell_boltzmann(m, batch, torch.tensor([100.0, 300.0]), g1, n_mol=2)
    xi = torch.randn((12, 3), generator=g2)
    assert torch.equal(torch.randn(4, generator=g1), torch.randn(4, generator=g2))       # exactly one (N, 3) draw was taken
    raw = xi * torch.sqrt(K_BOLTZMANN * torch.tensor([100.0] * 5 + [300.0] * 7).double() / m.double()).float()[:, None]
    for b in (0, 1):
        sel = batch == b
        p = (m[sel, None].double() * v[sel].double()).sum(0)
        assert p.abs().max() <= 1e-6 * (m[sel, None] * v[sel].abs()).sum()
        shift = (raw[sel] - v[sel]).double()
        assert (shift - shift[0]).abs().max() <= 1e-6 * raw.abs().max()                   # a rigid shift per molecule, nothing else


def test_reference_conserves_energy_to_second_order():
    """gamma = 0 on a 1-D harmonic oscillator (omega = 1): the energy error over 1e4 steps stays bounded and is O(dt^2)"""
    e1, e2 = mr.harmonic_energy_error(0.1, 10000), mr.harmonic_energy_error(0.05, 10000)
    # velocity Verlet conserves the shadow energy E + (dt^2 / 8)(...): the error oscillates, it never exceeds dt^2 / 8 x 2 E_0 k / m
    assert e1 <= 0.1 ** 2 / 8.0 * 1.001 and e2 <= 0.05 ** 2 / 8.0 * 1.001
    assert abs(e1 / e2 - 4.0) <= 0.4
    assert mr.harmonic_energy_error(0.1, 1000) <= e1 * 1.0001               # bounded: ten times the run adds nothing


def test_reference_free_particle_variance():
    """F = 0, v_0 = 0: Var v_n = (k_B T / m)(1 - c1^(2n)) in expectation, from the recurrence of the O step -- on the formula"""
    from newtonnet_amd.vibrations import K_BOLTZMANN
    kTm = K_BOLTZMANN * 300.0 / 12.011
    for gdt in (1e-3, 0.01, 0.7):
        c1 = math.exp(-gdt)
        sigma = math.sqrt((1.0 - c1 * c1) * kTm)
        for n in (1, 7, 1000):
            assert abs(mr.free_variance(c1, sigma, n) - kTm * (1.0 - c1 ** (2 * n))) <= 1e-12 * kTm
    # and md_step's O step is that map: v -> c1 v + sigma xi, positions drift by dth (v_before + v_after)
    v, xi = np.array([[0.3, -0.2, 0.1]]), np.array([[1.0, -2.0, 0.5]])
    out = mr.md_step(mr.BEGIN, np.zeros((1, 3)), v, np.zeros((1, 3)), np.array([0.01]), sigma=np.array([0.2]), xi=xi, c1=0.9, dth=0.05)
    np.testing.assert_allclose(out['v'], 0.9 * v + 0.2 * xi, rtol=1e-15)
    np.testing.assert_allclose(out['x'], 0.05 * (v + out['v']), rtol=1e-15)


def test_reference_bound_is_first_order_in_eps32():
    rng = np.random.default_rng(0)
    x, v, F = rng.uniform(-8, 8, (5, 3)), rng.uniform(-0.2, 0.2, (5, 3)), rng.uniform(-5, 5, (5, 3))
    hk, m = np.full(5, 0.002), np.full(5, 12.0)
    out = mr.md_step(mr.FINISH | mr.BEGIN, x, v, F, hk, m, dth=0.025)
    assert np.all(out['bx'] >= mr.C_MD * mr.EPS32 * np.abs(out['x'])) and np.all(out['bx'] <= 8 * mr.EPS32 * (np.abs(out['x']) + 1))
    assert np.all(out['bv'] >= mr.C_MD * mr.EPS32 * np.abs(out['v'])) and np.all(out['bv'] <= 8 * mr.EPS32 * (np.abs(out['v']) + 1))
    assert np.all(out['bke'] >= mr.C_MD * mr.EPS32 * out['ke']) and np.all(out['bke'] <= 16 * mr.EPS32 * out['ke'] + 1e-12)
    fs = mr.full_step(x, v, F, F, hk, m, dth=0.025)
    # chaining: BEGIN then FINISH with the same forces is two half kicks, and the second launch's bound contains the first's
    np.testing.assert_allclose(fs['v'], v + 2 * hk[:, None] * F, rtol=1e-14)
    begin = mr.md_step(mr.BEGIN, x, v, F, hk, dth=0.025)
    assert np.all(fs['bv'] > begin['bv']) and np.array_equal(fs['x'], begin['x']) and np.array_equal(fs['bx'], begin['bx'])


class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force']


def _inputs(n=3, b=1):
    return (torch.ones(n, dtype=torch.long), torch.zeros(n, 3), torch.zeros(b, 3, 3), torch.zeros(n, dtype=torch.long))


def test_dynamics_validates_before_any_device_work():
    from newtonnet_amd.dynamics import Dynamics
    z, pos, cell, batch = _inputs()
    train = _FakeModel()
    train.training = True
    with pytest.raises(ValueError, match='eval'):
        Dynamics(train, z, pos, cell, batch)
    energy_only = _FakeModel()
    energy_only.output_properties = ['energy']
    with pytest.raises(ValueError, match='gradient_force'):
        Dynamics(energy_only, z, pos, cell, batch)
    ok = _FakeModel()
    with pytest.raises(ValueError, match='temperature'):
        Dynamics(ok, z, pos, cell, batch, friction=0.01)
    with pytest.raises(ValueError, match='pos'):
        Dynamics(ok, z, torch.zeros(3, 2), cell, batch)
    with pytest.raises(ValueError, match='cell'):
        Dynamics(ok, z, pos, torch.zeros(3, 3), batch)
    with pytest.raises(ValueError, match='batch'):
        Dynamics(ok, z, pos, cell, batch[:2])
    with pytest.raises(ValueError, match='float32'):
        Dynamics(ok, z, pos.double(), cell, batch)
    with pytest.raises(ValueError, match='masses'):
        Dynamics(ok, z, pos, cell, batch, masses=torch.ones(2))
    with pytest.raises(ValueError, match='velocities'):
        Dynamics(ok, z, pos, cell, batch, velocities=torch.zeros(3))
    with pytest.raises(ValueError, match='fixed'):
        Dynamics(ok, z, pos, cell, batch, fixed=torch.zeros(3))
    with pytest.raises(ValueError, match='timestep'):
        Dynamics(ok, z, pos, cell, batch, timestep=0.0)
    with pytest.raises(ValueError, match='friction'):
        Dynamics(ok, z, pos, cell, batch, friction=-1.0, temperature=300.0)
    with pytest.raises(ValueError, match='temperature'):
        Dynamics(ok, z, pos, cell, batch, temperature=-5.0)
    with pytest.raises(ValueError, match='temperature'):
        Dynamics(ok, z, pos, cell, batch, temperature=torch.tensor([300.0, 200.0]))      # one molecule, two temperatures
    with pytest.raises(RuntimeError, match='MI355X'):                                     # CPU tensors: no CPU path
        Dynamics(ok, z, pos, cell, batch)


def test_run_md_validates_before_any_device_work():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype = torch.device('cpu'), torch.float32
    calc.model = _FakeModel()
    a, b = FakeAtoms([8, 1, 1], np.zeros((3, 3))), FakeAtoms([6, 1], np.zeros((2, 3)))
    with pytest.raises(ValueError, match='n_steps'):
        calc.run_md(a, -1)
    with pytest.raises(ValueError, match='n_steps'):
        calc.run_md(a, 2.5)
    with pytest.raises(ValueError, match='record_every'):
        calc.run_md(a, 4, record_every=-2)
    with pytest.raises(ValueError, match='sizes'):
        calc.run_md([a, b], 4)
    with pytest.raises(ValueError, match='temperature'):
        calc.run_md(a, 4, friction=0.01)
    with pytest.raises(ValueError, match='timestep'):
        calc.run_md(a, 4, timestep=-0.5)
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.run_md(a, 4)
