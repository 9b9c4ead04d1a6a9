"""CPU-side checks of the bias on collective variables (newtonnet_amd/metadynamics.py, csrc/bias.hip): the C ABI exports the two
entry points and the header's constants are the Python ones, arguments are refused before any device work, and the reference the GPU
tests compare against (tests/bias_ref.py) is right -- its gradients are the central differences of its own values, they carry no
net force and no net torque, its bias force is minus the gradient of V + U, and its deposits have the well-tempered heights."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import bias_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_listed_and_exported_and_the_constants_agree():
    from newtonnet_amd import abi, hip, metadynamics
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for name in ('nnhip_bias_step', 'nnhip_bias_eval'):
        assert name in declared and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bbias\b.*\)', f.read(), re.M)

    def define(name):
        return int(re.search(rf'#define NNHIP_BIAS_{name} (\S+)', header).group(1))
    assert define('MAX_CVS') == hip.BIAS_MAX_CVS == br.MAX_CVS == 2
    assert (define('DISTANCE'), define('ANGLE'), define('TORSION')) == (hip.BIAS_DISTANCE, hip.BIAS_ANGLE, hip.BIAS_TORSION) \
        == (br.DISTANCE, br.ANGLE, br.TORSION) == (1, 2, 3)
    assert define('DEPOSIT') == hip.BIAS_DEPOSIT == br.DEPOSIT == 1
    assert define('THREADS') == hip.BIAS_THREADS == br.THREADS == 256
    assert define('STATUS_INVALID') == hip.BIAS_STATUS_INVALID == br.STATUS_INVALID == abi.CONSTANTS['NNHIP_BIAS_STATUS_INVALID']
    assert lib.nnhip_version() == 113
    from newtonnet_amd.vibrations import K_BOLTZMANN
    assert K_BOLTZMANN == br.K_BOLTZMANN and metadynamics.TWO_PI32 == br.TWO_PI32


# ---- arguments ----------------------------------------------------------------------------------------------------------------------

class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force']

    def metadynamics(self, *a, **kw):
        from newtonnet_amd.models import NewtonNet
        return NewtonNet.metadynamics(self, *a, **kw)


def _inputs(n=5, g=2):
    return (torch.ones(n * g, dtype=torch.long), torch.zeros(n * g, 3), torch.zeros(g, 3, 3), torch.arange(g).repeat_interleave(n))


CVS = [('torsion', 0, 1, 2, 3), ('distance', 0, 4)]
GOOD = dict(temperature=300.0, friction=0.02, hill_height=0.01, hill_width=[0.3, 0.1], pace=5)


def _make(model, cvs=CVS, inputs=None, **kw):
    a = dict(GOOD, **kw)
    z, pos, cell, batch = inputs or _inputs()
    return model.metadynamics(z, pos, cell, batch, cvs, a.pop('temperature'), a.pop('friction'), a.pop('hill_height'),
                              a.pop('hill_width'), a.pop('pace'), **a)


def test_metadynamics_validates_before_any_device_work():
    ok = _FakeModel()
    train = _FakeModel()
    train.training = True
    with pytest.raises(ValueError, match='eval'):
        _make(train)
    energy_only = _FakeModel()
    energy_only.output_properties = ['energy']
    with pytest.raises(ValueError, match='gradient_force'):
        _make(energy_only)
    bad_cvs = [[('bond', 0, 1)], [('distance', 0)], [('distance', 0, 1, 2)], [('angle', 0, 1)], [('torsion', 0, 1, 2)],     # kinds, arities
               [('distance', 0, 5)], [('distance', -1, 2)], [('angle', 0, 1, 2.5)], [('distance', 0, True)],                  # indices
               [('distance', 1, 1)], [('angle', 0, 1, 0)], [('torsion', 0, 1, 2, 1)],                                         # repeated atoms
               [('distance', 0, 1), ('distance', 1, 2), ('distance', 2, 3)],                                                # more than two
               [[('distance', 0, 1)]], [[('distance', 0, 1)], [('distance', 0, 1)], []],                                    # one list per system
               'torsion', [('distance', 0, 1), 7]]
    for bad in bad_cvs:
        with pytest.raises(ValueError, match='cvs'):
            _make(ok, cvs=bad)
    for bad in (0.0, -0.1, [0.3, 0.0], [0.3], [0.3, 0.1, 0.2], float('nan'), 'x'):
        with pytest.raises(ValueError, match='hill_width'):
            _make(ok, hill_width=bad)
    for bad in (-0.01, float('nan'), float('inf'), 'x'):
        with pytest.raises(ValueError, match='hill_height'):
            _make(ok, hill_height=bad)
    for bad in (1.0, 0.5, -2.0, float('nan'), float('inf'), 'x'):
        with pytest.raises(ValueError, match='bias_factor'):
            _make(ok, bias_factor=bad)
    for bad in (-1, 2.5, float('nan'), 'x', None, True):
        with pytest.raises(ValueError, match='pace'):
            _make(ok, pace=bad)
    for bad in (0, -1, 1.5, 'x', None, True):
        with pytest.raises(ValueError, match='walkers'):
            _make(ok, walkers=bad)
    for bad in (0, -4, 2.5):
        with pytest.raises(ValueError, match='hill_capacity'):
            _make(ok, hill_capacity=bad)
    # restraints: both or neither, and a shape that broadcasts to [G, W, n_cv] = [2, 3, 2]
    with pytest.raises(ValueError, match='restraint'):
        _make(ok, walkers=3, restraint_k=1.0)
    with pytest.raises(ValueError, match='restraint'):
        _make(ok, walkers=3, restraint_center=1.0)
    for bad in (np.zeros(3), np.zeros((3, 3, 2)), np.zeros((2, 2, 2)), np.zeros((2, 3, 2, 1)), 'x'):
        with pytest.raises(ValueError, match='restraint'):
            _make(ok, walkers=3, restraint_k=bad, restraint_center=0.0)
        with pytest.raises(ValueError, match='restraint'):
            _make(ok, walkers=3, restraint_k=1.0, restraint_center=bad)
    for bad in (-1.0, float('nan')):
        with pytest.raises(ValueError, match='restraint'):
            _make(ok, restraint_k=bad, restraint_center=0.0)
    # depositing needs a thermostat; friction = 0 is fine without hills
    with pytest.raises(ValueError, match='friction'):
        _make(ok, friction=0.0)
    with pytest.raises(ValueError, match='friction'):
        _make(ok, friction=-0.1)
    with pytest.raises(ValueError, match='variable'):
        _make(ok, cvs=[], hill_width=1.0)
    with pytest.raises(ValueError, match='temperature'):
        _make(ok, temperature=None)
    with pytest.raises(ValueError, match='temperature'):
        _make(ok, temperature=None, friction=0.0, pace=0, bias_factor=5.0)
    with pytest.raises(ValueError, match='timestep'):
        _make(ok, timestep=0.0)
    with pytest.raises(ValueError, match='pos'):
        _make(ok, inputs=(_inputs()[0], torch.zeros(10, 2)) + _inputs()[2:])
    with pytest.raises(ValueError, match='fixed'):
        _make(ok, fixed=torch.zeros(10))
    # everything valid: CPU tensors are the one thing left to refuse
    W3 = dict(walkers=3)
    for good in (dict(), dict(bias_factor=8.0), dict(friction=0.0, pace=0), dict(friction=0.0, hill_height=0.0), dict(cvs=[], pace=0, hill_width=1.0),
                 dict(cvs=[[('angle', 0, 1, 2)], []], hill_width=0.2), dict(cvs=[[], []], pace=0, hill_width=[]),
                 dict(W3, restraint_k=2.0, restraint_center=[1.0, 2.0]), dict(W3, restraint_k=np.ones((2, 3, 2)), restraint_center=np.zeros((3, 1))),
                 dict(W3, restraint_k=torch.ones(2, 1, 1), restraint_center=0.0), dict(hill_width=0.2, cvs=[('distance', 0, 1)]),
                 dict(temperature=torch.tensor([300.0, 320.0]), bias_factor=4.0)):
        with pytest.raises(RuntimeError, match='MI355X'):
            _make(ok, **good)
    from newtonnet_amd.dynamics import Dynamics
    from newtonnet_amd.metadynamics import Metadynamics
    import inspect
    assert Metadynamics._recorded_steps is Dynamics._recorded_steps
    assert inspect.getsource(Metadynamics.run).index('_recorded_steps') < inspect.getsource(Metadynamics.run).index('_ensure_state')


def test_calculator_run_metad_validates_before_any_device_work():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype = torch.device('cpu'), torch.float32
    calc.model = _FakeModel()
    a, b = FakeAtoms([8, 1, 1, 1, 6], np.zeros((5, 3))), FakeAtoms([6, 1], np.zeros((2, 3)))
    args = (300.0, 0.02, 0.01, [0.3, 0.1], 5)
    with pytest.raises(ValueError, match='at least one'):
        calc.run_metad([], CVS, 10, *args)
    with pytest.raises(ValueError, match='sizes'):
        calc.run_metad([a, b], CVS, 10, *args)
    with pytest.raises(ValueError, match='cvs'):
        calc.run_metad(a, [('distance', 0, 5)], 10, *args)
    with pytest.raises(ValueError, match='hill_width'):
        calc.run_metad(a, CVS, 10, 300.0, 0.02, 0.01, [0.3, -0.1], 5)
    with pytest.raises(ValueError, match='bias_factor'):
        calc.run_metad(a, CVS, 10, *args, bias_factor=1.0)
    with pytest.raises(ValueError, match='walkers'):
        calc.run_metad(a, CVS, 10, *args, walkers=0)
    with pytest.raises(ValueError, match='friction'):
        calc.run_metad(a, CVS, 10, 300.0, 0.0, 0.01, [0.3, 0.1], 5)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match='pace'):
            calc.run_metad(a, CVS, 10, 300.0, 0.02, 0.01, [0.3, 0.1], bad)
        with pytest.raises(ValueError, match='n_steps'):
            calc.run_metad(a, CVS, bad, *args)
        with pytest.raises(ValueError, match='record_every'):
            calc.run_metad(a, CVS, 10, *args, record_every=bad)
    with pytest.raises(ValueError, match='timestep'):
        calc.run_metad(a, CVS, 10, *args, timestep=0.0)
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.run_metad(a, CVS, 10, *args)
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.run_metad([a, a], [CVS, CVS[:1]], 10, *args, walkers=4, restraint_k=1.0, restraint_center=np.zeros((2, 4, 2)))


def test_tables_are_formed_in_fp64_and_rounded_once():
    from newtonnet_amd.metadynamics import check_bias_arguments, check_cvs, hill_parameters
    table = check_cvs([[('torsion', 3, 2, 1, 0), ('distance', 0, 4)], [('angle', 2, 0, 1)]], [5, 3])
    assert table.dtype == np.int32 and table.shape == (2, 2, 5)
    assert table.tolist() == [[[3, 3, 2, 1, 0], [1, 0, 4, 0, 0]], [[2, 2, 0, 1, 0], [0, 0, 0, 0, 0]]]
    height, widths, pace, gamma, W, kappa, centre, cap = check_bias_arguments(2, 300.0, 0.02, 0.01, [0.3, 0.1], 5, 6.0, 3, [1.0, 2.0],
                                                                              np.arange(6).reshape(2, 3, 1), 16, 2)
    assert (height, pace, gamma, W, cap) == (0.01, 5, 6.0, 3, 16) and widths.tolist() == [0.3, 0.1]
    assert kappa.shape == centre.shape == (2, 3, 2) and kappa[1, 2].tolist() == [1.0, 2.0] and centre[1, 2].tolist() == [5.0, 5.0]
    par = hill_parameters([2, 1], widths, height, gamma, [300.0, 400.0])
    assert par.dtype == np.float32 and par.shape == (2, 4)
    assert par[0].tolist() == [np.float32(1.0 / 0.09), np.float32(1.0 / (0.1 * 0.1)), np.float32(0.01),
                               np.float32(1.0 / (br.K_BOLTZMANN * 5.0 * 300.0))]
    assert par[1, 1] == 0.0 and par[1, 3] == np.float32(1.0 / (br.K_BOLTZMANN * 5.0 * 400.0))
    assert hill_parameters([1], widths, height, None, [0.0])[0, 3] == 0.0


# ---- the reference's own mathematics ---------------------------------------------------------------------------------------------------

def _wrapped(d):
    return d - 2.0 * np.pi * np.rint(d / (2.0 * np.pi))


def _chain(rng, n=5):
    """a self-avoiding chain: bond 1.1 .. 1.5 A, random directions, no two consecutive bonds near collinear"""
    while True:
        x = np.cumsum(rng.normal(size=(n, 3)) * 0.8 + np.array([1.0, 0.0, 0.0]), axis=0)
        b = np.diff(x, axis=0)
        cos = [(b[i] @ b[i + 1]) / np.linalg.norm(b[i]) / np.linalg.norm(b[i + 1]) for i in range(n - 2)]
        if np.all(np.abs(cos) < 0.9):
            return x


def _value_and_rows(kind, idx, x):
    s, _, atoms, rows, degenerate = br.variable(kind, idx, x)
    assert not degenerate and atoms == list(idx)
    return float(s.v), np.array([[float(c.v) for c in r] for r in rows])


CASES = [(br.DISTANCE, (0, 3)), (br.ANGLE, (0, 2, 4)), (br.ANGLE, (1, 0, 2)), (br.TORSION, (0, 1, 2, 3)), (br.TORSION, (4, 2, 1, 0))]


@pytest.mark.parametrize('kind, idx', CASES)
def test_reference_gradients_are_central_differences_and_carry_no_net_force_or_torque(kind, idx):
    rng = np.random.default_rng(20261019 + kind)
    h = 1e-5
    for trial in range(20):
        x = _chain(rng)
        s, rows = _value_and_rows(kind, idx, x)
        scale = np.abs(rows).max()
        for r, a in enumerate(idx):
            for k in range(3):
                xp, xm = x.copy(), x.copy()
                xp[a, k] += h
                xm[a, k] -= h
                d = _value_and_rows(kind, idx, xp)[0] - _value_and_rows(kind, idx, xm)[0]
                fd = (_wrapped(d) if kind == br.TORSION else d) / (2.0 * h)
                assert abs(fd - rows[r, k]) <= 1e-7 * scale, (trial, a, k, fd, rows[r, k])
        assert np.abs(rows.sum(0)).max() <= 1e-12 * scale                                         # no net force
        torque = np.cross(x[list(idx)], rows).sum(0)
        assert np.abs(torque).max() <= 1e-12 * scale * np.abs(x).max()                            # no net torque


def test_reference_torsion_is_continuous_across_pi_through_the_wrapped_difference():
    """a planar trans chain twisted by +-1e-4: s jumps from +pi to -pi, the wrapped difference does not, and it is the gradient"""
    def twisted(phi):
        return np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.5], [np.cos(phi), np.sin(phi), 2.5]])
    eps = 1e-4
    sp, rows = _value_and_rows(br.TORSION, (0, 1, 2, 3), twisted(np.pi / 4 + np.pi))
    a = _value_and_rows(br.TORSION, (0, 1, 2, 3), twisted(np.pi / 4 + np.pi - eps))[0]
    b = _value_and_rows(br.TORSION, (0, 1, 2, 3), twisted(np.pi / 4 + np.pi + eps))[0]
    assert abs(abs(sp) - np.pi) < 1e-12 and a * b < 0 and abs(a - b) > 6.0
    assert abs(abs(_wrapped(b - a)) - 2 * eps) < 1e-9
    # the hill sum sees a centre at -pi + 0.01 from s = pi - 0.01 at the distance 0.02, not 2 pi - 0.02
    V, G0, _, amb = br.hill_sum([[-np.pi + 0.01, 0.0, 1.0, 0.0]], br.B(np.pi - 0.01), br.B(0.0), 1.0 / 0.01, 0.0, br.TWO_PI32, 0.0)
    d = (np.pi - 0.01) - (-np.pi + 0.01) - br.TWO_PI32
    assert amb == 0 and abs(float(V.v) - np.exp(-0.5 * d * d / 0.01)) < 1e-12 and abs(d + 0.02) < 1e-6


def _five_atom_case(rng, gamma=None):
    x = _chain(rng).astype(np.float32).astype(np.float64)
    cv_def = np.array([[br.TORSION, 0, 1, 2, 3], [br.DISTANCE, 3, 4, 0, 0]])                    # the two variables share atom 3
    s = [float(br.variable(int(d[0]), d[1:].tolist(), x)[0].v) for d in cv_def]
    rows = np.zeros((300, 4), dtype=np.float32)
    rows[:, 0] = _wrapped(s[0] + rng.normal(size=300) * 0.4)
    rows[:, 1] = s[1] + rng.normal(size=300) * 0.15
    rows[:, 2] = rng.uniform(0.002, 0.01, 300)
    par = np.array([1.0 / 0.35 ** 2, 1.0 / 0.12 ** 2, 0.01, 0.0 if gamma is None else 1.0 / (br.K_BOLTZMANN * (gamma - 1.0) * 300.0)],
                   dtype=np.float32)
    restraint = np.array([[0.8, s[0] + 0.3], [3.0, s[1] - 0.1]], dtype=np.float32)
    return x, cv_def, restraint, par, rows


def test_reference_bias_force_is_minus_the_central_difference_of_v_plus_u():
    rng = np.random.default_rng(7)
    x, cv_def, restraint, par, rows = _five_atom_case(rng)
    w = br.walker(x, np.zeros_like(x), cv_def, restraint, par, rows)
    assert w['status'] == 0 and w['ambiguous'] == 0 and w['bias'][0] > 0.05 and w['bias'][1] > 0.01
    assert w['touched'].all()
    h = 1e-5
    scale = np.abs(w['force']).max()
    for a in range(5):
        for k in range(3):
            xp, xm = x.copy(), x.copy()
            xp[a, k] += h
            xm[a, k] -= h
            fd = -(br.potential(xp, cv_def, restraint, par, rows) - br.potential(xm, cv_def, restraint, par, rows)) / (2.0 * h)
            assert abs(fd - w['force'][a, k]) <= 1e-7 * scale, (a, k, fd, w['force'][a, k])
    assert np.abs(w['force'].sum(0)).max() <= 1e-12 * scale
    # an atom in no variable keeps its force, bit for bit, and a molecule without variables is a copy
    f = rng.normal(size=(5, 3)).astype(np.float32).astype(np.float64)
    only = br.walker(x, f, np.array([[br.DISTANCE, 0, 1, 0, 0], [0, 0, 0, 0, 0]]), restraint, par, rows)
    assert np.array_equal(only['force'][2:], f[2:]) and not only['touched'][2:].any() and only['touched'][:2].all()
    none = br.walker(x, f, np.zeros((2, 5), dtype=int), restraint, par, rows[:0])
    assert np.array_equal(none['force'], f) and not none['bias'].any() and not none['bforce'].any()


def test_reference_deposits_have_the_well_tempered_height():
    rng = np.random.default_rng(9)
    for gamma in (None, 6.0):
        x, cv_def, restraint, par, rows = _five_atom_case(rng, gamma)
        xs = np.stack([x, x + rng.normal(size=x.shape) * 0.05]).astype(np.float32).astype(np.float64)
        hills = np.zeros((400, 4), dtype=np.float32)
        hills[:300] = rows
        walkers, new = br.group(xs, np.zeros_like(xs), np.stack([cv_def] * 2), np.stack([restraint] * 2), par, hills, 150, br.DEPOSIT)
        for j, w in enumerate(walkers):
            V = w['bias'][0]
            assert V > 0.01
            if gamma is None:
                assert new[j, 2] == float(par[2]) and w['bheight'] <= 2 * br.TINY32 + 12 * br.EPS32 * par[2]
            else:
                want = float(par[2]) * np.exp(-V / (br.K_BOLTZMANN * (gamma - 1.0) * 300.0))
                assert abs(new[j, 2] - want) <= 1e-6 * want and new[j, 2] < 0.9 * float(par[2])
            assert new[j, 0] == w['cv'][0] and new[j, 1] == w['cv'][1] and new[j, 3] == 0.0


def test_free_energy_applies_the_well_tempered_factor():
    from newtonnet_amd.metadynamics import free_energy_factor
    V = np.array([0.30, 0.10, 0.25])
    assert free_energy_factor(None) == -1.0 and free_energy_factor(5.0) == -1.25
    np.testing.assert_allclose(br.free_energy(V, None), [0.0, 0.20, 0.05], atol=1e-15)
    np.testing.assert_allclose(br.free_energy(V, 5.0), np.array([0.0, 0.20, 0.05]) * 1.25, atol=1e-15)
    np.testing.assert_allclose(br.free_energy(V, 5.0), free_energy_factor(5.0) * V - (free_energy_factor(5.0) * V).min(), atol=1e-15)
