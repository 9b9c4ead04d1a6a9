"""CPU-side checks of the batched dimer-method saddle search (newtonnet_amd/dimer.py, csrc/dimer.hip): the C ABI exports the kernel
and the header's constants are the Python ones, arguments are refused before any device work, the root form of the angles the
device uses equals the atan / sin / cos form, one rotation is exact on a quadratic, the host fp64 loop dimer_ref.search finds
saddles, the float32 emulation of the chain lies inside the fp64 bound, and the synthetic kernel inputs reach every branch at every
size without an ambiguous decision -- the condition that lets the device test demand every decision exactly."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import dimer_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the ABI and the constants ----------------------------------------------------------------------------------------------------

def test_kernel_symbol_is_declared_listed_and_exported():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    assert 'nnhip_dimer_step' in declared and 'nnhip_dimer_step' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'nnhip_dimer_step')
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bdimer\b.*\)', f.read(), re.M)
    assert callable(hip.dimer_step)


def test_header_constants_equal_the_python_ones():
    from newtonnet_amd import hip
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()

    def define(name):
        return int(re.search(rf'#define {name} (\S+)', header).group(1))
    assert define('NNHIP_DIMER_CHECK_ONLY') == hip.DIMER_CHECK_ONLY == dr.CHECK_ONLY == 1
    assert define('NNHIP_DIMER_N_INT') == hip.DIMER_N_INT == len(dr.INTS)
    assert define('NNHIP_DIMER_N_FLOAT') == hip.DIMER_N_FLOAT == len(dr.FLOATS)
    assert define('NNHIP_DIMER_N_VEC') == hip.DIMER_N_VEC == len(dr.VECS)
    # the rows of the state blocks, in the order the reference names them
    names = dict(n_steps='steps', n_evals='evals', n_rot='rot', n_rot_total='rot_total', n_pairs='pairs', d_norm='dnorm')
    for k, name in enumerate(dr.INTS):
        assert hip.DIMER_I[names.get(name, name)] == k == define('NNHIP_DIMER_I_' + names.get(name, name).upper())
    for k, name in enumerate(dr.FLOATS):
        assert hip.DIMER_F[names.get(name, name)] == k == define('NNHIP_DIMER_F_' + names.get(name, name).upper())
    for k, name in enumerate(dr.VECS):
        assert hip.DIMER_V[name.lower()] == k == define('NNHIP_DIMER_V_' + name.upper())
    assert dr.SYN_MEMORY <= hip.LBFGS_MAX_MEMORY


def test_the_lbfgs_recursion_has_one_text():
    """relax.hip and dimer.hip include the device code of pair acceptance, two-loop and clamp; neither restates it"""
    src = os.path.join(ROOT, 'newtonnet_amd', 'csrc')
    chain = open(os.path.join(src, 'lbfgs_chain.h')).read()
    assert 'NNHIP_LBFGS_CURVATURE_MIN' in chain and 'two_loop_and_step' in chain
    for name in ('relax.hip', 'dimer.hip'):
        text = open(os.path.join(src, name)).read()
        assert '#include "lbfgs_chain.h"' in text and 'lbfgs_chain::step(' in text
        assert 'NNHIP_LBFGS_CURVATURE_MIN' not in re.sub(r'//[^\n]*', '', text)


# ---- 2. refusals before any device work ----------------------------------------------------------------------------------------------

class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force']


def _inputs(n=3, b=1):
    return (torch.ones(n, dtype=torch.long), torch.zeros(n, 3), torch.zeros(b, 3, 3), torch.zeros(n, dtype=torch.long))


def test_saddle_search_validates_before_any_device_work():
    from newtonnet_amd.dimer import SaddleSearch, check_arguments, check_run_arguments
    from newtonnet_amd.models.newtonnet import NewtonNet
    assert callable(NewtonNet.saddle_search)
    z, pos, cell, batch = _inputs()
    train = _FakeModel()
    train.training = True
    with pytest.raises(ValueError, match='eval'):
        SaddleSearch(train, z, pos, cell, batch)
    for props in (['energy'], ['gradient_force']):
        one_head = _FakeModel()
        one_head.output_properties = props
        with pytest.raises(ValueError, match='heads'):
            SaddleSearch(one_head, z, pos, cell, batch)
    ok = _FakeModel()
    with pytest.raises(ValueError, match='pos'):
        SaddleSearch(ok, z, torch.zeros(3, 2), cell, batch)
    with pytest.raises(ValueError, match='cell'):
        SaddleSearch(ok, z, pos, torch.zeros(3, 3), batch)
    with pytest.raises(ValueError, match='batch'):
        SaddleSearch(ok, z, pos, cell, batch[:2])
    with pytest.raises(ValueError, match='float32'):
        SaddleSearch(ok, z, pos.double(), cell, batch)
    with pytest.raises(ValueError, match='fixed'):
        SaddleSearch(ok, z, pos, cell, batch, fixed=torch.zeros(3))
    with pytest.raises(ValueError, match='direction'):
        SaddleSearch(ok, z, pos, cell, batch, direction=torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match='direction'):
        SaddleSearch(ok, z, pos, cell, batch, direction=torch.zeros(2, 3))
    one = torch.ones(3, 3)
    for name in ('fmax', 'dimer_length', 'maxstep', 'alpha'):
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match=name):
                SaddleSearch(ok, z, pos, cell, batch, direction=one, **{name: bad})
    for bad in (0.0, -5.0, 45.0, 90.0, float('nan')):
        with pytest.raises(ValueError, match='rotation_tolerance'):
            SaddleSearch(ok, z, pos, cell, batch, direction=one, rotation_tolerance=bad)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match='max_rotations'):
            SaddleSearch(ok, z, pos, cell, batch, direction=one, max_rotations=bad)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match='memory'):
            SaddleSearch(ok, z, pos, cell, batch, direction=one, memory=bad)
    with pytest.raises(ValueError, match='solver'):
        SaddleSearch(ok, z, pos, cell, batch, solver='no such solver')
    with pytest.raises(RuntimeError, match='MI355X'):                                     # CPU tensors: no CPU path
        SaddleSearch(ok, z, pos, cell, batch, direction=one)
    assert check_arguments(0.001, 0.01, 5.0, 8, 16, 0.2, 70.0) == (0.001, 0.01, 5.0, 8, 16, 0.2, 70.0)
    for name in ('max_evaluations', 'check_every', 'record_every'):
        for bad in (-1, 2.5):
            with pytest.raises(ValueError, match=name):
                check_run_arguments(**{**dict(max_evaluations=1, check_every=1, record_every=0), name: bad})


def test_calculator_find_saddle_validates_before_any_device_work():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype = torch.device('cpu'), torch.float32
    calc.model = _FakeModel()
    a, b = FakeAtoms([8, 1, 1], np.zeros((3, 3))), FakeAtoms([6, 1], np.zeros((2, 3)))
    with pytest.raises(ValueError, match='at least one'):
        calc.find_saddle([])
    with pytest.raises(ValueError, match='sizes'):
        calc.find_saddle([a, b])
    with pytest.raises(ValueError, match='fmax'):
        calc.find_saddle(a, fmax=-0.01)
    with pytest.raises(ValueError, match='dimer_length'):
        calc.find_saddle(a, dimer_length=0.0)
    with pytest.raises(ValueError, match='rotation_tolerance'):
        calc.find_saddle(a, rotation_tolerance=60.0)
    with pytest.raises(ValueError, match='max_evaluations'):
        calc.find_saddle(a, max_evaluations=-1)
    with pytest.raises(ValueError, match='check_every'):
        calc.find_saddle(a, check_every=2.5)
    with pytest.raises(ValueError, match='solver'):
        calc.find_saddle(a, solver='no such solver')
    with pytest.raises(ValueError, match='fixed'):
        calc.find_saddle(a, fixed=np.zeros(2, dtype=bool))
    with pytest.raises(ValueError, match='direction'):
        calc.find_saddle([a, a], direction=np.ones((3, 3)))
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.find_saddle(a, direction=np.ones((3, 3)))


# ---- 3. the angles: roots against atan / sin / cos -------------------------------------------------------------------------------------

def test_root_form_of_the_angles_equals_the_atan_form():
    worst = 0.0
    for r in np.exp(np.linspace(math.log(1e-6), math.log(1e6), 241)):
        worst = max(worst, max(abs(p - q) for p, q in zip(dr.trial_angle_roots(r), dr.trial_angle_atan(r))))
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                a1, b1 = sa * 0.7, sb * 0.7 * r
                scale = 1.0 / math.hypot(a1, b1)
                got, want = dr.min_angle_roots(a1 * scale, b1 * scale), dr.min_angle_atan(a1 * scale, b1 * scale)
                # cos phi = 0 is the one point where the two forms may name the same axis by opposite signs
                flip = -1.0 if got[0] < 1e-9 and got[1] * want[1] < 0 else 1.0
                worst = max(worst, abs(got[0] - flip * want[0]), abs(got[1] - flip * want[1]))
                # and it is the minimum of the fitted curve: the value there is -sqrt(a1^2 + b1^2)
                c2, s2 = got[0] ** 2 - got[1] ** 2, 2 * got[0] * got[1]
                worst = max(worst, abs(a1 * scale * c2 + b1 * scale * s2 + 1.0))
    print(f'largest difference between the two forms: {worst:.2e}')
    assert worst < 1e-12
    assert dr.min_angle_roots(0.0, 0.0) == (1.0, 0.0)


# ---- 4. one rotation on an exact quadratic ------------------------------------------------------------------------------------------------

def _quadratic(seed=7, d=9):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = np.concatenate([[-0.8], rng.uniform(0.5, 8.0, d - 1)])
    return (Q * lam) @ Q.T, rng.uniform(-1, 1, d), Q[:, 0]


def test_one_trial_rotation_is_exact_on_a_quadratic():
    """phi_m minimises N(phi).H.N(phi) in the (N, Theta) plane, and the interpolated F1 is the force at the rotated endpoint"""
    H, xs, _ = _quadratic()
    n, delta = 3, 0.01
    rng = np.random.default_rng(11)

    def forces(x):
        return -(H @ (x.reshape(-1) - xs)).reshape(n, 3)
    x0 = (xs + rng.normal(0, 0.3, 9)).reshape(n, 3)
    u = rng.standard_normal((n, 3))
    st = dr.new_state(n, 4, x0, u / np.linalg.norm(u))
    par = dr.params(dimer_length=delta, rotation_tolerance=1e-3, fp32=False)
    probe = x0
    for _ in range(3):                                       # centre, endpoint, trial endpoint
        r = dr.dimer_step(probe, forces(probe), None, st, par, eps=0.0)
        before, st, probe = st, r['state'], r['x_out']
    assert r['path'].startswith('p2') and st['n_rot_total'] == 1
    N0, Th = before['mode'].reshape(-1), before['theta'].reshape(-1)
    assert abs(N0 @ Th) < 1e-12 and abs(Th @ Th - 1) < 1e-12
    a, b, c = N0 @ H @ N0, N0 @ H @ Th, Th @ H @ Th         # N(phi).H.N(phi) = a cos^2 + 2 b sin cos + c sin^2
    phi = 0.5 * math.atan2(2 * b, a - c)
    cands = [phi, phi + 0.5 * math.pi]
    best = min(cands, key=lambda p: a * math.cos(p) ** 2 + 2 * b * math.sin(p) * math.cos(p) + c * math.sin(p) ** 2)
    cp, sp = r['phi']
    want = np.array([math.cos(best), math.sin(best)])
    want = -want if want[0] < 0 else want
    assert abs(cp - want[0]) < 1e-10 and abs(sp - want[1]) < 1e-10
    N1 = st['mode'].reshape(-1)
    assert np.abs(N1 - (cp * N0 + sp * Th)).max() < 1e-12
    true_f1 = forces(st['center'] + delta * st['mode'])
    assert np.abs(st['F1'] - true_f1).max() < 1e-10
    assert abs(st['curvature'] - N1 @ H @ N1) < 1e-10


def test_search_finds_the_saddle_and_the_lowest_mode_of_a_quadratic():
    H, xs, v0 = _quadratic()
    rng = np.random.default_rng(3)

    def energy_forces(x):
        d = x.reshape(-1) - xs
        return 0.5 * d @ H @ d, -(H @ d).reshape(3, 3)
    x0 = (xs + rng.normal(0, 0.2, 9)).reshape(3, 3)
    r = dr.search(energy_forces, x0, rng.standard_normal((3, 3)), fmax=1e-6, alpha=8.0, max_evaluations=400)
    print(f"quadratic: {r['n_evaluations']} evaluations, {r['n_steps']} translations, {r['n_rotations']} rotations, curvature "
          f"{r['curvature']:.6f}")
    assert r['converged'] and r['fmax'] < 1e-6
    assert np.abs(r['x'].reshape(-1) - xs).max() < 1e-5
    # the mode is as good as the rotations' own stopping rule: a cycle ends when the predicted rotation falls below 5 degrees, so
    # the mode lies within that angle t of the eigenvector, and N.H.N within (lambda_max - lambda_min) sin^2 t above lambda_min
    overlap = abs(r['mode'].reshape(-1) @ v0)
    lam = np.linalg.eigvalsh(H)
    print(f'overlap with the lowest eigenvector {overlap:.6f}')
    assert overlap > math.cos(math.radians(5.0))
    assert lam[0] - 1e-9 <= r['curvature'] <= lam[0] + (lam[-1] - lam[0]) * math.sin(math.radians(5.0)) ** 2


def test_search_finds_the_mueller_brown_saddle():
    from tests.test_neb_host import MB_SADDLE, _mb_energy_forces, _mb_hessian, _mb_stationary
    saddle = _mb_stationary(MB_SADDLE)
    rng = np.random.default_rng(5)

    def energy_forces(x):
        E, F = _mb_energy_forces(x[None])
        return E[0], F[0]
    off = rng.standard_normal(3)
    x0 = np.concatenate([saddle, [0.0]])[None] + 0.1 * off / np.linalg.norm(off)
    r = dr.search(energy_forces, x0, rng.standard_normal((1, 3)), fmax=5e-4, alpha=4.0, max_evaluations=400)
    print(f"Mueller-Brown: {r['n_evaluations']} evaluations, {r['n_steps']} translations, {r['n_rotations']} rotations, curvature "
          f"{r['curvature']:.4f}, |x - saddle| {np.abs(r['x'][0, :2] - saddle).max():.2e}")
    assert r['converged'] and r['curvature'] < 0
    assert np.abs(r['x'][0, :2] - saddle).max() < 1e-3 and abs(r['x'][0, 2]) < 1e-3
    lam, V = np.linalg.eigh(_mb_hessian(saddle))
    assert abs(abs(r['mode'][0, :2] @ V[:, 0]) - 1.0) < 1e-2


# ---- 5. the reference: emulation inside the bound, synthetic inputs that reach every branch -----------------------------------------------

@pytest.fixture(scope='module')
def emulation():
    return dr.main()


def test_float32_emulation_stays_inside_the_bound(emulation):
    worst, total, _ = emulation
    assert total >= len(dr.SYN_SIZES) * 12
    assert set(worst) == set(dr.GROUPS)
    assert max(worst.values()) < 1.0


def test_bound_is_first_order_in_eps():
    c = next(c for c in dr.synthetic_cases(False) if c['n'] == 21 and c['path'].startswith('p2') and c['path'].endswith('trial'))
    full, half, none = (dr.dimer_step(c['x'], c['F'], None, c['st'], dr.SYN_PAR, eps=e) for e in (dr.EPS32, 0.5 * dr.EPS32, 0.0))
    assert not none['bx'].any() and all(not np.any(b) for b in none['bounds'].values())
    moved = full['bx'] > 0
    assert moved.any() and np.allclose(half['bx'][moved], 0.5 * full['bx'][moved], rtol=1e-5)
    for k in ('F1', 'mode', 'theta'):
        m = full['bounds'][k] > 0
        assert m.any() and np.allclose(half['bounds'][k][m], 0.5 * full['bounds'][k][m], rtol=1e-5)
    assert np.array_equal(full['x_out'], none['x_out'])


@pytest.mark.parametrize('masked', (False, True))
def test_synthetic_inputs_reach_every_branch_at_every_size_without_an_ambiguous_decision(masked, emulation):
    assert emulation[2] == 0                               # the GPU test may demand every decision
    cases = dr.synthetic_cases(masked)
    for n in dr.SYN_SIZES:
        earned = set()
        for c in (c for c in cases if c['n'] == n):
            ref = dr.dimer_step(c['x'], c['F'], c['free'] if masked else None, c['st'], dr.SYN_PAR)
            assert not ref['bad'] and not any(ref['ambiguous'].values())
            earned |= dr._labels(ref, c['st'])
            if masked:
                assert np.isnan(c['F'][~c['free']]).all()  # a fixed atom's force row holds NaN
            # a check-only launch freezes the molecule and touches nothing
            chk = dr.dimer_step(c['x'], c['F'], c['free'] if masked else None, c['st'], dr.SYN_PAR, dr.CHECK_ONLY)
            assert chk['frozen'] and np.array_equal(chk['x_out'], c['x'].astype(np.float64))
            assert all(np.array_equal(np.asarray(chk['state'][k]), np.asarray(c['st'][k])) for k in c['st'])
        assert earned == set(dr.SYN_WANTED), f'size {n}: {sorted(set(dr.SYN_WANTED) - earned)} not reached'
    d = dr.synthetic_batch(masked)
    assert [0 if c is None else c['n'] for c in d['cases']].count(0) == 3 and d['ptr'][-1] == d['x'].shape[0]
    if masked:
        assert not d['free'].all()
