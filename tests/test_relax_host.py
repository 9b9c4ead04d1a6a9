"""CPU-side checks of the batched geometry relaxation (newtonnet_amd/relax.py, csrc/relax.hip): the C ABI exports the kernel and
the header's constants are the Python ones, arguments are refused before any device work, and the fp64 restatement the GPU tests
compare against (tests/relax_ref.py) is L-BFGS -- its two-loop recursion is the product with the dense BFGS inverse Hessian, it
minimises a quadratic -- with a bound that contains a float32 emulation of the chain and is first order in eps.  The synthetic
inputs of the GPU kernel test are checked HERE to contain no ambiguous decision, so that test can demand every case."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import relax_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def syn():
    return rr.synthetic_batch()


def test_kernel_symbol_is_declared_listed_and_exported():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    assert 'nnhip_lbfgs_step' in declared and 'nnhip_lbfgs_step' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'nnhip_lbfgs_step')
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\brelax\b.*\)', f.read(), re.M)


def test_header_constants_equal_the_python_ones():
    from newtonnet_amd import hip
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()

    def define(name):
        return re.search(rf'#define {name} (\S+)', header).group(1)
    assert int(define('NNHIP_LBFGS_CHECK_ONLY')) == hip.LBFGS_CHECK_ONLY == rr.CHECK_ONLY == 1
    assert int(define('NNHIP_LBFGS_MAX_MEMORY')) == hip.LBFGS_MAX_MEMORY == rr.MAX_MEMORY
    assert define('NNHIP_LBFGS_CURVATURE_MIN') == '1e-4f' and hip.LBFGS_CURVATURE_MIN == rr.CURVATURE_MIN == 1e-4
    assert rr.CURVATURE_MIN2 == float(np.float32(np.float32(1e-4) * np.float32(1e-4)))


class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force']


def _inputs(n=3, b=1):
    return (torch.ones(n, dtype=torch.long), torch.zeros(n, 3), torch.zeros(b, 3, 3), torch.zeros(n, dtype=torch.long))


def test_relaxation_validates_before_any_device_work():
    from newtonnet_amd.relax import Relaxation, check_run_arguments
    z, pos, cell, batch = _inputs()
    train = _FakeModel()
    train.training = True
    with pytest.raises(ValueError, match='eval'):
        Relaxation(train, z, pos, cell, batch)
    energy_only = _FakeModel()
    energy_only.output_properties = ['energy']
    with pytest.raises(ValueError, match='gradient_force'):
        Relaxation(energy_only, z, pos, cell, batch)
    ok = _FakeModel()
    with pytest.raises(ValueError, match='pos'):
        Relaxation(ok, z, torch.zeros(3, 2), cell, batch)
    with pytest.raises(ValueError, match='cell'):
        Relaxation(ok, z, pos, torch.zeros(3, 3), batch)
    with pytest.raises(ValueError, match='batch'):
        Relaxation(ok, z, pos, cell, batch[:2])
    with pytest.raises(ValueError, match='float32'):
        Relaxation(ok, z, pos.double(), cell, batch)
    with pytest.raises(ValueError, match='fixed'):
        Relaxation(ok, z, pos, cell, batch, fixed=torch.zeros(3))
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='fmax'):
            Relaxation(ok, z, pos, cell, batch, fmax=bad)
        with pytest.raises(ValueError, match='maxstep'):
            Relaxation(ok, z, pos, cell, batch, maxstep=bad)
        with pytest.raises(ValueError, match='alpha'):
            Relaxation(ok, z, pos, cell, batch, alpha=bad)
    for bad in (0, -3, 65, 2.5):
        with pytest.raises(ValueError, match='memory'):
            Relaxation(ok, z, pos, cell, batch, memory=bad)
    with pytest.raises(RuntimeError, match='MI355X'):                                     # CPU tensors: no CPU path
        Relaxation(ok, z, pos, cell, batch)
    for bad in ((-1, 10, 0), (2.5, 10, 0), (5, -1, 0), (5, 10, -2), (5, 1.5, 0)):
        with pytest.raises(ValueError):
            check_run_arguments(*bad)
    assert check_run_arguments(5, 0, 0) == (5, 0, 0)


def test_calculator_relax_validates_before_any_device_work():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype = torch.device('cpu'), torch.float32
    calc.model = _FakeModel()
    a, b = FakeAtoms([8, 1, 1], np.zeros((3, 3))), FakeAtoms([6, 1], np.zeros((2, 3)))
    with pytest.raises(ValueError, match='at least one'):
        calc.relax([])
    with pytest.raises(ValueError, match='sizes'):
        calc.relax([a, b])
    with pytest.raises(ValueError, match='fmax'):
        calc.relax(a, fmax=-0.01)
    with pytest.raises(ValueError, match='max_steps'):
        calc.relax(a, max_steps=-1)
    with pytest.raises(ValueError, match='max_steps'):
        calc.relax(a, max_steps=2.5)
    with pytest.raises(ValueError, match='memory'):
        calc.relax(a, memory=0)
    with pytest.raises(ValueError, match='maxstep'):
        calc.relax(a, maxstep=0.0)
    with pytest.raises(ValueError, match='alpha'):
        calc.relax(a, alpha=-70.0)
    with pytest.raises(ValueError, match='check_every'):
        calc.relax(a, check_every=-1)
    with pytest.raises(ValueError, match='fixed'):
        calc.relax(a, fixed=[True, False])
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.relax(a)


# ---- the reference is L-BFGS ---------------------------------------------------------------------------------------------------------

def _quadratic(n=7, seed=1):
    # (eigenvalues 10 .. 140 eV/A^2 around alpha = 70: without a line search the method needs H0 = 1 / alpha not to overshoot the
    # stiffest direction by more than a factor 2, here as in ASE)
    rng = np.random.default_rng(seed)
    A = rr._spd(rng, 3 * n, 10.0, 140.0)
    x_min = rng.uniform(-2, 2, 3 * n)
    return A, x_min


def test_two_loop_equals_the_dense_bfgs_inverse_hessian():
    """m pairs y = A s in a wrapped ring: the step of the reference (no clamp) is -H f with H from the BFGS recursion
    H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T applied oldest pair first to H0 = I / alpha"""
    n, m, alpha = 7, 5, 70.0
    A, _ = _quadratic(n)
    rng = np.random.default_rng(2)
    for n_pairs, head in ((0, 0), (1, 1), (3, 1), (5, 2), (5, 0)):
        st = rr.new_state(n, m)
        st.update(n_steps=0, n_pairs=n_pairs, head=head)          # n_steps = 0: no pending pair, the two-loop alone
        H = np.eye(3 * n) / alpha
        for k in reversed(rr.pair_slots(head, n_pairs, m)):        # oldest first
            s = rng.normal(0, 0.05, 3 * n)
            y = A @ s
            rho = 1.0 / (y @ s)
            st['S'][k], st['Y'][k], st['rho'][k] = s.reshape(n, 3), y.reshape(n, 3), rho
            V = np.eye(3 * n) - rho * np.outer(y, s)
            H = V.T @ H @ V + rho * np.outer(s, s)
        f = rng.normal(0, 0.01, (n, 3))
        x = rng.uniform(-1, 1, (n, 3))
        r = rr.lbfgs_step(x, f, None, st, 1e-12, alpha, 1e9, eps=0.0)
        assert not r['frozen'] and not r['clamped']
        np.testing.assert_allclose(r['x_out'] - x, (H @ f.reshape(-1)).reshape(n, 3), rtol=1e-9, atol=1e-14)
        # the secant condition of the newest pair: H y = s
        if n_pairs:
            k = rr.pair_slots(head, n_pairs, m)[0]
            np.testing.assert_allclose(H @ st['Y'][k].reshape(-1), st['S'][k].reshape(-1), rtol=1e-8, atol=1e-14)


def test_reference_minimises_a_quadratic_and_honours_clamp_freeze_and_fixed_atoms():
    n = 7
    A, x_min = _quadratic(n)
    free = np.ones(n, dtype=bool)
    free[2] = False
    x0 = x_min.reshape(n, 3) + np.random.default_rng(3).normal(0, 0.3, (n, 3))

    def ef(x):
        d = x.reshape(-1) - x_min
        return np.array([0.5 * d @ A @ d]), -(A @ d).reshape(n, 3)
    out = rr.minimise(ef, x0, [0, n], fmax=1e-3, memory=16, max_steps=300)
    assert out['converged'][0] and out['fmax'][0] < 1e-3 and out['n_steps'][0] < 60
    assert out['energy'][0] < 1e-8 * out['energy0'][0]
    held = rr.minimise(ef, x0, [0, n], fmax=1e-3, memory=16, max_steps=300, free=free)
    assert held['converged'][0] and np.array_equal(held['x'][2], x0[2]) and not np.array_equal(held['x'][3], x0[3])
    assert np.abs(rr.masked(ef(held['x'])[1], free)).max() < 1e-3
    # one step: the first is steepest descent with H0 = 1 / alpha, clamped to maxstep
    st = rr.new_state(n, 4)
    f = ef(x0)[1]
    r = rr.lbfgs_step(x0, f, None, st, 1e-6, 70.0, 0.2, eps=0.0)
    longest = np.sqrt(((f / 70.0) ** 2).sum(1).max())
    assert r['clamped'] == (longest >= 0.2) and r['clamped']
    np.testing.assert_allclose(r['x_out'] - x0, f / 70.0 * (0.2 / longest), rtol=1e-12)
    np.testing.assert_allclose(np.sqrt(((r['x_out'] - x0) ** 2).sum(1).max()), 0.2, rtol=1e-12)
    assert r['state']['n_steps'] == 1 and r['state']['n_pairs'] == 0 and np.array_equal(r['state']['f_prev'], f)
    # check-only and converged molecules move nothing and keep their state; only a small force sets the flag
    c = rr.lbfgs_step(x0, f, None, st, 1e-6, 70.0, 0.2, flags=rr.CHECK_ONLY)
    assert c['frozen'] and np.array_equal(c['x_out'], x0) and not c['state']['converged'] and c['state']['n_steps'] == 0
    c = rr.lbfgs_step(x0, f * 1e-9, None, st, 1e-6, 70.0, 0.2, flags=rr.CHECK_ONLY)
    assert c['frozen'] and c['state']['converged']
    done = dict(st, converged=True)
    c = rr.lbfgs_step(x0, f, None, done, 1e-6, 70.0, 0.2)
    assert c['frozen'] and np.array_equal(c['x_out'], x0) and c['state']['n_steps'] == 0
    # a rejected pair leaves the slot to be reused; in a full ring it costs the oldest pair
    m = 3
    st = rr.new_state(n, m)
    st.update(n_steps=5, n_pairs=m, head=1, f_prev=f - 1.0)            # y = f_prev - f = -1 everywhere
    st['S'][1] = 0.01                                                  # s = +0.01 everywhere: y.s < 0
    st['rho'][:] = 1.0
    r = rr.lbfgs_step(x0, f, None, st, 1e-6, 70.0, 0.2, eps=0.0)
    assert r['accepted'] is False and r['state']['head'] == 1 and r['state']['n_pairs'] == m - 1
    assert np.array_equal(r['state']['Y'], st['Y']) and np.array_equal(r['state']['rho'], st['rho'])


# ---- the bound ------------------------------------------------------------------------------------------------------------------------

def test_float32_emulation_stays_inside_the_bound_and_the_bound_scales_with_eps(syn):
    B = len(syn['kinds'])
    worst = 0.0
    moved = 0
    for b in range(B):
        a0, a1 = int(syn['ptr'][b]), int(syn['ptr'][b + 1])
        ref = rr.batch_step(syn, b)
        x32, fmax32, st32 = rr.emulate_step(syn['x'][a0:a1], syn['F'][a0:a1], syn['free'][a0:a1], rr.batch_state(syn, b), syn['tol2'],
                                            syn['alpha'], syn['maxstep'])
        new = ref['state']
        for k in ('converged', 'n_steps', 'n_pairs', 'head'):
            assert st32[k] == new[k], (b, syn['kinds'][b], k)
        assert abs(float(fmax32) - ref['fmax']) <= ref['b_fmax'] + rr.half_ulp32(ref['fmax'])
        err = np.abs(x32.astype(np.float64) - ref['x_out'])
        bound = ref['bx'] + rr.half_ulp32(ref['x_out'])
        assert np.all(err <= bound), (b, syn['kinds'][b], float((err / bound).max()))
        if ref['frozen']:
            assert np.array_equal(x32, syn['x'][a0:a1])
            continue
        if a1 > a0:
            worst = max(worst, float((err / bound).max()))
        moved += 1
        assert np.array_equal(x32[~syn['free'][a0:a1]], syn['x'][a0:a1][~syn['free'][a0:a1]])
        if ref['accepted']:
            h = rr.batch_state(syn, b)['head']
            assert abs(st32['rho'][h] - new['rho'][h]) <= ref['b_rho_new'] + rr.half_ulp32(new['rho'][h])
            assert np.array_equal(st32['Y'][h], new['Y'][h])
        # first order in eps: twice the eps, twice the bound (TINY32 aside); no eps, no bound
        two = rr.batch_step(syn, b, eps=2.0 * rr.EPS32)
        np.testing.assert_allclose(two['bx'] - rr.TINY32 * (two['bx'] > 0), 2.0 * (ref['bx'] - rr.TINY32 * (ref['bx'] > 0)), rtol=1e-9)
        zero = rr.batch_step(syn, b, eps=0.0)
        assert np.all(zero['bx'] <= rr.TINY32) and np.array_equal(zero['x_out'], ref['x_out'])
        # and not vacuous: a free atom's bound is at least its last rounding and stays below 1 % of the molecule's longest step
        # (the largest: one atom with four pairs in its three dimensions, 0.2 %)
        fr = syn['free'][a0:a1]
        assert np.all(ref['bx'][fr] >= rr.C_RX * rr.EPS32 * np.abs(ref['x_out'][fr]))
        assert ref['bx'].max() <= 1e-2 * np.abs(ref['x_out'] - syn['x'][a0:a1]).max() + 16 * rr.EPS32 * 8.0
    assert moved > 50
    print(f'float32 emulation over {moved} moving molecules: worst err / bound {worst:.3f} (C_RX = {rr.C_RX})')
    assert worst <= 0.75


def test_synthetic_kernel_inputs_cover_every_branch_without_an_ambiguous_decision(syn):
    seen = set()
    sizes = set()
    for b, kind in enumerate(syn['kinds']):
        n = int(syn['ptr'][b + 1] - syn['ptr'][b])
        for flags in (0, rr.CHECK_ONLY):
            r = rr.batch_step(syn, b, flags)
            assert not any(r['ambiguous'].values()), (b, kind, flags, r['ambiguous'])
        r = rr.batch_step(syn, b)
        st = rr.batch_state(syn, b)
        fixed = bool((~syn['free'][syn['ptr'][b]:syn['ptr'][b + 1]]).any())
        seen.add((kind, r['frozen'], r['accepted'], r['clamped']))
        seen.add(('pairs', st['n_pairs']))
        seen.add(('fixed', fixed, r['frozen']))
        if r['accepted'] and r['state']['head'] < st['head']:
            seen.add('accepted pair wraps the head')
        if st['n_pairs'] and st['head'] - st['n_pairs'] < 0 and not r['frozen']:
            seen.add('stored pairs wrap the ring')
        sizes.add(n)
        assert {'accept': r['accepted'] is True, 'reject_neg': r['accepted'] is False, 'reject_cos': r['accepted'] is False,
                'first': r['accepted'] is None and not r['frozen'], 'converged': r['frozen'] and st['converged'],
                'converging': r['frozen'] and r['state']['converged'] and not st['converged'],
                'empty': r['frozen'] and r['state']['converged']}[kind], (b, kind)
    assert sizes == {0, 1, 2, 21, 63, 64, 65, 200}
    m = rr.SYN_MEMORY
    for want in ([('accept', False, True, c) for c in (False, True)] + [('first', False, None, c) for c in (False, True)]
                 + [(k, False, False, c) for k in ('reject_neg', 'reject_cos') for c in (False, True)]
                 + [('converged', True, None, False), ('converging', True, None, False), ('empty', True, None, False)]
                 + [('pairs', p) for p in (0, 1, m - 1, m)] + [('fixed', True, False), ('fixed', False, False), ('fixed', True, True)]
                 + ['accepted pair wraps the head', 'stored pairs wrap the ring']):
        assert want in seen, want
