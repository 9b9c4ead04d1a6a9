"""CPU-side checks of the batched nudged elastic band (newtonnet_amd/neb.py, csrc/neb.hip): the C ABI exports the kernel and the
header's constants are the Python ones, arguments are refused before any device work, and the fp64 restatement the GPU tests
compare against (tests/neb_ref.py) is a climbing-image NEB -- on the Mueller-Brown surface its climbing image ends at the known
saddle and its force has neither a perpendicular spring part nor a parallel true part -- with a bound that contains a float32
emulation of the chain and is first order in eps.  The synthetic inputs of the GPU kernel test are checked HERE to reach every
branch without an ambiguous decision, so that test can demand every case."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import neb_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_SETS = (0, nr.CLIMB, nr.CLIMB | nr.CHECK_ONLY)


@pytest.fixture(scope='module')
def syn():
    return nr.synthetic_bands()


def test_kernel_symbol_is_declared_listed_and_exported_and_the_constants_agree():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    assert 'nnhip_neb_step' in declared and 'nnhip_neb_step' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'nnhip_neb_step')
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bneb\b.*\)', f.read(), re.M)

    def define(name):
        return int(re.search(rf'#define {name} (\S+)', header).group(1))
    assert define('NNHIP_NEB_CHECK_ONLY') == hip.NEB_CHECK_ONLY == nr.CHECK_ONLY == 1
    assert define('NNHIP_NEB_CLIMB') == hip.NEB_CLIMB == nr.CLIMB == 2
    assert define('NNHIP_NEB_MAX_IMAGES') == hip.NEB_MAX_IMAGES == nr.MAX_IMAGES >= 64
    # ASE's FIRE constants, in the order the launch takes them, as the fp32 values the reference uses
    dt, dt_max, n_min, f_inc, f_dec, a_start, f_a, maxstep = hip.NEB_FIRE_DEFAULTS
    assert (dt, dt_max, n_min, f_inc, f_dec, a_start, f_a, maxstep) == (0.1, 1.0, 5, 1.1, 0.5, 0.1, 0.99, 0.2)
    for k, v in dict(dt=dt, dt_max=dt_max, f_inc=f_inc, f_dec=f_dec, a_start=a_start, f_a=f_a, maxstep=maxstep).items():
        assert nr.FIRE[k] == float(np.float32(v)), k
    assert nr.FIRE['n_min'] == n_min


class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force']

    def band(self, *a, **kw):
        from newtonnet_amd.models import NewtonNet
        return NewtonNet.band(self, *a, **kw)


def _inputs(n=3, b=3):
    return (torch.ones(n * b, dtype=torch.long), torch.zeros(n * b, 3), torch.zeros(b, 3, 3),
            torch.arange(b).repeat_interleave(n))


def test_band_validates_before_any_device_work():
    from newtonnet_amd.neb import Band, band_counts, interpolate
    from newtonnet_amd.relax import check_run_arguments
    z, pos, cell, batch = _inputs()
    ok = _FakeModel()
    train = _FakeModel()
    train.training = True
    with pytest.raises(ValueError, match='eval'):
        train.band(z, pos, cell, batch, 3)
    energy_only = _FakeModel()
    energy_only.output_properties = ['energy']
    with pytest.raises(ValueError, match='gradient_force'):
        energy_only.band(z, pos, cell, batch, 3)
    with pytest.raises(ValueError, match='pos'):
        ok.band(z, torch.zeros(9, 2), cell, batch, 3)
    with pytest.raises(ValueError, match='cell'):
        ok.band(z, pos, torch.zeros(3, 3), batch, 3)
    with pytest.raises(ValueError, match='batch'):
        ok.band(z, pos, cell, batch[:2], 3)
    with pytest.raises(ValueError, match='float32'):
        ok.band(z, pos.double(), cell, batch, 3)
    with pytest.raises(ValueError, match='fixed'):
        ok.band(z, pos, cell, batch, 3, fixed=torch.zeros(9))
    for bad in (2, 4, 0, -3, 2.5, [2, 1], [3, 3], [3.5], 'x', None, True):
        with pytest.raises(ValueError, match='n_images'):
            ok.band(z, pos, cell, batch, bad)
    z70, pos70, cell70, batch70 = _inputs(1, 70)
    with pytest.raises(ValueError, match='n_images'):                 # more images than NNHIP_NEB_MAX_IMAGES
        ok.band(z70, pos70, cell70, batch70, 70)
    for name in ('spring', 'fmax', 'climb_below', 'dt', 'dt_max', 'maxstep'):
        for bad in (0.0, -1.0, float('nan'), float('inf'), 'x'):
            with pytest.raises(ValueError, match=name):
                ok.band(z, pos, cell, batch, 3, **{name: bad})
    with pytest.raises(ValueError, match='dt'):
        ok.band(z, pos, cell, batch, 3, dt=2.0, dt_max=1.0)
    with pytest.raises(RuntimeError, match='MI355X'):                 # CPU tensors: no CPU path
        ok.band(z, pos, cell, batch, 3)
    with pytest.raises(RuntimeError, match='MI355X'):
        Band(ok, z, pos, cell, batch, [3])
    assert band_counts(3, 9) == [3, 3, 3] and band_counts([4, 5], 9) == [4, 5] and band_counts(np.int64(9), 9) == [9]
    # Band.run takes relax's checks of its three numbers
    for bad in ((-1, 10, 0), (2.5, 10, 0), (5, -1, 0), (5, 10, -2), (5, 1.5, 0)):
        with pytest.raises(ValueError):
            check_run_arguments(*bad)
    import inspect
    assert 'check_run_arguments(max_steps, check_every, record_every)' in inspect.getsource(Band.run)
    # interpolate: linear, endpoints bitwise, on the inputs' device
    a, b = torch.randn(4, 3), torch.randn(4, 3)
    im = interpolate(a, b, 5)
    assert im.shape == (5, 4, 3) and torch.equal(im[0], a) and torch.equal(im[-1], b)
    assert torch.allclose(im[2], 0.5 * (a + b), atol=1e-6) and torch.allclose(im[1] - im[0], im[3] - im[2], atol=1e-6)
    for bad in (2, 2.5, 65):
        with pytest.raises(ValueError, match='n_images'):
            interpolate(a, b, bad)
    with pytest.raises(ValueError, match='interpolate'):
        interpolate(a, b[:3], 5)


def test_calculator_neb_validates_before_any_device_work():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype = torch.device('cpu'), torch.float32
    calc.model = _FakeModel()
    a, b = FakeAtoms([8, 1, 1], np.zeros((3, 3))), FakeAtoms([6, 1], np.zeros((2, 3)))
    with pytest.raises(ValueError, match='at least one'):
        calc.neb([])
    with pytest.raises(ValueError, match='images'):
        calc.neb([a, a])
    with pytest.raises(ValueError, match='images'):
        calc.neb([[a, a, a], [b, b]])
    with pytest.raises(ValueError, match='sizes'):
        calc.neb([a, b, a])
    with pytest.raises(ValueError, match='fmax'):
        calc.neb([a, a, a], fmax=-0.01)
    with pytest.raises(ValueError, match='spring'):
        calc.neb([a, a, a], spring=0.0)
    with pytest.raises(ValueError, match='climb_below'):
        calc.neb([a, a, a], climb_below=float('nan'))
    with pytest.raises(ValueError, match='maxstep'):
        calc.neb([a, a, a], maxstep=0.0)
    with pytest.raises(ValueError, match='max_steps'):
        calc.neb([a, a, a], max_steps=2.5)
    with pytest.raises(ValueError, match='check_every'):
        calc.neb([a, a, a], check_every=-1)
    with pytest.raises(ValueError, match='fixed'):
        calc.neb([a, a, a], fixed=[True, False])
    with pytest.raises(ValueError, match='fixed'):
        calc.neb([[a, a, a], [b, b, b]], fixed=[True, False, False])
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.neb([a, a, a])
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.neb([[a, a, a], [b, b, b, b]])


# ---- the reference is a climbing-image NEB ---------------------------------------------------------------------------------------------

# Mueller-Brown (Mueller and Brown 1979) for ONE "atom" (x, y) plus a harmonic z term, scaled by MB_SCALE = 1e-3: the surface's
# energies of ~100 and curvatures of up to ~4000 become ~0.1 eV and <= 4.1 eV/A^2, so that FIRE with ASE's dt_max = 1 (mass 1) is
# at its stability limit omega dt = 2 only at the stiffest point of the deepest minimum and well inside it along the path
MB_SCALE = 1e-3
MB_KZ = 1.0                                                  # eV/A^2, the z term
_A, _a, _b = np.array([-200., -100., -170., 15.]), np.array([-1., -1., -6.5, 0.7]), np.array([0., 0., 11., 0.6])
_c, _X0, _Y0 = np.array([-10., -10., -6.5, 0.7]), np.array([1., 0., -0.5, -1.]), np.array([0., 0.5, 1.5, 1.])
MB_SADDLE = np.array([-0.822, 0.624])                        # the known saddle between the minima below (3 decimals)
MB_MIN_A, MB_MIN_B = np.array([-0.558, 1.442]), np.array([-0.050, 0.467])


def _mb(p):
    dx, dy = p[..., 0:1] - _X0, p[..., 1:2] - _Y0
    e = _A * np.exp(_a * dx * dx + _b * dx * dy + _c * dy * dy)
    f = -np.stack([(e * (2 * _a * dx + _b * dy)).sum(-1), (e * (_b * dx + 2 * _c * dy)).sum(-1)], -1)
    return MB_SCALE * e.sum(-1), MB_SCALE * f


def _mb_hessian(p, h=1e-5):
    H = np.zeros((2, 2))
    for i in range(2):
        d = np.zeros(2)
        d[i] = h
        H[i] = -(_mb(p + d)[1] - _mb(p - d)[1]) / (2 * h)
    return 0.5 * (H + H.T)


def _mb_stationary(p):
    for _ in range(30):
        p = p + np.linalg.solve(_mb_hessian(p), _mb(p)[1])
    return p


def _mb_energy_forces(x):
    E, f = _mb(x[:, 0, :2])
    z = x[:, 0, 2]
    return E + 0.5 * MB_KZ * z * z, np.concatenate([f, -MB_KZ * z[:, None]], 1)[:, None]


def test_reference_finds_the_mueller_brown_saddle():
    saddle = _mb_stationary(MB_SADDLE)
    assert np.abs(saddle - MB_SADDLE).max() < 1e-3
    lam = np.linalg.eigvalsh(_mb_hessian(saddle))
    assert lam[0] < 0 < lam[1]
    ends = [_mb_stationary(MB_MIN_A), _mb_stationary(MB_MIN_B)]
    n_img, fmax = 9, 1e-3
    w = np.linspace(0, 1, n_img)[:, None]
    x0 = np.zeros((n_img, 1, 3))
    x0[:, 0, :2] = ends[0] * (1 - w) + ends[1] * w
    x0[1:-1, 0, 2] = 0.05                                     # off the plane: the z term has to bring the images back
    out = nr.minimise(_mb_energy_forces, x0, spring=0.1, fmax=fmax, climb_below=5 * fmax, max_steps=2000)
    assert out['converged'] and out['climbing'] and out['fmax'] < fmax and out['n_steps'] < 400
    assert np.array_equal(out['x'][0], x0[0]) and np.array_equal(out['x'][-1], x0[-1])        # endpoints bitwise
    top = out['saddle']
    ci = out['x'][top, 0]
    # at a converged climbing image |F| = |f| < fmax (the reflection keeps the norm), so to first order the image lies within
    # fmax / min |lambda| of the stationary point (lambda: the Hessian's eigenvalues there, kz among them); twice that allows for the
    # second order
    tol = 2.0 * fmax / min(abs(lam[0]), abs(lam[1]), MB_KZ)
    dist = float(np.linalg.norm(ci - np.append(saddle, 0.0)))
    print(f'Mueller-Brown x {MB_SCALE}: {out["n_steps"]} steps (climbing from step {out["climb_step"]}), climbing image {top} at '
          f'{ci[:2]}, {dist:.2e} A from the saddle {saddle} (allowed {tol:.2e}); eigenvalues there {lam}; barrier '
          f'{out["barrier_forward"]:.5f} eV')
    assert dist <= tol
    assert abs(out['barrier_forward'] - (_mb(saddle)[0] - _mb(ends[0])[0])) <= fmax * dist + 1e-9
    # the nudging: in F the spring force has no perpendicular part and the true force no parallel part
    E, F = _mb_energy_forces(out['x'])
    x, t, Fn = out['x'], out['tangent'], out['neb_force']
    for i in range(1, n_img - 1):
        that = t[i].reshape(-1)
        assert abs(that @ that - 1.0) < 1e-12
        f = F[i].reshape(-1)
        spring = 0.1 * (np.linalg.norm(x[i + 1] - x[i]) - np.linalg.norm(x[i] - x[i - 1])) * that
        perp = Fn[i].reshape(-1) - (Fn[i].reshape(-1) @ that) * that
        np.testing.assert_allclose(perp, f - (f @ that) * that, rtol=0, atol=1e-15)              # only the true force, perpendicular
        par = float(Fn[i].reshape(-1) @ that)
        want = -(f @ that) if i == top else float(spring @ that)                                # only the spring (or the reflection)
        assert abs(par - want) <= 1e-15, (i, par, want)
    assert np.all(np.abs(t[0]) == 0) and np.all(Fn[-1] == 0)
    # without the climbing image the band converges too, and its highest image is NOT at the saddle to that tolerance
    plain = nr.minimise(_mb_energy_forces, x0, spring=0.1, fmax=fmax, climb=False, max_steps=2000)
    assert plain['converged'] and not plain['climbing']
    assert plain['energy'][plain['saddle']] < out['energy'][top] and np.linalg.norm(plain['x'][plain['saddle'], 0, :2] - saddle) > tol
    # fixed "atom": a band whose only atom is fixed never moves: its first launch switches the climbing image on, its second converges
    held = nr.minimise(_mb_energy_forces, x0, fmax=fmax, max_steps=5, free=np.zeros((n_img, 1), dtype=bool))
    assert held['converged'] and held['n_steps'] == 1 and np.array_equal(held['x'], x0)


def test_reference_fire_step_is_ases():
    """three steps of ase.optimize.FIRE written out (mass 1) on the NEB forces of a band, against neb_step"""
    rng = np.random.default_rng(5)
    n_img, n = 5, 4
    x = rng.normal(0, 1, (n_img, n, 3))
    prm = nr.params(0.1, 1e-6)
    st = nr.new_state(n_img, n)
    v = None
    dt, a, n_pos = nr.FIRE['dt'], nr.FIRE['a_start'], 0
    for step in range(8):
        E = -(x ** 2).sum((1, 2)) * 0.01 + np.arange(n_img) * 0.02
        F = 0.3 * np.sin(x + step)                          # any forces: signs of P of both kinds come up
        r = nr.neb_step(x, F, E, None, st, prm, nr.CLIMB, eps=0.0)
        Fn = r['neb_force']
        if v is None:
            v = np.zeros_like(x)
        else:
            vf = float((Fn * v).sum())
            if vf > 0.0:
                v = (1.0 - a) * v + a * Fn / np.sqrt((Fn * Fn).sum()) * np.sqrt((v * v).sum())
                if n_pos > 5:
                    dt = min(dt * nr.FIRE['f_inc'], 1.0)
                    a *= nr.FIRE['f_a']
                n_pos += 1
            else:
                v = np.zeros_like(x)
                a, dt, n_pos = nr.FIRE['a_start'], dt * 0.5, 0
        v = v + dt * Fn
        dr = dt * v
        norm = np.sqrt((dr * dr).sum())
        if norm > nr.FIRE['maxstep']:
            dr = nr.FIRE['maxstep'] * dr / norm
        np.testing.assert_allclose(r['x_out'], x + dr, rtol=1e-13, atol=1e-15)
        assert r['state']['n_pos'] == n_pos and abs(r['state']['dt'] - dt) < 1e-15 and abs(r['state']['a'] - a) < 1e-15
        x, st = r['x_out'], r['state']
    assert st['n_steps'] == 8


# ---- the bound ------------------------------------------------------------------------------------------------------------------------

def test_float32_emulation_stays_inside_the_bound_and_the_bound_scales_with_eps(syn):
    prm = nr.params(nr.SYN_SPRING, nr.SYN_FMAX, nr.SYN_CLIMB_BELOW)
    worst = dict(x=0.0, F=0.0, t=0.0, v=0.0)
    moved = 0
    for k, b in enumerate(syn):
        if b['kind'] == 'unequal':
            continue
        for flags in FLAG_SETS:
            ref = nr.band_step(b, flags)
            emu = nr.emulate_step(b['x'], b['F'], b['E'], b['free'], nr.band_state(b), prm, flags)
            what = (k, b['kind'], flags)
            new = ref['state']
            for name in ('converged', 'climbing', 'n_steps', 'n_pos'):
                assert emu[name] == new[name], what + (name,)
            assert emu['saddle'] == ref['saddle']
            assert abs(float(emu['fmax']) - ref['fmax']) <= ref['b_fmax'] + nr.half_ulp32(ref['fmax']), what
            for key, val, rv, rb in (('F', emu['neb_force'], ref['neb_force'], ref['b_neb_force']),
                                     ('t', emu['tangent'], ref['tangent'], ref['b_tangent']),
                                     ('x', emu['pos_out'], ref['x_out'], ref['bx'])):
                err, bound = np.abs(val.astype(np.float64) - rv), rb + nr.half_ulp32(rv)
                assert np.all(err <= bound), what + (key, float((err / bound).max()))
                worst[key] = max(worst[key], float((err / bound).max()))
            if ref['frozen']:
                assert np.array_equal(emu['pos_out'], b['x']) and np.array_equal(emu['vel'], b['vel'])
                continue
            moved += 1
            err, bound = np.abs(emu['vel'].astype(np.float64) - new['vel']), ref['b_vel_out'] + nr.half_ulp32(new['vel'])
            assert np.all(err <= bound), what + ('vel', float((err / bound).max()))
            worst['v'] = max(worst['v'], float((err / bound).max()))
            assert abs(float(emu['dt']) - new['dt']) <= ref['b_dt_out'] + nr.half_ulp32(new['dt']), what
            assert abs(float(emu['a']) - new['a']) <= ref['b_a_out'] + nr.half_ulp32(new['a']), what
            fixed = ~np.broadcast_to(b['free'][:, :, None], b['x'].shape).copy()
            fixed[0], fixed[-1] = True, True
            assert np.array_equal(emu['pos_out'][fixed], b['x'][fixed]) and np.array_equal(emu['vel'][fixed], b['vel'][fixed])
            if flags == nr.CLIMB:
                # first order in eps: twice the eps, twice the bound (TINY32 aside); no eps, no bound
                two, zero = nr.band_step(b, flags, eps=2.0 * nr.EPS32), nr.band_step(b, flags, eps=0.0)
                for key in ('bx', 'b_neb_force', 'b_tangent', 'b_vel_out'):
                    np.testing.assert_allclose(two[key] - nr.TINY32 * (two[key] > 0), 2.0 * (ref[key] - nr.TINY32 * (ref[key] > 0)),
                                               rtol=1e-9, err_msg=str(what + (key,)))
                    assert np.all(zero[key] <= nr.TINY32)
                # and not vacuous: a moving coordinate's bound is at least its last rounding and far below the step itself
                mv = ref['bx'] > 0
                assert np.all(ref['bx'][mv] >= nr.C_NEB * nr.EPS32 * np.abs(ref['x_out'][mv]))
                assert ref['bx'].max() <= 1e-2 * np.abs(ref['x_out'] - b['x']).max() + 16 * nr.EPS32 * 8.0, what
    assert moved > 100
    print(f'float32 emulation over {moved} moving band-launches: worst err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items())
          + f' (C_NEB = {nr.C_NEB})')
    assert max(worst.values()) <= 0.75


def test_synthetic_kernel_inputs_cover_every_branch_without_an_ambiguous_decision(syn):
    seen = set()
    sizes, images = set(), set()
    for k, b in enumerate(syn):
        if b['kind'] == 'unequal':
            assert len(set(b['sizes'])) > 1
            continue
        st = nr.band_state(b)
        fixed = bool((~b['free']).any())
        for flags in FLAG_SETS:
            r = nr.band_step(b, flags)
            assert not any(r['ambiguous'].values()), (k, b['kind'], flags, r['ambiguous'])
            new = r['state']
            seen.add((b['kind'], flags, r['frozen'], r['fire'], new['converged'], new['climbing']))
            if not r['frozen']:
                seen.add(('fire', r['fire'], r['clamped']))
                seen.add(('fixed atoms move nothing', fixed))
            if r['capped']:
                seen.add('dt capped')
            if st['climbing'] and not r['frozen']:
                seen.add(('climbing image at', r['saddle'] == 1, r['saddle'] == b['n_img'] - 2))
        sizes.add(b['n'])
        images.add(b['n_img'])
        seen.add((b['profile'], tuple(sorted(set(r['cases'])))))
        seen.update(('case', c) for c in r['cases'])
        seen.add((b['profile'], 'top', r['saddle']) if b['profile'] in ('ties', 'flat') else (b['profile'], 'top'))
        if b['kind'] in ('coincident', 'flat'):
            i = 1
            assert not r['tangent'][i].any(), 'a zero-length tangent must give the zero vector'
            np.testing.assert_array_equal(r['neb_force'][i], np.where(b['free'][i][:, None], b['F'][i].astype(np.float64), 0.0))
    assert sizes == set(nr.SYN_SIZES) | {21} and images == set(nr.SYN_IMAGES)
    C, K = nr.CLIMB, nr.CLIMB | nr.CHECK_ONLY
    want = [
        # FIRE: first step, P > 0 below and above n_min, dt at the cap, P <= 0; each with and without the clamp
        *[('fire', f, c) for f in ('first', 'mix', 'mix_inc', 'reset') for c in (False, True)], 'dt capped',
        ('fixed atoms move nothing', True), ('fixed atoms move nothing', False),
        # climbing: not allowed (no CLIMB: never set), off (CLIMB, fmax above climb_below), switching now, on
        ('switch', 0, False, 'mix', False, False), ('first', C, False, 'first', False, False), ('switch', C, False, 'mix', False, True),
        ('climbing', C, False, 'mix', False, True),
        # convergence: already, now, check-only (no flag set), tol2 met while the climb is pending (sets the flag, moves on)
        ('converged', C, True, None, True, False), ('converging', C, True, None, True, True), ('converging', 0, True, None, True, True),
        ('converging', K, True, None, False, True), ('pending', K, True, None, False, False), ('pending', C, False, 'mix', False, True),
        ('pending', 0, True, None, True, False),
        # tangents: the two pure cases, the mixed one; the plateau of 'ties' gives the lowest index
        ('case', 'up'), ('case', 'down'), ('case', 'mixed'), ('rising', ('up',)), ('falling', ('down',)), ('ties', 'top', 1),
        ('flat', 'top', 1), ('max_first', 'top'), ('max_mid', 'top'), ('max_last', 'top'), ('min', 'top'),
        ('climbing image at', True, False), ('climbing image at', False, True), ('climbing image at', False, False)]
    for w in want:
        assert w in seen, w
