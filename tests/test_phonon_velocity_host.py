"""Host-side checks of the phonon group velocities: the fp64 yardstick (tests/phonon_velocity_ref.py) against an analytic lattice
and against central differences of its own eigenvalues, the rule at a crossing, the condition on the inputs of the device tests,
the argument checks, the unit factors, the ABI symbol, and the call sequence with and without the option (no device)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from newtonnet_amd import phonons as ph
from tests import phonon_ref as pr
from tests import phonon_velocity_ref as pv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_yardstick_against_the_analytic_lattice():
    for n_fold in pv.ANALYTIC_FOLDS:
        case = pv.coupled_cubic_lattice(n_fold=n_fold)
        for q in pv.ANALYTIC_Q:
            p = pv.problem(*case, q)
            lam, dlam = pv.coupled_cubic_analytic(q, n_fold=n_fold)
            assert len(set(p['first'])) == 3 * n_fold and not p['capped'].any()          # a generic q: no groups
            assert np.abs(p['lam'] - lam).max() <= 1e-13 * np.abs(lam).max()
            assert np.abs(p['dlam'] - dlam).max() <= 1e-13 * np.abs(dlam).max()


def test_yardstick_against_central_differences_of_its_own_eigenvalues():
    _, fc = pr.random_crystal(2, pr.TRICLINIC_S, 5)
    args = (fc, pr.TRICLINIC_POS, pr.TRICLINIC_CELL, pr.TRICLINIC_S, pr.TRICLINIC_MASSES)
    table = pr.image_table_fast(*args[1:4])
    q = np.array([0.31, -0.17, 0.44])
    p = pv.problem(*args, q, table=table)
    assert len(set(p['first'])) == 6
    h = 1e-6                                         # 1 / A
    to_frac = pr.TRICLINIC_CELL / (2.0 * np.pi)      # q_frac = q_cart @ cell^T / 2 pi
    for a in range(3):
        dq = np.zeros(3)
        dq[a] = h
        dq = dq @ to_frac.T
        up = np.linalg.eigvalsh(pr.dynamical_matrix(*args, q + dq, table))
        dn = np.linalg.eigvalsh(pr.dynamical_matrix(*args, q - dq, table))
        fd = (up - dn) / (2.0 * h)
        assert np.abs(fd - p['dlam'][:, a]).max() <= 1e-8 * np.abs(p['dlam']).max()


def test_crossing_pairs_come_out_as_the_unfolded_branches():
    # pr.cubic_lattice's springs folded twice: at q_x = 1/2 the x branches of k = 0 and k = 1 cross with slopes -7.5 and +7.5
    p = pv.problem(*pv.folded_cubic_lattice(2), np.array([0.5, 0.1, 0.2]), direction=pv.CROSSING_DIRECTION)
    assert p['first'].tolist() == [0, 0, 2, 2, 4, 4]
    assert np.allclose(p['dlam'][4:, 0], [-7.5, 7.5], rtol=0, atol=1e-13) and np.abs(p['dlam'][4:, 1:]).max() <= 1e-13
    # the coupled lattice: every mode sits in a pair (k, n_fold - 1 - k); along the direction the pair is (-v_x, +v_x)
    for n_fold in (2, 22):
        p = pv.problem(*pv.coupled_cubic_lattice(n_fold=n_fold), pv.CROSSING_Q, direction=pv.CROSSING_DIRECTION)
        lam, dlam = pv.coupled_cubic_analytic(pv.CROSSING_Q, n_fold=n_fold)
        assert p['first'].tolist() == [2 * (k // 2) for k in range(3 * n_fold)]
        for s in range(0, 3 * n_fold, 2):
            pair = dlam[s:s + 2][np.argsort(dlam[s:s + 2] @ pv.CROSSING_DIRECTION)]
            assert np.abs(p['dlam'][s:s + 2] - pair).max() <= 1e-12 * np.abs(dlam).max()
            assert pair[0, 0] < 0.0 < pair[1, 0] and abs(pair[0, 0] + pair[1, 0]) <= 1e-12


def test_group_cap_and_zero_modes():
    p = pv.problem(*pv.folded_cubic_lattice(22), np.array([0.3, 0.1, 0.2]))
    assert p['capped'].sum() == 44 and not p['defined'][p['capped']].any() and np.abs(p['v'][p['capped']]).max() == 0.0
    assert sorted(np.unique(p['first'][p['capped']], return_counts=True)[1].tolist()) == [22, 22]
    g = pv.problem(*pv.coupled_cubic_lattice(n_fold=2), np.zeros(3))
    assert (~g['defined']).sum() == 3 and np.array_equal(g['n'], [1.0, 0.0, 0.0])


def test_the_bound_of_the_device_tests_is_tight_on_their_inputs():
    """For every mode the analytic device test compares, the bound C eps32 max ||G_a|| (1 + ||D|| / gap) with the tests' constant is
    at most 1 % of the problem's largest |dlam| (the end-to-end test, whose force constants exist on the device only, asserts the
    same on its own inputs).

    Figures with BOUND_C = 16: at most 0.79 % at n_fold = 22 (d = 66), below 0.02 % at d = 3 and 6.  The q are the best of a scan
    through the lattice's formula; twice the constant would not fit d = 66 (1.25 % at best)."""
    for n_fold in pv.ANALYTIC_FOLDS:
        case = pv.coupled_cubic_lattice(n_fold=n_fold)
        for q, n in [(q, None) for q in pv.ANALYTIC_Q] + [(pv.CROSSING_Q, pv.CROSSING_DIRECTION)]:
            p = pv.problem(*case, q, direction=n)
            keep = p['defined']
            ratio = (pv.error_bound(pv.BOUND_C, p)[keep] / np.abs(p['dlam']).max()).max()
            print(f'n_fold {n_fold} q {q}: bound / max |dlam| = {ratio:.2e}')
            assert ratio <= 0.01
    # the 33-atom crystal of the end-to-end case at d = 99 (fp32 force constants, as the device holds them)
    fc, pos, cell, S, m = pv.planted_levels_crystal(pv.straddle_levels('pair'))
    p = pv.problem(fc.astype(np.float32).astype(np.float64), pos, cell, S, m.astype(np.float32).astype(np.float64), pv.STRADDLE_Q)
    ratio = (pv.error_bound(pv.BOUND_C, p) / np.abs(p['dlam']).max()).max()
    print(f'd = 99: bound / max |dlam| = {ratio:.2e}')
    assert ratio <= 0.01 and p['defined'].all()


def test_designed_spectrum_of_the_33_atom_crystal():
    for kind in ('pair', 'cap'):
        lev = pv.straddle_levels(kind)
        p = pv.problem(*pv.planted_levels_crystal(lev), pv.STRADDLE_Q)
        assert np.abs(p['lam'] - np.sort(lev)).max() <= 1e-12 * lev.max()
        want = np.arange(99)
        if kind == 'pair':          # the group straddles modes 63 | 64, the boundary of the kernel's tiles of 64 modes
            want[64] = 63
            assert np.abs(p['dlam'][64] - p['dlam'][63]).max() > 1.0 and (p['dlam'][64] - p['dlam'][63]) @ p['n'] > 0
        else:
            want[55:73] = 55
            assert p['capped'].sum() == 18
        assert np.array_equal(p['first'], want)


def test_unit_factors_against_codata():
    e, amu, c = 1.602176634e-19, 1.66053906660e-27, 2.99792458e8
    v = np.sqrt(e / amu) * 1e-2          # m / s -> A / ps
    assert abs(ph.ANGSTROM_PER_PS_PER_SQRT_EV_AMU - v) <= 1e-12 * v and abs(v - 98.2269) < 1e-3
    assert abs(pv.ANGSTROM_PER_PS_PER_SQRT_EV_AMU - v) <= 1e-12 * v
    k = e * 1e22                         # eV / (K A ps) -> W / (m K)
    assert abs(ph.WATT_PER_M_K_PER_PS - k) <= 1e-12 * k and abs(pv.WATT_PER_M_K_PER_PS - k) <= 1e-12 * k
    # the wavenumber of the same unit frequency, the way the module derives the factor
    from newtonnet_amd import vibrations
    assert abs(vibrations.WAVENUMBER_PER_SQRT_EIGENVALUE * 2.0 * np.pi * c * 100.0 * 1e-12 - v) <= 1e-12 * v
    assert ph.MAX_DEGENERATE == pv.MAX_DEGENERATE == 16 and ph.STATUS_GROUP == 8 and ph.STATUS_NONFINITE == 16


def test_new_arguments_are_checked_before_any_device_work():
    fc, pos, cell = pr.cubic_lattice()
    p = ph.Phonons.from_force_constants(fc, [1], pos, cell, pr.CUBIC_S, masses=[pr.CUBIC_MASS], device='cpu')
    q = [[0.1, 0.2, 0.3], [0.0, 0.0, 0.0]]
    for bad in (np.ones(2), np.ones((3, 3)), np.ones((2, 2))):
        with pytest.raises(ValueError, match='direction'):
            p.frequencies(q, velocities=True, direction=bad)
    with pytest.raises(ValueError, match='finite'):
        p.frequencies(q, velocities=True, direction=[1.0, float('nan'), 0.0])
    with pytest.raises(ValueError, match='non-zero'):
        p.frequencies(q, velocities=True, direction=[[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    for bad in (-1e-3, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='degeneracy_tol'):
            p.frequencies(q, velocities=True, degeneracy_tol=bad)
    with pytest.raises(ValueError, match='zero length'):
        p.band_structure([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], 4, velocities=True)
    with pytest.raises(RuntimeError, match='MI355X'):          # ... and a good set of arguments gets as far as the device check
        p.frequencies(q, velocities=True, direction=[0.0, 2.0, 0.0], degeneracy_tol=1e-4)
    n = ph._check_direction([0.0, 2.0, 0.0], 2)
    assert n.shape == (2, 3) and np.array_equal(n, [[0.0, 1.0, 0.0]] * 2)
    d = ph.segment_directions([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.5, 0.5, 0.0]], 2, pr.TRICLINIC_CELL)
    recip = 2.0 * np.pi * np.linalg.inv(pr.TRICLINIC_CELL).T
    want = [recip[0] / np.linalg.norm(recip[0])] * 2 + [recip[1] / np.linalg.norm(recip[1])] * 3
    assert d.shape == (5, 3) and np.allclose(d, want, rtol=0, atol=1e-15)
    bands = ph.PhononBands(q=np.zeros((1, 3)))
    assert bands.group_velocities is None and bands.velocity_defined is None and bands.degenerate_group is None
    assert bands.eigenvalue_gradients is None
    with pytest.raises(ValueError, match='velocities=True'):
        bands.velocities(0)
    with pytest.raises(ValueError, match='velocities=True'):
        ph.PhononMesh(bands, p).transport_tensor(300.0)


def test_kernel_symbol_is_declared_listed_and_exported():
    from newtonnet_amd import abi, hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    name = 'nnhip_phonon_velocities'
    assert name in declared and name in abi.FUNCTIONS and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bphonon_velocity\b.*\)', f.read(), re.M)
    # the size bound and the null pointers are refused by the library itself, from the host offsets and before any launch
    hip.abi.bind(lib, (name, 'nnhip_last_error'))
    one = ctypes.c_void_p(8)            # never dereferenced
    big = (ctypes.c_int32 * 2)(0, ph.max_dim_large() // 3 + 1)
    args = [one, one, one, big, one, one, one, one, None, one, 1, one, one, 1, None, one, one, one, one, one, None, None, one, one, None]
    assert lib.nnhip_phonon_velocities(*args) == 2 and str(ph.max_dim_large()) in lib.nnhip_last_error().decode()
    ok = (ctypes.c_int32 * 2)(0, 2)
    for k in (0, 11, 15, 16, 19, 22, 23):          # fc, cells, evals, modes, vel, defined, status
        a = list(args)
        a[3] = ok
        a[k] = None
        assert lib.nnhip_phonon_velocities(*a) == 1, k
    assert lib.nnhip_phonon_velocities(*(args[:10] + [0] + args[11:])) == 0          # no crystals: nothing to do


class _Device(str):
    """a device string torch takes for 'cpu' that tells Phonons.frequencies it is a GPU"""
    type = 'cuda'


class _OnDevice(torch.Tensor):
    device = property(lambda self: _Device('cpu'))


class _Recorder:
    """stands in for the library: records (name, which arguments are null) of every call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            if name == 'nnhip_phonon_max_dim':
                return 96
            if name == 'nnhip_phonon_large_max_dim':
                return 768
            self.calls.append((name, tuple(a if isinstance(a, int) and abs(a) < 1 << 20 else a is not None for a in args)))
            return 0
        return call


def test_without_the_option_the_call_sequence_is_untouched(monkeypatch):
    from newtonnet_amd import hip
    fc, pos, cell = pr.cubic_lattice()
    p = ph.Phonons.from_force_constants(fc, [1], pos, cell, pr.CUBIC_S, masses=[pr.CUBIC_MASS], device='cpu')
    p.fc = p.fc.as_subclass(_OnDevice)
    rec = _Recorder()
    monkeypatch.setattr(hip, 'lib', lambda: rec)
    monkeypatch.setattr(hip, '_stream', lambda dev: None)
    q = [[0.1, 0.2, 0.3], [0.0, 0.0, 0.0]]
    seen = {}
    for key, kw in (('plain', {}), ('off', dict(velocities=False)), ('modes', dict(modes=True)), ('on', dict(velocities=True)),
                    ('both', dict(velocities=True, modes=True, dynamical_matrix=True))):
        rec.calls.clear()
        out = p.frequencies(q, **kw)
        seen[key] = (list(rec.calls), out)
    assert [c[0] for c in seen['plain'][0]] == ['nnhip_phonon_bands']
    assert seen['plain'][0] == seen['off'][0] and seen['plain'][0][0][1][14] is False          # no modes asked of the kernel
    assert seen['plain'][1].group_velocities is None and seen['plain'][1].modes is None
    assert [c[0] for c in seen['on'][0]] == ['nnhip_phonon_bands', 'nnhip_phonon_velocities']
    assert seen['on'][0][0] == seen['modes'][0][0]                   # the bands launch of modes=True, then one more launch
    assert seen['on'][1].modes is None and seen['both'][1].modes is not None and seen['both'][1].dynamical_matrix is not None
    for key in ('on', 'both'):
        out = seen[key][1]
        assert tuple(out.group_velocities.shape) == (6, 3) and out.group_velocities.dtype == torch.float32
        assert out.velocity_defined.dtype == torch.bool and out.degenerate_group.dtype == torch.int32
        v, ok = out.velocities(0)
        assert tuple(v.shape) == (2, 3, 3) and tuple(ok.shape) == (2, 3)
    name, a = seen['on'][0][1]
    assert a[10] == 1 and a[13] == 2 and a[14] is False and a[20] is True and a[21] is True          # n_cry, n_q, direction, dlam, group
    # an explicit direction reaches the kernel; band_structure hands over one per crystal
    rec.calls.clear()
    p.frequencies(q, velocities=True, direction=[0.0, 0.0, 3.0])
    assert rec.calls[1][1][14] is True
    rec.calls.clear()
    p.band_structure([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], 3, velocities=True)
    assert [c[0] for c in rec.calls] == ['nnhip_phonon_bands', 'nnhip_phonon_velocities'] and rec.calls[1][1][14] is True
    rec.calls.clear()
    m = p.mesh(2, 2, 2, velocities=True)
    assert [c[0] for c in rec.calls] == ['nnhip_phonon_bands', 'nnhip_phonon_velocities'] and rec.calls[1][1][14] is False
    assert tuple(m.transport_tensor(300.0).shape) == (1, 3, 3)
