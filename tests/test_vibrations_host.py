"""CPU-side checks of the normal-mode analysis (newtonnet_amd/vibrations.py, csrc/eig.hip): the C ABI exports the solver, the
unit constant and the mass table are what they claim, and the fp64 yardstick the GPU tests compare against (tests/vib_ref.py)
is itself right on the oracle's Hessian."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import hessian_ref as hr
from tests import util
from tests import vib_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solver_symbols_are_declared_listed_and_exported():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for sym in ('nnhip_eig_blocks', 'nnhip_eig_max_dim'):
        assert sym in declared, f'{sym} is not declared in the header'
        assert sym in hip.EXPORTED_SYMBOLS, f'{sym} is not listed in EXPORTED_SYMBOLS'
        assert hasattr(lib, sym), f'{sym} is not exported'
    lib.nnhip_eig_max_dim.restype = ctypes.c_int
    assert lib.nnhip_eig_max_dim() >= 96
    assert lib.nnhip_version() >= 110


def test_wavenumber_constant_from_codata():
    from newtonnet_amd import vibrations as vib
    e, amu, c_cm, h = 1.602176634e-19, 1.66053906660e-27, 2.99792458e10, 6.62607015e-34
    want = math.sqrt(e / (1e-20 * amu)) / (2.0 * math.pi * c_cm)
    assert abs(want - 521.4709) < 1e-3
    assert abs(vib.WAVENUMBER_PER_SQRT_EIGENVALUE - want) <= 1e-6 * want
    assert abs(vr.WAVENUMBER - want) <= 1e-6 * want
    # zero-point energy: hbar omega / 2 = h c nu~ / 2
    assert abs(vib.EV_PER_WAVENUMBER - h * c_cm / e) <= 1e-6 * h * c_cm / e
    assert abs(vib.EV_PER_WAVENUMBER - 1.239841984e-4) <= 1e-6 * 1.239841984e-4


def test_mass_table():
    from newtonnet_amd import vibrations as vib
    for z, m in ((1, 1.008), (6, 12.011), (7, 14.007), (8, 15.999)):
        assert vib.atomic_mass(z) == m
    got = vib.table_masses(torch.tensor([8, 1, 1, 6, 7]))
    assert got.dtype == torch.float32
    assert torch.equal(got, torch.tensor([15.999, 1.008, 1.008, 12.011, 14.007], dtype=torch.float32))
    for bad in (0, 118, 43, 200, -1):
        with pytest.raises(ValueError, match='masses='):
            vib.atomic_mass(bad)
        with pytest.raises(ValueError, match='masses='):
            vib.table_masses(torch.tensor([1, bad]))


def test_solver_refuses_host_inputs():
    from newtonnet_amd import vibrations as vib
    with pytest.raises(RuntimeError, match='cuda'):
        vib.eig_blocks(torch.zeros(9), torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long), torch.zeros(1, 3),
                       torch.zeros(1, 3, 3))


def test_yardstick_on_the_oracle_hessian_of_ethanol():
    """Without projection the three translations are exact null vectors of the oracle's mass-weighted Hessian (translation invariance
    of the energy) while the rotations are not (the geometry is not stationary): three, not six, eigenvalues vanish.  With
    projection exactly n_proj = 6 do.  Measured: ||A d|| / (||A||_2 ||d||) = 2e-17 .. 4e-17; unprojected |lambda| / s =
    1e-17 .. 6e-17 for three eigenvalues, then 2.1e-4 or more; projected: six below 1.1e-16, then 1.4e-3 or more."""
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand', torch.float32)
    H = hr.oracle_hessian(sd, z, pos.double(), cell.double(), batch).numpy()
    for b in range(int(batch.max()) + 1):
        idx = (batch == b).nonzero().reshape(-1).numpy()
        Hb, pb = H[idx][:, :, idx], pos[idx].double().numpy()
        m = np.array([vr.MASSES[int(q)] for q in z[idx]])
        free = vr.analyse(Hb, pb, m, project=False)
        s = free['s']
        assert s > 0 and free['n_proj'] == 0
        D = vr.tr_rot_vectors(pb, m)
        assert D.shape == (6, 27)
        assert np.abs(D @ D.T - np.eye(6)).max() <= 1e-12
        for d in D[:3]:
            r = np.linalg.norm(free['A'] @ d)
            print(f'molecule {b}: ||A d|| / (s ||d||) = {r / s:.2e}')
            assert r <= 1e-8 * s * np.linalg.norm(d)
        small = np.sort(np.abs(free['evals']))
        print(f'molecule {b}: unprojected smallest |lambda| / s', small[:7] / s)
        assert np.count_nonzero(small <= 1e-12 * s) == 3          # the translations only: the six smallest are not all zero
        proj = vr.analyse(Hb, pb, m, project=True)
        small = np.sort(np.abs(proj['evals']))
        print(f'molecule {b}: projected smallest |lambda| / s', small[:8] / proj['s'])
        assert proj['n_proj'] == 6
        assert np.count_nonzero(small <= 1e-12 * proj['s']) == 6
        # the projection leaves the other eigenvalues of P A P what they are: A_proj d = 0 for every projected vector
        assert np.abs(proj['A'] @ D.T).max() <= 1e-12 * s


def test_yardstick_drop_rule_for_linear_single_and_periodic_molecules():
    m2, m1 = np.array([1.008, 1.008]), np.array([15.999])
    assert len(vr.tr_rot_vectors(np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.74]]), m2)) == 5
    assert len(vr.tr_rot_vectors(np.array([[1.0, 2.0, 3.0]]), m1)) == 3
    rng = np.random.default_rng(0)
    assert len(vr.tr_rot_vectors(rng.standard_normal((5, 3)), None, periodic=True)) == 3
    assert len(vr.tr_rot_vectors(rng.standard_normal((5, 3)), None)) == 6


@pytest.mark.parametrize('M', [63, 126])
def test_synthetic_spectra_are_deterministic_and_the_yardstick_recovers_them(M):
    """tests/test_hip_eig_spectra.py: the generators give the same arrays on every call, their fp32 form is the fp64 one rounded
    once, and the yardstick returns the planted eigenvalues to 1e-12 s from the fp64 matrix"""
    a, b = vr.hard_spectra(M), vr.hard_spectra(M)
    assert list(a) == list(b) and len(a) == 9
    pos = np.zeros((M // 3, 3))
    for name, (lam, A64, A32) in a.items():
        assert np.array_equal(A64, b[name][1]) and np.array_equal(A32, A64.astype(np.float32)) and np.array_equal(A64, A64.T)
        assert A32.shape == (M, M) and A32.dtype == np.float32 and np.all(np.isfinite(A32))
        if lam is None:
            continue
        got = vr.analyse(A64, pos, None, project=False)
        assert np.abs(got['evals'] - lam).max() <= 1e-12 * got['s'], name
    assert np.count_nonzero(a['cluster'][0] == 1.0) == M - 3 and np.all(np.bincount(np.unique(a['triples'][0], return_inverse=True)[1]) == 3)
    T = a['tiny_coupling'][2]
    assert np.all(np.abs(T[0::2, 1::2].diagonal()) < 1e-29) and np.all(T[0::2, 1::2].diagonal() > 0)      # normal fp32 numbers, not 0
    mixed = a['tiny_and_plain_coupling'][2][0::2, 1::2].diagonal()
    assert np.all(mixed[0::2] < 1e-29) and np.all(mixed[1::2] >= 0.5)
    rng1, rng2 = np.random.default_rng(42), np.random.default_rng(42)
    assert np.array_equal(vr.random_symmetric(7, rng1), vr.random_symmetric(7, rng2))


def test_drop_rule_molecules_give_the_stated_counts_in_the_yardstick():
    """tests/test_hip_eig_spectra.py::test_projection_drop_rule: 5 for the collinear molecules (not along an axis) and for a bend of
    1e-7 of the length, 6 for a bend of 1e-3 and for the planar molecule, 3 for all of them in a periodic cell; the remainder of
    the dropped or kept sixth vector is a decade or more away from DROP_TOL"""
    mols = vr.drop_rule_molecules()
    assert [n for _, _, n in mols] == [5, 5, 6, 5, 5, 6, 6] and [p.shape[0] for _, p, _ in mols] == [3, 3, 3, 4, 4, 4, 4]
    for name, pos, n_proj in mols:
        assert pos.dtype == np.float32
        m = np.array(([15.999, 1.008] * 2)[:pos.shape[0]])
        for masses in (None, m):
            assert len(vr.tr_rot_vectors(pos, masses)) == n_proj, name
            assert len(vr.tr_rot_vectors(pos, masses, periodic=True)) == 3, name
            # the same count with the rule a decade tighter and a decade looser: the cases are not on its edge
            keep = vr.DROP_TOL
            try:
                for tol in (keep / 10, keep * 10):
                    vr.DROP_TOL = tol
                    assert len(vr.tr_rot_vectors(pos, masses)) == n_proj, (name, tol)
            finally:
                vr.DROP_TOL = keep
        A = vr.gapped_symmetric(pos.shape[0], np.random.default_rng(1), m)
        for periodic, want in ((False, n_proj), (True, 3)):
            got = vr.analyse(A, pos, m, project=True, periodic=periodic)
            small = np.sort(np.abs(got['evals']))
            assert got['n_proj'] == want and np.count_nonzero(small <= 1e-12 * got['s']) == want
            assert small[want] >= 0.1 * got['s']                     # the gap the projected-zero count of check_solver needs


@pytest.mark.parametrize('mixed_masses', [False, True])
def test_every_size_batch_keeps_its_spectra_away_from_zero(mixed_masses):
    """tests/test_hip_eig_spectra.py::test_every_size_in_one_launch_and_in_any_order: deterministic, every size 1 .. 42, and after
    the projection the smallest genuine |eigenvalue| of every molecule is at least 0.1 s -- the solver bound is 1e-4 s at most, so
    the count of eigenvalues inside it is the count of projected vectors and nothing else"""
    sizes, mats, poss, masses = vr.every_size_batch(mixed_masses)
    again = vr.every_size_batch(mixed_masses)
    assert sizes == list(range(1, 43))
    for n, A, p, m, B in zip(sizes, mats, poss, masses, again[1]):
        assert A.shape == (3 * n, 3 * n) and A.dtype == np.float32 and np.array_equal(A, B) and np.array_equal(A, A.T)
        if mixed_masses:
            assert m.dtype == np.float32 and set(np.unique(m)) <= {np.float32(1.008), np.float32(126.90)}
        got = vr.analyse(A, p.astype(np.float32), m, project=True)
        want = 3 if n == 1 else 5 if n == 2 else 6
        assert got['n_proj'] == want
        small = np.sort(np.abs(got['evals']))
        if 3 * n > want:
            assert vr.solver_bound(3 * n, got['s']) <= 1e-4 * got['s'] and small[want] >= 0.1 * got['s'], n
            assert np.count_nonzero(small <= 1e-12 * got['s']) == want
        free = vr.analyse(A, p, m, project=False)
        assert np.abs(free['evals']).min() >= 0.1 * free['s']
