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
