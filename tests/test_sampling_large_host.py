"""CPU-side checks of the tiled sampling kernel (csrc/sample_large.hip): the C ABI exports it next to the unchanged LDS kernel, its
bound is the blocked eigensolver's, and the `kernel` / `solver` keywords of every entry that samples are validated before anything
touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_sampling_host import host_modes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('nnhip_mode_sample_large_max_dim', 'nnhip_mode_sample_large')


def library():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip, ctypes.CDLL(hip.LIB_PATH)


def test_tiled_kernel_symbols_are_declared_listed_and_exported():
    hip, lib = library()
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for sym in NEW_SYMBOLS:
        assert sym in declared, f'{sym} is not declared in the header'
        assert sym in hip.EXPORTED_SYMBOLS, f'{sym} is not listed in EXPORTED_SYMBOLS'
        assert hasattr(lib, sym), f'{sym} is not exported'
    assert lib.nnhip_version() >= 113


def test_bound_is_the_blocked_solvers():
    from newtonnet_amd import vibrations as vib
    _, lib = library()
    lib.nnhip_mode_sample_large_max_dim.restype = ctypes.c_int
    lib.nnhip_eig_large_max_dim.restype = ctypes.c_int
    assert lib.nnhip_mode_sample_large_max_dim() == lib.nnhip_eig_large_max_dim() == 1536
    assert vib.max_dim_sample_large() == lib.nnhip_mode_sample_large_max_dim() == vib.max_dim_large()


def test_library_validates_before_any_launch():
    """the checks that come before the first launch need no device: the pointers are never followed"""
    hip, _ = library()
    L = hip.lib()
    bound = L.nnhip_mode_sample_large_max_dim()
    n = bound // 3 + 1
    fake = 4096                                                     # a non-null address that is never read

    def call(offsets, n_samples=1, T=300.0, amp=fake, min_dim=0, dev_ptr=fake):
        host = torch.tensor(offsets, dtype=torch.int32)
        return L.nnhip_mode_sample_large(fake, fake, fake, dev_ptr, host.data_ptr(), len(offsets) - 1, None, fake, fake, T, 0,
                                         n_samples, fake, fake, fake, amp, fake, min_dim, None)
    assert call([0, 3, 3 + n]) == 2                                 # NNHIP_E_UNSUPPORTED
    msg = L.nnhip_last_error().decode()
    assert str(bound) in msg and 'molecule 1' in msg
    assert call([0, n, n + 3], min_dim=3 * n + 1) == 0              # min_dim does not select the molecule above the bound: nothing to do
    assert call([0, 3, 45], min_dim=136) == 0                       # nothing selected
    assert call([0, 0, 0]) == 0 and call([0, 43], n_samples=0) == 0
    assert call([0, 43], amp=None) == 1                             # NNHIP_E_INVALID
    assert 'amplitudes' in L.nnhip_last_error().decode()
    assert call([0, 5, 3]) == 1 and 'decreases at molecule 1' in L.nnhip_last_error().decode()
    for T in (-1.0, float('nan'), float('inf')):
        assert call([0, 43], T=T) == 1
    assert call([0, 43], n_samples=-1) == 1 and call([0, 43], dev_ptr=None) == 1
    assert call([0, 43], n_samples=65535 * 32 + 1) == 2 and str(65535 * 32) in L.nnhip_last_error().decode()


def test_unknown_kernel_or_solver_is_refused_before_the_device_check():
    nm = host_modes()
    with pytest.raises(ValueError, match="'lds', 'auto', 'tiled'"):
        nm.sample(1, 300.0, kernel='nope')
    with pytest.raises(ValueError, match="'lds', 'auto', 'tiled'"):
        nm.sample(0, float('nan'), kernel='blocked')                # (the solver's word is not the kernel's) before every other check
    for ok in ('lds', 'auto', 'tiled'):                             # a known value gets as far as the device check
        with pytest.raises(RuntimeError, match='MI355X'):
            nm.sample(2, 300.0, xi=torch.zeros(18), kernel=ok)
    from newtonnet_amd.models import NewtonNet
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.eval()
    z, pos, cell, batch = torch.ones(1, dtype=torch.long), torch.zeros(1, 3), torch.zeros(1, 3, 3), torch.zeros(1, dtype=torch.long)
    with pytest.raises(ValueError, match="'lds', 'auto', 'blocked'"):
        model.sample_displacements(z, pos, cell, batch, 1, 300.0, solver='nope')
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype, calc.model = torch.device('cpu'), torch.float32, model
    atoms = FakeAtoms([8, 1, 1], np.random.default_rng(0).random((3, 3)))
    with pytest.raises(ValueError, match="'lds', 'auto', 'blocked'"):
        calc.sample(atoms, 1, 300.0, solver='nope')
    for ok in ('lds', 'auto', 'blocked'):
        with pytest.raises(RuntimeError, match='MI355X'):
            model.sample_displacements(z, pos, cell, batch, 1, 300.0, solver=ok)
        with pytest.raises(RuntimeError, match='MI355X'):
            calc.sample(atoms, 1, 300.0, solver=ok)
