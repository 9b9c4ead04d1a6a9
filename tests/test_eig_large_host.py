"""CPU-side checks of the blocked eigensolver (csrc/eig_large.hip): the C ABI exports it next to the unchanged one-workgroup
solver, the workspace size behaves, and the `solver` keyword is validated before anything touches a device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('nnhip_eig_large_max_dim', 'nnhip_eig_large_ws_bytes', 'nnhip_eig_blocks_large')


def library():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip, ctypes.CDLL(hip.LIB_PATH)


def test_blocked_solver_symbols_are_declared_listed_and_exported():
    hip, lib = library()
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for sym in NEW_SYMBOLS:
        assert sym in declared, f'{sym} is not declared in the header'
        assert sym in hip.EXPORTED_SYMBOLS, f'{sym} is not listed in EXPORTED_SYMBOLS'
        assert hasattr(lib, sym), f'{sym} is not exported'
    assert lib.nnhip_version() >= 112


def test_bounds_of_the_two_solvers():
    from newtonnet_amd import vibrations as vib
    _, lib = library()
    lib.nnhip_eig_large_max_dim.restype = ctypes.c_int
    lib.nnhip_eig_max_dim.restype = ctypes.c_int
    assert lib.nnhip_eig_large_max_dim() >= 1536
    assert lib.nnhip_eig_max_dim() == 126
    assert vib.max_dim_large() == lib.nnhip_eig_large_max_dim() and vib.max_dim() == 126


def test_workspace_size():
    hip, _ = library()
    L = hip.lib()
    one = torch.tensor([0, 43], dtype=torch.int32)
    without, with_modes = (int(L.nnhip_eig_large_ws_bytes(one.data_ptr(), 1, m)) for m in (0, 1))
    # M = 129 pads to 192: A alone is 4 x 192^2 bytes, the eigenvectors take the same again
    assert without >= 4 * 192 * 192 and with_modes >= without + 4 * 192 * 192
    assert with_modes <= 4 * without
    two = torch.tensor([0, 43, 86], dtype=torch.int32)
    assert int(L.nnhip_eig_large_ws_bytes(two.data_ptr(), 2, 1)) > with_modes
    # a molecule without atoms takes nothing; one above the bound has no size
    assert int(L.nnhip_eig_large_ws_bytes(torch.tensor([0, 43, 43], dtype=torch.int32).data_ptr(), 2, 1)) == with_modes
    n = L.nnhip_eig_large_max_dim() // 3 + 1
    assert int(L.nnhip_eig_large_ws_bytes(torch.tensor([0, n], dtype=torch.int32).data_ptr(), 1, 1)) == 0


def test_unknown_solver_is_refused_before_the_device_check():
    from newtonnet_amd import vibrations as vib
    host = (torch.zeros(9), torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long), torch.zeros(1, 3), torch.zeros(1, 3, 3))
    with pytest.raises(ValueError, match="'lds', 'auto', 'blocked'"):
        vib.eig_blocks(*host, solver='nope')
    for ok in ('lds', 'auto', 'blocked'):                 # a known value gets as far as the device check
        with pytest.raises(RuntimeError, match='cuda'):
            vib.eig_blocks(*host, solver=ok)
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.eval()
    z, pos, cell, batch = torch.ones(1, dtype=torch.long), torch.zeros(1, 3), torch.zeros(1, 3, 3), torch.zeros(1, dtype=torch.long)
    with pytest.raises(ValueError, match="'lds', 'auto', 'blocked'"):
        model.normal_modes(z, pos, cell, batch, solver='nope')
    with pytest.raises(ValueError, match="'lds', 'auto', 'blocked'"):
        model.frequencies(z, pos, cell, batch, solver='nope')
