"""CPU-side checks of the Hessian feature: C ABI and ctypes mirror, calculator wiring, the fp64 yardstick of the GPU tests."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import hessian_ref as hr
from tests import util


def test_library_exports_the_hessian_entry_points_and_the_mirror_matches_the_header():
    from newtonnet_amd import hip
    lib = hip.lib()
    assert lib.nnhip_version() >= 109
    for name in ('nnhip_hessian_vp', 'nnhip_hessian_blocks', 'nnhip_hvp_ws_bytes'):
        assert name in hip.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert C.sizeof(hip.HvpWs) == lib.nnhip_hvp_ws_bytes()
    hdr = open(hip.os.path.join(hip.os.path.dirname(hip.__file__), '..', 'include', 'newtonnet_hip.h')).read()
    end = hdr.index('} nnhip_hvp_ws;')
    body = hdr[hdr.rindex('typedef struct {', 0, end) + len('typedef struct {'):end]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'(\w+)\s*[,;]', body)
    assert names == [n for n, _ in hip.HvpWs._fields_]


def test_calculator_lists_hessian_and_the_output_head_still_raises():
    from newtonnet_amd.models.output import get_output_by_string
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    assert 'hessian' in MLAseCalculator.implemented_properties
    with pytest.raises(NotImplementedError):
        get_output_by_string('hessian')
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype, calc.properties = torch.device('cpu'), torch.float32, ['energy', 'forces', 'hessian']
    model = calc.load_model(util.load_state('ckpt', torch.float32))
    assert model.output_properties == ['energy', 'gradient_force']


def test_reference_module_with_a_hessian_head_loads(tmp_path):
    """a whole-module pickle of the reference with a HessianOutput head (no parameters): the head is dropped, 'hessian' is
    served by the method and properties=None includes it"""
    from newtonnet_amd.models import NewtonNet
    from newtonnet_amd.utils import ase_interface
    from tests.test_ase_calculator import _save_fake_reference_pickle
    sd = util.load_state('ckpt', torch.float32)
    path = str(tmp_path / 'best_model.pt')
    _save_fake_reference_pickle(path, sd, False)
    obj = torch.load(path, map_location='cpu', weights_only=False, pickle_module=ase_interface._ReferencePickle)
    obj.output_properties = ['energy', 'gradient_force', 'hessian']
    obj.output_layers.append(torch.nn.Module())
    obj.scalers.append(torch.nn.Module())
    calc = ase_interface.MLAseCalculator.__new__(ase_interface.MLAseCalculator)
    calc.device, calc.dtype, calc.properties = torch.device('cpu'), torch.float32, None
    model = calc.load_model(obj)
    assert isinstance(model, NewtonNet) and model.output_properties == ['energy', 'gradient_force']
    assert calc.properties == ['energy', 'forces', 'hessian']


def test_oracle_hessian_is_symmetric_and_matches_force_differences():
    """the yardstick of tests/test_hip_hessian.py: fp64 double backward of the oracle energy, symmetric to 1e-12 and equal to
    central differences of the oracle's forces"""
    from oracle import newtonnet_ref as ref
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand', torch.float64)
    keep = batch < 2
    z, pos, batch, cell = z[keep], pos[keep], batch[keep], cell[:2]
    H = hr.oracle_hessian(sd, z, pos, cell, batch)
    n = pos.shape[0]
    Hm = H.reshape(3 * n, 3 * n)
    assert (Hm - Hm.T).abs().max().item() <= 1e-12 * Hm.abs().max().item()
    assert Hm[:27, 27:].abs().max().item() == 0          # no coupling between molecules
    eps = 1e-5
    for k in (0, 13, 40):
        e = torch.zeros(3 * n, dtype=torch.float64)
        e[k] = eps
        fp = ref.energy_forces(sd, z, pos + e.view(n, 3), cell, batch)['forces'].reshape(-1)
        fm = ref.energy_forces(sd, z, pos - e.view(n, 3), cell, batch)['forces'].reshape(-1)
        fd = -(fp - fm) / (2 * eps)
        assert (fd - Hm[:, k]).abs().max().item() <= 1e-6 * Hm.abs().max().item()
