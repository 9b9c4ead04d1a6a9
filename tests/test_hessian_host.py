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


def test_replica_arithmetic_of_the_sixteen_aspirins():
    """tests/test_hip_hessian_forms.py: 16 aspirins are 336 atoms and 63 directions -> 48 replicas, two passes, the second with 15
    live directions; mixed_rand at R = 5 runs 13 passes, the last with 3"""
    from newtonnet_amd import hessian as nh
    z, pos, cell, batch = hr.jittered_aspirins(16, seed=16)
    assert pos.shape == (336, 3) and pos.dtype == torch.float32 and cell.shape == (16, 3, 3) and batch.tolist() == sorted(batch.tolist())
    assert torch.equal(torch.bincount(batch), torch.full((16,), 21))
    assert nh.replicas_for(336, 63) == 48 and 48 * 336 <= nh.REPLICA_ATOM_BUDGET < 49 * 336
    assert hr.pass_count(63, 48) == (2, 15) and hr.pass_count(63, 5) == (13, 3) and hr.pass_count(63, 63) == (1, 63)
    assert nh.replicas_for(33, 63) == 63                      # mixed_rand: one replica per direction
    again = hr.jittered_aspirins(16, seed=16)
    assert torch.equal(again[1], pos)
    # copies differ (the jitter) and sit 20 A apart: no fp32 coordinate above 60 A
    assert not torch.equal(pos[:21] - pos[0], pos[21:42] - pos[21]) and pos.abs().max().item() < 60.0
    z7, p7, _, b7 = hr.jittered_aspirins(700, seed=700)
    assert p7.shape == (14700, 3) and p7.abs().max().item() < 200.0 and int(b7.max()) == 699


def test_short_and_long_pair_geometry_and_the_per_molecule_oracle():
    z, pos, cell, batch = hr.short_and_long_pairs()
    d = (pos[:, None] - pos[None]).norm(dim=-1)
    assert abs(d[0, 1].item() - 0.7) < 1e-6 and 4.9985 < d[0, 2].item() < 5.0
    assert (d + 9 * torch.eye(6)).min().item() >= 0.7 - 1e-6
    # every molecule alone, on a thread pool, with another envelope: equal to the whole batch through the oracle
    sd = util.load_state('rand')
    z, pos, cell, batch = hr.ethanol_and_aspirin()
    keep = batch == 0
    z2, p2, c2, b2 = hr.short_and_long_pairs()
    z, pos, cell, batch = torch.cat([z[keep], z2]), torch.cat([pos[keep], p2]), torch.zeros(2, 3, 3), torch.cat([batch[keep], b2 + 1])
    whole = hr.oracle_hessian(sd, z, pos, cell, batch, envelope=('polynomial', 2))
    parts = hr.dense_from_blocks(hr.oracle_hessian_per_molecule(sd, z, pos, cell, batch, envelope=('polynomial', 2), workers=2), batch)
    assert (whole - parts).abs().max().item() <= 1e-12 * whole.abs().max().item()
    default = hr.oracle_hessian(sd, z, pos, cell, batch)
    assert (whole - default).abs().max().item() > 1e-3 * whole.abs().max().item()        # the envelope reached the oracle
    from oracle import newtonnet_ref as ref
    x = torch.tensor([0.3], dtype=torch.float64)
    assert torch.equal(ref._envelope(x), ref.poly_envelope(x, 9)) and ref._act is torch.nn.functional.silu   # ... and was put back


def test_relu_model_of_the_activation_tests_has_no_pre_activation_near_zero():
    """tests/test_hip_hessian_forms.py::test_other_activations[relu]: the Hessian of a relu model depends on the branch of every
    hidden unit, and the fp32 device and the fp64 oracle can take different branches only where a pre-activation is within the
    fp32 error of 0.  That error is relative to the unit's ROW (h[r] = W x[r]), so the condition is  |h[r][f]| >= 1e-5 max_f
    |h[r][f]|  for every row of every hidden layer, in the fp64 oracle: 24 of the seeds 0 .. 599 meet it, hr.RELU_SEED = 152
    with 2.3e-5.  The same margin against the LAYER's largest pre-activation cannot be met by any weights: the pair rows of the
    edge MLPs carry the cutoff envelope of their pair, so about 2 % of them are below 1e-5 of the layer's maximum whatever
    the seed (best of 600 seeds: 2.3e-9)."""
    from newtonnet_amd.models import NewtonNet
    z, pos, cell, batch = hr.ethanol_and_aspirin()
    assert torch.bincount(batch).tolist() == [9, 21]
    torch.manual_seed(hr.RELU_SEED)
    model = NewtonNet(activation='relu', output_properties=['energy', 'gradient_force'])
    sd = {k: v.detach().double() for k, v in model.state_dict().items()}
    rows, layers, calls = hr.preactivation_margin(sd, z, pos, cell, batch, 'relu')
    print(f'relu seed {hr.RELU_SEED}: row margin {rows:.3e}, layer margin {layers:.3e}, {calls} hidden layers')
    assert calls == 3 * 3 + 2 and rows >= 1e-5
