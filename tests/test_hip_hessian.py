"""Analytic Hessians / Hessian-vector products on the HIP path (newtonnet_amd/hessian.py, csrc/hessian.hip) against the fp64
double-backward Hessian of the pinned oracle (tests/hessian_ref.py: the math of the reference's HessianOutput,
newtonnet/models/output.py:134-152).

Tolerances per molecule block, relative to max |H| of the block: max |dH| <= 1e-4, mean |dH| <= 1e-5."""
import numpy as np
import pytest
import torch

from tests import hessian_ref as hr
from tests import util

pytestmark = pytest.mark.gpu


def make_model(sd, props=('energy', 'gradient_force'), **kw):
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=list(props), **kw)
    missing = model.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys
    model = model.to('cuda')
    model.eval()
    return model


def cuda(*ts):
    return [t.cuda() for t in ts]


def check_blocks(H, H_ref, batch):
    """per-molecule tolerance, exact zeros between molecules"""
    H, H_ref = H.detach().cpu().double(), H_ref.double()
    b = batch.cpu()
    n = b.numel()
    same = (b[:, None] == b[None, :])
    off = H.permute(0, 2, 1, 3)[~same]
    assert torch.count_nonzero(off) == 0, 'non-zero entries between molecules'
    for m in torch.unique(b).tolist():
        idx = (b == m).nonzero().reshape(-1)
        hb, rb = H[idx][:, :, idx], H_ref[idx][:, :, idx]
        scale = rb.abs().max().item()
        d = (hb - rb).abs()
        if scale == 0:
            assert d.max().item() == 0
            continue
        assert d.max().item() <= 1e-4 * scale, f'molecule {m}: max |dH| {d.max().item():.3e} of {scale:.3e}'
        assert d.mean().item() <= 1e-5 * scale, f'molecule {m}: mean |dH| {d.mean().item():.3e} of {scale:.3e}'
    assert n == H.shape[0]


def block_errors(H, H_ref, batch):
    """{m: (max |dH|, mean |dH|, max |H_ref|)} per molecule, for printing next to check_blocks"""
    H, H_ref = H.detach().cpu().double(), H_ref.double()
    b = batch.cpu()
    out = {}
    for m in torch.unique(b).tolist():
        idx = (b == m).nonzero().reshape(-1)
        d = (H[idx][:, :, idx] - H_ref[idx][:, :, idx]).abs()
        out[m] = (d.max().item(), d.mean().item(), H_ref[idx][:, :, idx].abs().max().item())
    return out


def mol_subset(z, pos, cell, batch, mols):
    keep = torch.isin(batch, torch.tensor(mols))
    remap = {m: k for k, m in enumerate(mols)}
    return z[keep], pos[keep], cell[list(mols)], torch.tensor([remap[int(b)] for b in batch[keep]])


@pytest.mark.parametrize('case', ['aspirin1_ckpt', 'ethanol4_rand', 'mixed_rand'])
def test_dense_hessian_against_the_oracle(case):
    which = case.split('_')[-1]
    sd = util.load_state(which)
    z, pos, cell, batch, _ = util.case_inputs(case, torch.float32)
    model = make_model(sd)
    H = model.hessian(*cuda(z, pos, cell, batch))
    assert H.shape == (pos.shape[0], 3, pos.shape[0], 3) and H.dtype == torch.float32
    H_ref = hr.oracle_hessian(sd, z, pos.double(), cell.double(), batch)
    check_blocks(H, H_ref, batch)
    # fp32 result is not symmetrised (as the reference); it is symmetric to rounding
    Hm = H.reshape(3 * pos.shape[0], -1)
    assert (Hm - Hm.T).abs().max().item() <= 1e-4 * Hm.abs().max().item()


def test_one_and_two_atom_molecules():
    """a zero-edge molecule (its block is exactly 0) and a two-atom molecule next to an ethanol"""
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand', torch.float32)
    z, pos, cell, batch = mol_subset(z, pos, cell, batch, [0])
    z = torch.cat([z, torch.tensor([8, 1, 1])])
    pos = torch.cat([pos, torch.tensor([[30.0, 0.0, 0.0], [-30.0, 0.0, 0.0], [-30.0, 0.0, 0.74]])])
    cell = torch.zeros(3, 3, 3)
    batch = torch.cat([batch, torch.tensor([1, 2, 2])])
    model = make_model(sd)
    H = model.hessian(*cuda(z, pos, cell, batch))
    assert torch.count_nonzero(H[9, :, 9, :]) == 0
    check_blocks(H, hr.oracle_hessian(sd, z, pos.double(), cell.double(), batch), batch)
    assert H[10:, :, 10:, :].abs().max() > 0


def test_layer_norm_and_cosine_envelope():
    from newtonnet_amd.layers import CosineCutoff
    c = util.load_npz('case_layernorm.npz')
    sd = {k[3:]: torch.from_numpy(v) for k, v in c.items() if k.startswith('sd.')}
    z, pos, cell, batch = (torch.from_numpy(c[k]) for k in ('z', 'pos', 'cell', 'batch'))
    z, pos, cell, batch = mol_subset(z.long(), pos.float(), cell.float(), batch.long(), [0, 1])
    model = make_model(sd, layer_norm=True)
    check_blocks(model.hessian(*cuda(z, pos, cell, batch)), hr.oracle_hessian(sd, z, pos.double(), cell.double(), batch), batch)

    c = util.load_npz('case_envelope.npz')
    z, batch = torch.from_numpy(c['z']).long(), torch.from_numpy(c['batch']).long()
    pos, cell = torch.from_numpy(c['pos']).float(), torch.from_numpy(c['cell']).float()
    z, pos, cell, batch = mol_subset(z, pos, cell, batch, [0, 1])
    sd = util.load_state('rand')
    model = make_model(sd)
    model.embedding_layers.edge_embedding.envelope = CosineCutoff()
    H = model.hessian(*cuda(z, pos, cell, batch))
    check_blocks(H, hr.oracle_hessian(sd, z, pos.double(), cell.double(), batch, envelope='cosine'), batch)


def test_periodic_batch_columns():
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('pbc_batch2_rand', torch.float32)
    model = make_model(sd)
    blocks, ptr = model.hessian(*cuda(z, pos, cell, batch), blocks=True)
    rng = np.random.default_rng(3)
    n0 = int((batch == 0).sum())
    cols = np.sort(rng.choice(3 * pos.shape[0], 24, replace=False))
    ref = hr.oracle_hessian_columns(sd, z, pos.double(), cell.double(), batch, cols)   # [24, N, 3]
    H = blocks.cpu().double()
    for k, col in enumerate(cols.tolist()):
        a = col // 3
        b = 0 if a < n0 else 1
        s, n = (0, n0) if b == 0 else (n0, pos.shape[0] - n0)
        blk = H[ptr[b].item():ptr[b].item() + 9 * n * n].view(n, 3, n, 3)
        got = blk[:, :, a - s, col % 3]
        want = ref[k][s:s + n]
        scale = want.abs().max().item()
        assert (got - want).abs().max().item() <= 1e-4 * scale, (col, (got - want).abs().max().item(), scale)
        other = ref[k][n0:] if b == 0 else ref[k][:n0]
        assert other.abs().max().item() == 0


def test_hessian_vector_product():
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('mixed_rand', torch.float32)
    model = make_model(sd)
    g = torch.Generator().manual_seed(7)
    v = torch.randn(pos.shape[0], 3, generator=g)
    hv = model.hessian_vector_product(*cuda(z, pos, cell, batch), v.cuda())
    H_ref = hr.oracle_hessian(sd, z, pos.double(), cell.double(), batch)
    want = (H_ref.reshape(3 * pos.shape[0], -1) @ v.double().reshape(-1)).reshape(-1, 3)
    d = (hv.cpu().double() - want).abs()
    assert d.max().item() <= 1e-4 * want.abs().max().item() * 3, (d.max().item(), want.abs().max().item())
    # linear in v, and the same pass as a column of the Hessian
    H = model.hessian(*cuda(z, pos, cell, batch))
    e = torch.zeros_like(v)
    e[5, 1] = 1.0
    col = model.hessian_vector_product(*cuda(z, pos, cell, batch), e.cuda())
    torch.testing.assert_close(col, H[:, :, 5, 1], rtol=0, atol=1e-6 * H.abs().max().item())


def test_replicas_and_direction_loop_agree_and_repeat_bitwise():
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand', torch.float32)
    model = make_model(sd)
    args = cuda(z, pos, cell, batch)
    from newtonnet_amd import hessian as nh
    b_rep, p_rep = nh.hessian_blocks(model, *args)
    b_one, p_one = nh.hessian_blocks(model, *args, replicas=1)
    assert torch.equal(p_rep, p_one)
    torch.testing.assert_close(b_rep, b_one, rtol=0, atol=1e-5 * b_one.abs().max().item())
    b_again, _ = nh.hessian_blocks(model, *args)
    assert torch.equal(b_again, b_rep)
    blocks, ptr = model.hessian(*args, blocks=True)
    H = model.hessian(*args)
    assert torch.equal(H, nh.blocks_to_dense(blocks, ptr, batch.cuda(), pos.shape[0]))
    assert torch.equal(model.hessian(*args), H)


def test_forward_unchanged_and_weight_change_picked_up():
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('aspirin1_rand', torch.float32)
    model = make_model(sd)
    args = cuda(z, pos, cell, batch)
    o1 = model(*args)
    e1, f1 = o1.energy.clone(), o1.gradient_force.clone()
    H1 = model.hessian(*args)
    o2 = model(*args)
    assert torch.equal(o2.energy, e1) and torch.equal(o2.gradient_force, f1)
    with torch.no_grad():
        model.interaction_layers[1].message_edgepart.weight.mul_(1.5)
    H2 = model.hessian(*args)
    assert not torch.equal(H1, H2)
    sd2 = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    check_blocks(H2, hr.oracle_hessian(sd2, z, pos.double(), cell.double(), batch), batch)


def test_train_mode_and_missing_energy_head_raise():
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('aspirin1_rand', torch.float32)
    model = make_model(sd)
    args = cuda(z, pos, cell, batch)
    model.train()
    with pytest.raises(NotImplementedError, match='eval'):
        model.hessian(*args)
    with pytest.raises(NotImplementedError, match='eval'):
        model.hessian_vector_product(*args, torch.zeros_like(args[1]))
    from newtonnet_amd.models import NewtonNet
    m2 = NewtonNet(output_properties=['direct_force']).cuda()
    m2.eval()
    with pytest.raises(NotImplementedError, match='energy'):
        m2.hessian(*args)


def test_calculator_hessian_one_and_three_frames():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    z, pos, cell, batch, _ = util.case_inputs('aspirin8_rand', torch.float32)
    sd = util.load_state('rand', torch.float32)
    calc = MLAseCalculator(sd, properties=['energy', 'forces', 'hessian'], device='cuda')
    frames = [FakeAtoms(z[batch == b].numpy(), pos[batch == b].numpy().astype(np.float64)) for b in range(3)]
    calc.calculate(frames[0])
    h1 = calc.results['hessian']
    assert h1.shape == (21, 3, 21, 3) and h1.dtype == np.float32
    calc.calculate(frames)
    h3 = calc.results['hessian']
    assert h3.shape == (3, 21, 3, 21, 3)
    zz, pp, cc, bb = calc.format_data(frames)
    H = calc.model.hessian(zz, pp, cc, bb).cpu().numpy()
    for b in range(3):
        np.testing.assert_array_equal(h3[b], H[21 * b:21 * (b + 1), :, 21 * b:21 * (b + 1), :])
    np.testing.assert_allclose(h1, h3[0], rtol=0, atol=1e-5 * np.abs(h1).max())
