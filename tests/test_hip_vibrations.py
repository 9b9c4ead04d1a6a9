"""Batched normal-mode analysis on the HIP path (newtonnet_amd/vibrations.py, csrc/eig.hip).

Solver alone: the device's own fp32 Hessian blocks are copied to the host and the fp64 yardstick (tests/vib_ref.py) runs ON THOSE
SAME BLOCKS with the same masses and projection, so the Hessian's error does not enter.  Per molecule, with M = 3 n_b,
s = ||A||_2 from the yardstick, eps32 = 2^-24 and c = 8 (vib_ref.C_SOLVER; the backward-error form of Jacobi's method):
    max_k |lambda_k - lambda_k_ref| <= c M eps32 s,   max |A v_k - lambda_k v_k| <= c M eps32 s,   max |V V^T - I| <= c M eps32.
Modes are never compared entry by entry (near-degenerate pairs rotate freely).

End to end: model.normal_modes against the yardstick on the fp64 oracle Hessian, with the Weyl bound
    B = ||A_dev - A_oracle||_2 + c M eps32 s
on eigenvalues and 521.47 B / sqrt(|lambda_oracle|) on the frequencies of the modes with |lambda_oracle| > 2 B.

The fixture pbc_batch2_rand holds molecules of 216 and 125 atoms (M = 648 and 375): a 648 x 648 fp32 matrix is 1.6 MB, ten times
the LDS of a CU, so the one-workgroup solver cannot serve it at any bound.  For that case the test holds the solver to the
documented refusal (NotImplementedError naming the bound, before any launch); the periodic projection rule (three translations)
is checked on two ethanols placed in a periodic box instead."""
import numpy as np
import pytest
import torch

from tests import hessian_ref as hr
from tests import util
from tests import vib_ref as vr
from tests.test_hip_hessian import cuda, make_model, mol_subset

pytestmark = pytest.mark.gpu


def table(z):
    """the package's table values as the device sees them (fp32)"""
    from newtonnet_amd import vibrations as vib
    return vib.table_masses(z)


def periodic_ethanols():
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand', torch.float32)
    z, pos, cell, batch = mol_subset(z, pos, cell, batch, [0, 1])
    cell = torch.eye(3).repeat(2, 1, 1) * torch.tensor([16.0, 17.0])[:, None, None]
    pos = pos - pos.min(0).values + 1.0                      # inside both boxes
    return z, pos, cell, batch


def solver_inputs(case):
    if case == 'periodic_ethanol2_rand':
        sd = util.load_state('rand')
        return (sd,) + periodic_ethanols()
    sd = util.load_state(case.split('_')[-1])
    z, pos, cell, batch, _ = util.case_inputs(case, torch.float32)
    return sd, z, pos, cell, batch


def molecules(batch):
    b = batch.cpu()
    for m in range(int(b.max()) + 1):
        idx = (b == m).nonzero().reshape(-1)
        if idx.numel():                                       # (an empty molecule slot owns nothing to check)
            yield m, idx


def check_solver(nm, blocks_host, ptr_host, z, pos, cell, batch, masses, project, label):
    """the bounds of the module docstring for every molecule; returns the observed constants"""
    worst = dict(evals=0.0, resid=0.0, orth=0.0)
    lam_all = nm.eigenvalues.cpu().double().numpy()
    for m, idx in molecules(batch):
        n = idx.numel()
        M = 3 * n
        Hb = blocks_host[ptr_host[m]:ptr_host[m] + 9 * n * n].reshape(M, M)
        mm = None if masses is None else masses[idx].double().numpy()
        periodic = bool(cell[m].abs().max() > 0)
        ref = vr.analyse(Hb, pos[idx].double().numpy(), mm, project=project, periodic=periodic)
        s, bound = ref['s'], vr.solver_bound(M, ref['s'])
        freq, modes = nm.molecule(m)
        lam = lam_all[3 * idx[0].item():3 * idx[0].item() + M]
        V = modes.cpu().double().numpy().reshape(M, M)
        assert int(nm.status[m]) == 0, f'{label} molecule {m}: sweep cap hit ({int(nm.sweeps[m])} sweeps)'
        assert int(nm.n_projected[m]) == ref['n_proj']
        assert np.all(np.diff(lam) >= 0), 'eigenvalues are not ascending'
        # sign convention: the component of largest magnitude (lowest index on a tie) is positive
        V32 = modes.cpu().numpy().reshape(M, M)
        k = np.argmax(np.abs(V32), axis=1)
        assert np.all(V32[np.arange(M), k] > 0)
        orth = np.abs(V @ V.T - np.eye(M)).max()
        c_orth = orth / (M * vr.EPS32)
        assert orth <= vr.C_SOLVER * M * vr.EPS32, f'{label} molecule {m}: orthonormality c = {c_orth:.2f}'
        worst['orth'] = max(worst['orth'], c_orth)
        if s == 0:
            assert np.count_nonzero(lam) == 0 and np.count_nonzero(freq.cpu().numpy()) == 0
            print(f'{label} molecule {m} (M = {M}): zero block, n_projected {ref["n_proj"]}')
            continue
        d_ev = np.abs(lam - ref['evals']).max()
        resid = np.abs(ref['A'] @ V.T - V.T * lam[None, :]).max()
        c_ev, c_res = d_ev / (M * vr.EPS32 * s), resid / (M * vr.EPS32 * s)
        print(f'{label} molecule {m} (M = {M}, project {project}): sweeps {int(nm.sweeps[m])}, c eigenvalues {c_ev:.3f}, '
              f'c residual {c_res:.3f}, c orthonormality {c_orth:.3f}')
        assert d_ev <= bound, f'{label} molecule {m}: eigenvalues c = {c_ev:.2f}'
        assert resid <= bound, f'{label} molecule {m}: residual c = {c_res:.2f}'
        if project:
            assert np.count_nonzero(np.abs(lam) <= bound) == ref['n_proj']
        worst['evals'], worst['resid'] = max(worst['evals'], c_ev), max(worst['resid'], c_res)
    return worst


@pytest.mark.parametrize('project', [True, False])
@pytest.mark.parametrize('case', ['aspirin1_ckpt', 'ethanol4_rand', 'mixed_rand', 'periodic_ethanol2_rand'])
def test_solver_against_fp64_on_the_same_blocks(case, project):
    from newtonnet_amd import vibrations as vib
    sd, z, pos, cell, batch = solver_inputs(case)
    model = make_model(sd)
    zc, pc, cc, bc = cuda(z, pos, cell, batch)
    blocks, ptr = model.hessian(zc, pc, cc, bc, blocks=True)
    masses = table(z)
    nm = vib.eig_blocks(blocks, ptr, bc, pc, cc, masses.cuda(), project=project)
    check_solver(nm, blocks.cpu().double().numpy(), ptr.cpu().tolist(), z, pos, cell, batch, masses, project, case)
    want = {'aspirin1_ckpt': [6], 'ethanol4_rand': [6] * 4, 'mixed_rand': [6, 6, 3, 5], 'periodic_ethanol2_rand': [3, 3]}[case]
    assert nm.n_projected.tolist() == (want if project else [0] * len(want))


def test_fixture_above_the_bound_is_refused():
    """pbc_batch2_rand (216 and 125 atoms) does not fit one workgroup: refused by name of the bound before any launch"""
    from newtonnet_amd import vibrations as vib
    z, pos, cell, batch, _ = util.case_inputs('pbc_batch2_rand', torch.float32)
    model = make_model(util.load_state('rand'))
    with pytest.raises(NotImplementedError, match=str(vib.max_dim())):
        model.normal_modes(*cuda(z, pos, cell, batch))


@pytest.mark.parametrize('case', ['aspirin1_ckpt', 'ethanol4_rand', 'mixed_rand'])
def test_normal_modes_against_the_oracle(case):
    sd = util.load_state(case.split('_')[-1])
    z, pos, cell, batch, _ = util.case_inputs(case, torch.float32)
    model = make_model(sd)
    args = cuda(z, pos, cell, batch)
    nm = model.normal_modes(*args)
    blocks, ptr = model.hessian(*args, blocks=True)
    blocks, ptr = blocks.cpu().double().numpy(), ptr.cpu().tolist()
    H_or = hr.oracle_hessian(sd, z, pos.double(), cell.double(), batch).numpy()
    masses = table(z).double().numpy()
    lam_all, nu_all = nm.eigenvalues.cpu().double().numpy(), nm.frequencies.cpu().double().numpy()
    for m, idx in molecules(batch):
        n = idx.numel()
        M, o = 3 * n, 3 * idx[0].item()
        ii = idx.numpy()
        p = pos[idx].double().numpy()
        dev = vr.analyse(blocks[ptr[m]:ptr[m] + 9 * n * n].reshape(M, M), p, masses[ii], project=True)
        orc = vr.analyse(H_or[ii][:, :, ii], p, masses[ii], project=True)
        lam, nu = lam_all[o:o + M], nu_all[o:o + M]
        assert int(nm.n_projected[m]) == orc['n_proj']
        if orc['s'] == 0:
            assert np.count_nonzero(lam) == 0 and np.count_nonzero(nu) == 0
            assert int(nm.n_imaginary[m]) == 0 and float(nm.zero_point_energy[m]) == 0.0
            continue
        B = np.linalg.norm(dev['A'] - orc['A'], 2) + vr.solver_bound(M, dev['s'])
        d = np.abs(lam - orc['evals'])
        print(f'{case} molecule {m} (M = {M}): B / s = {B / orc["s"]:.3e}, max |d lambda| / B = {d.max() / B:.3f}')
        assert d.max() <= B
        sel = np.abs(orc['evals']) > 2 * B
        left_out = M - np.count_nonzero(sel)
        print(f'{case} molecule {m}: {left_out} modes inside 2 B (n_projected {orc["n_proj"]})')
        assert left_out <= orc['n_proj'] + (M - orc['n_proj']) // 10
        nu_or = vr.frequencies(orc['evals'])
        dnu = np.abs(nu - nu_or)[sel]
        lim = (vr.WAVENUMBER * B / np.sqrt(np.abs(orc['evals'])))[sel]
        print(f'{case} molecule {m}: worst frequency error {np.max(dnu / lim):.3f} of its bound')
        assert np.all(dnu <= lim), f'worst {np.max(dnu / lim):.3f} of the bound'
        n_neg, n_amb = np.count_nonzero(orc['evals'] < -2 * B), np.count_nonzero(~sel)
        assert n_neg <= int(nm.n_imaginary[m]) <= n_neg + n_amb
        print(f'{case} molecule {m}: n_imaginary {int(nm.n_imaginary[m])} (oracle {n_neg} below -2 B)')


def test_repeatable_and_modes_false_bitwise():
    sd, z, pos, cell, batch = solver_inputs('mixed_rand')
    model = make_model(sd)
    args = cuda(z, pos, cell, batch)
    a, b = model.normal_modes(*args), model.normal_modes(*args)
    assert torch.equal(a.eigenvalues, b.eigenvalues) and torch.equal(a.modes, b.modes) and torch.equal(a.sweeps, b.sweeps)
    c = model.normal_modes(*args, modes=False)
    assert c.modes is None and torch.equal(c.eigenvalues, a.eigenvalues) and torch.equal(c.sweeps, a.sweeps)
    assert torch.equal(model.frequencies(*args), a.frequencies)
    f0, m0 = a.molecule(0)
    assert f0.shape == (63,) and m0.shape == (63, 21, 3) and c.molecule(0)[1] is None
    assert a.ptr.tolist() == [0, 63, 90, 93, 99] and a.ptr.dtype == torch.int64
    cart = a.cartesian(1)
    masses = table(z).cuda()
    torch.testing.assert_close(cart, a.molecule(1)[1] / masses[21:30].sqrt()[None, :, None], rtol=0, atol=0)


def test_default_masses_are_the_table_and_unit_masses_give_plain_eigenvalues():
    from newtonnet_amd import vibrations as vib
    sd, z, pos, cell, batch = solver_inputs('ethanol4_rand')
    model = make_model(sd)
    args = cuda(z, pos, cell, batch)
    a = model.normal_modes(*args)
    b = model.normal_modes(*args, masses=table(z).cuda())
    assert torch.equal(a.eigenvalues, b.eigenvalues) and torch.equal(a.modes, b.modes)
    with pytest.raises(ValueError, match='masses='):
        model.normal_modes(torch.full_like(args[0], 43), *args[1:])
    blocks, ptr = model.hessian(*args, blocks=True)
    nm = vib.eig_blocks(blocks, ptr, args[3], args[1], args[2], None, project=False)
    check_solver(nm, blocks.cpu().double().numpy(), ptr.cpu().tolist(), z, pos, cell, batch, None, False, 'unit masses')
    assert nm.masses is None and nm.n_projected.tolist() == [0] * 4


def test_one_and_two_atom_molecules_next_to_an_ethanol():
    """the construction of test_hip_hessian.test_one_and_two_atom_molecules"""
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand', torch.float32)
    z, pos, cell, batch = mol_subset(z, pos, cell, batch, [0])
    z = torch.cat([z, torch.tensor([8, 1, 1])])
    pos = torch.cat([pos, torch.tensor([[30.0, 0.0, 0.0], [-30.0, 0.0, 0.0], [-30.0, 0.0, 0.74]])])
    cell = torch.zeros(3, 3, 3)
    batch = torch.cat([batch, torch.tensor([1, 2, 2])])
    model = make_model(sd)
    nm = model.normal_modes(*cuda(z, pos, cell, batch))
    assert nm.eigenvalues.shape == (36,) and nm.frequencies.shape == (36,) and nm.modes.shape == (81 * 9 + 9 + 36,)
    assert nm.n_projected.tolist() == [6, 3, 5] and nm.ptr.tolist() == [0, 27, 30, 36]
    f1, m1 = nm.molecule(1)
    assert torch.count_nonzero(f1) == 0 and torch.count_nonzero(nm.eigenvalues[27:30]) == 0 and m1.shape == (3, 1, 3)
    assert int(nm.sweeps[1]) == 0 and int(nm.n_imaginary[1]) == 0 and float(nm.zero_point_energy[1]) == 0.0
    f2, m2 = nm.molecule(2)
    assert f2.shape == (6,) and m2.shape == (6, 2, 3)
    blocks, ptr = model.hessian(*cuda(z, pos, cell, batch), blocks=True)
    check_solver(nm, blocks.cpu().double().numpy(), ptr.cpu().tolist(), z, pos, cell, batch, table(z), True, 'small molecules')


def test_molecule_above_the_bound_raises_before_any_kernel():
    from newtonnet_amd import hip
    from newtonnet_amd import vibrations as vib
    bound = vib.max_dim()
    assert 96 <= bound < 10 ** 6
    n = bound // 3 + 1
    blocks = torch.zeros(9 * n * n + 81, device='cuda')
    ptr = torch.tensor([0, 81], device='cuda')
    batch = torch.cat([torch.zeros(3, dtype=torch.long), torch.ones(n, dtype=torch.long)]).cuda()
    pos, cell = torch.randn(n + 3, 3, device='cuda'), torch.zeros(2, 3, 3, device='cuda')
    with pytest.raises(NotImplementedError, match=str(bound)):
        vib.eig_blocks(blocks, ptr, batch, pos, cell)
    # the library's own check (what a C caller meets): NNHIP_E_UNSUPPORTED, the message names the bound and the molecule
    mol_host = torch.tensor([0, 3, 3 + n], dtype=torch.int32)
    mol_dev = mol_host.cuda()
    ev = torch.full((3 * (n + 3),), 7.0, device='cuda')
    ints = torch.full((6,), -1, dtype=torch.int32, device='cuda')
    rc = hip.lib().nnhip_eig_blocks(blocks.data_ptr(), ptr.data_ptr(), mol_dev.data_ptr(), mol_host.data_ptr(), 2, pos.data_ptr(),
                                    cell.data_ptr(), None, 1, ev.data_ptr(), None, ints[0:2].data_ptr(), ints[2:4].data_ptr(),
                                    ints[4:6].data_ptr(), hip._stream(blocks.device))
    msg = hip.lib().nnhip_last_error().decode()
    assert rc == 2 and str(bound) in msg and 'molecule 1' in msg
    torch.cuda.synchronize()
    assert bool((ev == 7.0).all()) and bool((ints == -1).all())          # nothing ran


def test_largest_supported_molecule():
    """a synthetic block at the bound itself (the dynamic-LDS request above 64 KiB): random symmetric matrix, unit masses"""
    from newtonnet_amd import vibrations as vib
    M = vib.max_dim()
    n = M // 3
    g = torch.Generator().manual_seed(5)
    X = torch.randn(M, M, generator=g)
    blocks = (X + X.T).reshape(-1).contiguous()
    pos = torch.randn(n, 3, generator=g) * 3
    batch, cell, ptr = torch.zeros(n, dtype=torch.long), torch.zeros(1, 3, 3), torch.zeros(1, dtype=torch.long)
    for project in (False, True):
        nm = vib.eig_blocks(blocks.cuda(), ptr.cuda(), batch.cuda(), pos.cuda(), cell.cuda(), None, project=project)
        check_solver(nm, blocks.double().numpy(), [0], None, pos, cell, batch, None, project, f'M = {M}')


def test_forward_unchanged_and_preconditions():
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('aspirin1_rand', torch.float32)
    model = make_model(sd)
    args = cuda(z, pos, cell, batch)
    o1 = model(*args)
    e1, f1 = o1.energy.clone(), o1.gradient_force.clone()
    model.normal_modes(*args)
    o2 = model(*args)
    assert torch.equal(o2.energy, e1) and torch.equal(o2.gradient_force, f1)
    model.train()
    with pytest.raises(NotImplementedError, match='eval'):
        model.normal_modes(*args)
    with pytest.raises(NotImplementedError, match='eval'):
        model.frequencies(*args)
    from newtonnet_amd.models import NewtonNet
    m2 = NewtonNet(output_properties=['direct_force']).cuda()
    m2.eval()
    with pytest.raises(NotImplementedError, match='energy'):
        m2.normal_modes(*args)


def test_bad_mass_is_flagged_on_the_device_and_the_molecule_left_alone():
    from newtonnet_amd import vibrations as vib
    sd, z, pos, cell, batch = solver_inputs('ethanol4_rand')
    model = make_model(sd)
    args = cuda(z, pos, cell, batch)
    blocks, ptr = model.hessian(*args, blocks=True)
    masses = table(z).cuda()
    good = vib.eig_blocks(blocks, ptr, args[3], args[1], args[2], masses)
    for bad_value in (0.0, -1.0, float('nan'), float('inf')):
        m = masses.clone()
        m[9 + 4] = bad_value                                  # an atom of molecule 1
        nm = vib.eig_blocks(blocks, ptr, args[3], args[1], args[2], m)
        assert nm.status.tolist() == [0, 4, 0, 0]
        assert torch.count_nonzero(nm.eigenvalues[27:54]) == 0 and torch.count_nonzero(nm.molecule(1)[1]) == 0
        assert int(nm.n_imaginary[1]) == 0 and float(nm.zero_point_energy[1]) == 0.0
        for lo, hi in ((0, 27), (54, 108)):
            assert torch.equal(nm.eigenvalues[lo:hi], good.eigenvalues[lo:hi])


def test_library_skips_a_molecule_larger_than_the_host_offsets_said():
    """a C caller whose device and host offsets disagree: the molecule that would not fit the launch's LDS is skipped with status
    bit 1, nothing is written out of bounds"""
    from newtonnet_amd import hip
    blocks = torch.zeros(81 + 729, device='cuda')
    ptr = torch.tensor([0, 81], device='cuda')
    mol_dev = torch.tensor([0, 3, 12], dtype=torch.int32, device='cuda')      # molecule 1: 9 atoms
    mol_host = torch.tensor([0, 3, 6], dtype=torch.int32)                      # ... but 3 by the host copy
    ev = torch.full((36,), 7.0, device='cuda')
    ints = torch.full((6,), -1, dtype=torch.int32, device='cuda')
    pos, cell = torch.randn(12, 3, device='cuda'), torch.zeros(2, 3, 3, device='cuda')
    rc = hip.lib().nnhip_eig_blocks(blocks.data_ptr(), ptr.data_ptr(), mol_dev.data_ptr(), mol_host.data_ptr(), 2, pos.data_ptr(),
                                    cell.data_ptr(), None, 1, ev.data_ptr(), None, ints[0:2].data_ptr(), ints[2:4].data_ptr(),
                                    ints[4:6].data_ptr(), hip._stream(blocks.device))
    torch.cuda.synchronize()
    assert rc == 0 and ints[4:6].tolist() == [0, 2]
    assert torch.count_nonzero(ev[:9]) == 0 and bool((ev[9:] == 7.0).all())


def test_input_validation():
    from newtonnet_amd import vibrations as vib
    blocks, ptr = torch.zeros(81, device='cuda'), torch.zeros(1, dtype=torch.long, device='cuda')
    batch, pos, cell = torch.zeros(3, dtype=torch.long, device='cuda'), torch.zeros(3, 3, device='cuda'), torch.zeros(1, 3, 3, device='cuda')
    vib.eig_blocks(blocks, ptr, batch, pos, cell)
    with pytest.raises(ValueError):
        vib.eig_blocks(blocks.double(), ptr, batch, pos, cell)
    with pytest.raises(ValueError):
        vib.eig_blocks(blocks, ptr.int(), batch, pos, cell)
    with pytest.raises(ValueError):
        vib.eig_blocks(blocks[:80], ptr, batch, pos, cell)
    with pytest.raises(ValueError):
        vib.eig_blocks(blocks, ptr, batch, pos, cell, masses=torch.ones(2, device='cuda'))
    with pytest.raises(ValueError):
        vib.eig_blocks(blocks, ptr, batch, pos.cpu(), cell)
    with pytest.raises(NotImplementedError):
        vib.eig_blocks(blocks, ptr, batch, pos.double(), cell)


def test_calculator_vibrations_one_and_three_frames():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    z, pos, cell, batch, _ = util.case_inputs('aspirin8_rand', torch.float32)
    sd = util.load_state('rand', torch.float32)
    calc = MLAseCalculator(sd, properties=['energy', 'forces'], device='cuda')
    frames = [FakeAtoms(z[batch == b].numpy(), pos[batch == b].numpy().astype(np.float64)) for b in range(3)]
    f1, m1 = calc.vibrations(frames[0])
    assert f1.shape == (63,) and m1.shape == (63, 21, 3) and f1.dtype == np.float32
    f3, m3 = calc.vibrations(frames)
    assert f3.shape == (3, 63) and m3.shape == (3, 63, 21, 3)
    assert 'vibrations' not in calc.implemented_properties and 'frequencies' not in calc.implemented_properties
    # frame 0 alone and in the batch of three: each solve is within the solver bound of the exact spectrum of ITS matrix, and the
    # two matrices differ by what the two Hessian calls differ (another replica count, another summation order).  By Weyl the
    # eigenvalues differ by at most ||A_1 - A_3||_2, measured here from the device's own blocks (mass-weighted and projected by
    # the yardstick in fp64), plus the two solver bounds -- the construction of B in test_normal_modes_against_the_oracle.
    masses = table(z[:21]).double().numpy()
    p0 = pos[:21].double().numpy()
    zz, pp, cc, bb = calc.format_data(frames[:1])
    b1, _ = calc.model.hessian(zz, pp, cc, bb, blocks=True)
    zz, pp, cc, bb = calc.format_data(frames)
    b3, _ = calc.model.hessian(zz, pp, cc, bb, blocks=True)
    r1 = vr.analyse(b1.cpu().double().numpy(), p0, masses, project=True)
    r3 = vr.analyse(b3[:63 * 63].cpu().double().numpy(), p0, masses, project=True)
    dA = np.linalg.norm(r1['A'] - r3['A'], 2)
    lim = dA + vr.solver_bound(63, r1['s']) + vr.solver_bound(63, r3['s'])
    lam1, lam3 = (np.sign(f) * (f.astype(np.float64) / vr.WAVENUMBER) ** 2 for f in (f1, f3[0]))
    d = np.abs(lam1 - lam3).max()
    print(f'frame 0 alone vs in the batch: max |d lambda| {d:.3e}; ||A_1 - A_3||_2 {dA:.3e}, one solver bound '
          f'{vr.solver_bound(63, r1["s"]):.3e}, limit {lim:.3e}')
    assert d <= lim
    with pytest.raises(ValueError, match='different sizes'):
        calc.vibrations([frames[0], FakeAtoms(frames[0].numbers[:9], frames[0].positions[:9])])
    zz, pp, cc, bb = calc.format_data(frames[:1])
    # an atoms object with masses of its own: they are used

    class Heavy(FakeAtoms):
        def get_masses(self):
            return np.full(len(self.numbers), 4.0)
    f4, _ = calc.vibrations(Heavy(frames[0].numbers, frames[0].positions))
    nm = calc.model.normal_modes(zz, pp, cc, bb, masses=torch.full((21,), 4.0, device='cuda'))
    np.testing.assert_array_equal(f4, nm.frequencies.cpu().numpy())


def test_zero_point_energy_and_imaginary_count_definitions():
    sd = util.load_state('ckpt')
    z, pos, cell, batch, _ = util.case_inputs('aspirin1_ckpt', torch.float32)
    model = make_model(sd)
    nm = model.normal_modes(*cuda(z, pos, cell, batch))
    lam, nu = nm.eigenvalues.cpu().double().numpy(), nm.frequencies.cpu().double().numpy()
    np.testing.assert_allclose(nu, vr.frequencies(lam), rtol=4 * vr.EPS32, atol=0)
    thr = 8 * 63 * vr.EPS32 * np.abs(nm.eigenvalues.cpu().numpy()).max()
    assert int(nm.n_imaginary[0]) == np.count_nonzero(lam < -thr) and int(nm.n_imaginary[0]) > 0
    zpe = 0.5 * vr.EV_PER_WAVENUMBER * nu[lam > thr].sum()
    assert abs(float(nm.zero_point_energy[0]) - zpe) <= 63 * vr.EPS32 * zpe and zpe > 0
    assert np.count_nonzero(np.abs(lam) <= thr) == 6
    # a caller's own threshold
    nm2 = model.normal_modes(*cuda(z, pos, cell, batch), tol_zero=0.5)
    assert int(nm2.n_imaginary[0]) == np.count_nonzero(lam < -0.5 * np.abs(lam).max())
