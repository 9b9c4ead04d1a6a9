"""Normal-mode / Wigner sampling and harmonic thermochemistry on the HIP path (newtonnet_amd/vibrations.py, csrc/sample.hip).

Kernel alone: synthetic NormalModes inputs (tests/sample_ref.py: seeded orthonormal mode matrices, spectra with zeros, negatives and
values within 2 x of the threshold on both sides, explicit draws xi) against the fp64 statement of the same formulas on the SAME
fp32 inputs.  Per molecule and sample, with M = 3 n_b, eps32 = 2^-24 and c = 8 (sample_ref.C_SAMPLE, the eigensolver tests' constant):
    |dx - dx_ref|  <= c M eps32 max_k |q_k| / sqrt(m_min)        |q - q_ref| <= c M eps32 max_k |q_k|
    |E_h - E_h_ref| <= c M eps32 max_k |lambda_k q_k^2 / 2|
The kernel returns pos + dx rounded to fp32, so the position comparison adds that one rounding, half an fp32 ulp of |pos + dx|.
Thermochemistry: |X - X_ref| <= c M eps32 sum |terms| (+ the smallest normal fp32 number) for X = U, S, F, C_v with the terms of
sample_ref.thermo_terms."""
import numpy as np
import pytest
import torch

from tests import hessian_ref as hr
from tests import sample_ref as sr
from tests import util
from tests.test_hip_hessian import cuda, make_model

pytestmark = pytest.mark.gpu

TINY32 = float(np.finfo(np.float32).tiny)


def pack(mols, tol_zero=None):
    """the NormalModes eig_blocks would return for these spectra and modes (on the device), molecule b in the cell 100 (b + 1) I"""
    from newtonnet_amd import vibrations as vib
    counts = [m['n'] for m in mols]
    n_mol = len(mols)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    blk = np.concatenate([[0], np.cumsum([9 * n * n for n in counts])]).astype(np.int64)
    evals = torch.from_numpy(np.concatenate([m['lam'] for m in mols])).cuda()
    modes = torch.from_numpy(np.concatenate([m['modes'].reshape(-1) for m in mols])).cuda()
    ptr, blk_ptr = torch.from_numpy(3 * offs).cuda(), torch.from_numpy(blk[:-1].copy()).cuda()
    batch = torch.repeat_interleave(torch.arange(n_mol), torch.tensor(counts)).cuda()
    pos = torch.from_numpy(np.concatenate([m['pos'] for m in mols])).cuda()
    cell = (100.0 * torch.arange(1, n_mol + 1).float()[:, None, None] * torch.eye(3)).cuda()
    masses = None if mols[0]['masses'] is None else torch.from_numpy(np.concatenate([m['masses'] for m in mols])).cuda()
    z = (torch.arange(int(offs[-1])) % 8 + 1).cuda()
    freq, thr, n_imag, zpe = vib.derived_quantities(evals, ptr, batch, n_mol, tol_zero)
    zeros = torch.zeros(n_mol, dtype=torch.int32, device='cuda')
    return vib.NormalModes(eigenvalues=evals, frequencies=freq, modes=modes, ptr=ptr, blk_ptr=blk_ptr, n_projected=zeros, sweeps=zeros,
                           status=zeros, n_imaginary=n_imag, zero_point_energy=zpe, masses=masses, threshold=thr, pos=pos, cell=cell,
                           z=z, _counts=counts, _offsets=offs[:-1].tolist(), _blk_offsets=blk[:-1].tolist())


def pack_draws(draws):
    return torch.from_numpy(np.concatenate([d.reshape(-1) for d in draws])).cuda()


def per_molecule(out, mols, S):
    """[(pos [S, n, 3], q [S, M], energy [S])] per molecule, on the host"""
    pos, q, en = out.pos.cpu().numpy(), out.amplitudes.cpu().numpy(), out.harmonic_energy.cpu().numpy()
    res, a0 = [], 0
    for b, m in enumerate(mols):
        n = m['n']
        res.append((pos[S * a0:S * (a0 + n)].reshape(S, n, 3), q[3 * S * a0:3 * S * (a0 + n)].reshape(S, 3 * n), en[b * S:(b + 1) * S]))
        a0 += n
    return res


@pytest.mark.parametrize('quantum,T', [(False, 300.0), (True, 300.0), (True, 0.0)])
@pytest.mark.parametrize('S', [1, 33])
@pytest.mark.parametrize('with_masses', [False, True])
def test_kernel_against_fp64_on_the_same_inputs(with_masses, S, quantum, T):
    mols = sr.synthetic_molecules(with_masses)
    draws = sr.synthetic_draws(mols, S)
    nm = pack(mols)
    out = nm.sample(S, T, quantum=quantum, xi=pack_draws(draws))
    N, B = sum(m['n'] for m in mols), len(mols)
    assert out.pos.shape == (S * N, 3) and out.harmonic_energy.shape == (B * S,) and out.amplitudes.shape == (3 * S * N,)
    assert out.n_skipped_imaginary.shape == (B,) and out.batch.shape == (S * N,) and out.cell.shape == (B * S, 3, 3)
    thr_dev = nm.threshold.cpu().numpy()
    worst = dict(dx=0.0, q=0.0, e=0.0)
    a0 = 0
    for b, (m, xi, (pos_d, q_d, e_d)) in enumerate(zip(mols, draws, per_molecule(out, mols, S))):
        n, M = m['n'], 3 * m['n']
        # the sample batch: molecule b S + s is sample s of molecule b, with its cell and its species
        rows = slice(S * a0, S * (a0 + n))
        assert out.batch[rows].cpu().tolist() == [b * S + s for s in range(S) for _ in range(n)]
        assert torch.equal(out.cell[b * S:(b + 1) * S], nm.cell[b:b + 1].expand(S, 3, 3))
        assert torch.equal(out.z[rows], nm.z[a0:a0 + n].repeat(S))
        a0 += n
        if n == 0:
            assert int(out.n_skipped_imaginary[b]) == 0
            continue
        thr = float(thr_dev[b])
        assert thr_dev[b] == sr.default_threshold(M, np.abs(m['lam']).max())
        ref = sr.sample(m['modes'], m['lam'], thr, m['masses'], m['pos'], xi, T, quantum)
        assert int(out.n_skipped_imaginary[b]) == ref['n_skipped']
        if n == 1:
            assert np.array_equal(pos_d, np.broadcast_to(m['pos'], (S, 1, 3))) and not q_d.any() and not e_d.any()
            continue
        b_dx, b_e = sr.displacement_bound(M, ref['q'], m['masses']), sr.energy_bound(M, m['lam'], thr, ref['q'])
        b_q = sr.C_SAMPLE * M * sr.EPS32 * np.abs(ref['q']).max(axis=1)
        assert np.all(b_q > 0)
        half_ulp = 0.5 * np.spacing(np.abs(ref['pos']).astype(np.float32)).astype(np.float64)
        d_pos = np.abs(pos_d.astype(np.float64) - ref['pos'])
        d_q, d_e = np.abs(q_d - ref['q']).max(axis=1), np.abs(e_d - ref['energy'])
        c = dict(dx=float(np.max((d_pos - half_ulp).max(axis=(1, 2)) / b_dx)) * sr.C_SAMPLE, q=float(np.max(d_q / b_q)) * sr.C_SAMPLE,
                 e=float(np.max(d_e / b_e)) * sr.C_SAMPLE)
        print(f'molecule {b} (M = {M}, masses {with_masses}, S = {S}, quantum {quantum}, T = {T}): observed c displacement '
              f'{max(c["dx"], 0.0):.4f}, amplitudes {c["q"]:.4f}, energy {c["e"]:.4f} (allowed {sr.C_SAMPLE})')
        assert np.all(d_pos <= b_dx[:, None, None] + half_ulp), f'molecule {b}: displacement c = {c["dx"]:.3f}'
        assert np.all(d_q <= b_q), f'molecule {b}: amplitudes c = {c["q"]:.3f}'
        assert np.all(d_e <= b_e), f'molecule {b}: harmonic energy c = {c["e"]:.3f}'
        dead = m['lam'] <= thr
        assert not q_d[:, dead].any() and np.all(q_d[:, ~dead] != 0)
        for k in worst:
            worst[k] = max(worst[k], c[k])
    print(f'worst observed c: displacement {worst["dx"]:.4f}, amplitudes {worst["q"]:.4f}, energy {worst["e"]:.4f}')


def test_repeats_are_bitwise_and_a_sample_does_not_depend_on_the_number_of_samples():
    mols = sr.synthetic_molecules(True)
    nm = pack(mols)
    d1, d33 = sr.synthetic_draws(mols, 1), sr.synthetic_draws(mols, 33)
    for quantum in (False, True):
        a = nm.sample(33, 300.0, quantum=quantum, xi=pack_draws(d33))
        b = nm.sample(33, 300.0, quantum=quantum, xi=pack_draws(d33))
        for name in ('pos', 'harmonic_energy', 'amplitudes', 'n_skipped_imaginary', 'batch', 'z', 'cell'):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        one = nm.sample(1, 300.0, quantum=quantum, xi=pack_draws(d1))
        for (p1, q1, e1), (p33, q33, e33) in zip(per_molecule(one, mols, 1), per_molecule(a, mols, 33)):
            assert np.array_equal(p1[0], p33[0]) and np.array_equal(q1[0], q33[0]) and np.array_equal(e1, e33[:1])
        assert torch.equal(one.n_skipped_imaginary, a.n_skipped_imaginary)
    # sample 32 (the second tile's first) from a run of 33 and as the only sample of a run of its own
    tail = [d[32:] for d in d33]
    last = nm.sample(1, 300.0, xi=pack_draws(tail))
    full = nm.sample(33, 300.0, xi=pack_draws(d33))
    for (p1, q1, e1), (p33, q33, e33) in zip(per_molecule(last, mols, 1), per_molecule(full, mols, 33)):
        assert np.array_equal(p1[0], p33[32]) and np.array_equal(q1[0], q33[32]) and np.array_equal(e1, e33[32:])


def test_imaginary_modes_are_skipped_and_counted():
    rng = np.random.default_rng(5)
    lam = np.array([-1.0, -0.5, 0, 0, 0, 0, 0.7, 1.1, 2.0], dtype=np.float32)
    mol = dict(n=3, lam=lam, modes=np.ascontiguousarray(np.linalg.qr(rng.standard_normal((9, 9)))[0].T).astype(np.float32),
               pos=rng.standard_normal((3, 3)).astype(np.float32), masses=np.array([15.999, 1.008, 1.008], dtype=np.float32))
    nm = pack([mol])
    assert nm.n_imaginary.tolist() == [2]
    xi = rng.standard_normal((5, 9)).astype(np.float32)
    a = nm.sample(5, 300.0, quantum=True, xi=pack_draws([xi]))
    assert a.n_skipped_imaginary.tolist() == [2]
    for fill in (0.0, -3.0, float('nan')):
        xi2 = xi.copy()
        xi2[:, :2] = fill                                            # the draws of the two imaginary modes
        b = nm.sample(5, 300.0, quantum=True, xi=pack_draws([xi2]))
        for name in ('pos', 'harmonic_energy', 'amplitudes'):
            assert torch.equal(getattr(a, name), getattr(b, name)), (name, fill)
    assert torch.count_nonzero(a.amplitudes.view(5, 9)[:, :6]) == 0
    # a caller's own threshold moves the rule for all three users at once
    wide = pack([mol], tol_zero=0.4)                                 # threshold 0.8: one live mode short, one imaginary mode short
    out = wide.sample(5, 300.0, xi=pack_draws([xi]))
    assert wide.n_imaginary.tolist() == [1] and out.n_skipped_imaginary.tolist() == [1]
    assert torch.count_nonzero(out.amplitudes.view(5, 9)[:, :7]) == 0 and bool((out.amplitudes.view(5, 9)[:, 7:] != 0).all())


@pytest.mark.parametrize('T', [0.0, 10.0, 300.0, 2000.0])
def test_thermochemistry_against_fp64(T):
    mols = sr.synthetic_molecules(False)
    nm = pack(mols)
    t = nm.thermochemistry(T)
    got = {k: getattr(t, k).cpu().numpy() for k in ('U', 'S', 'F', 'Cv')}
    thr_dev = nm.threshold.cpu().numpy()
    for k, v in got.items():
        assert v.shape == (len(mols),) and v.dtype == np.float32, k
    if T == 0.0:
        assert torch.equal(t.U, nm.zero_point_energy) and torch.equal(t.F, nm.zero_point_energy)
        assert not got['S'].any() and not got['Cv'].any()
    for b, m in enumerate(mols):
        M = 3 * m['n']
        ref = sr.thermochemistry(m['lam'], float(thr_dev[b]), T) if M else dict(U=0, S=0, F=0, Cv=0, U_abs=0, S_abs=0, F_abs=0, Cv_abs=0)
        for k in ('U', 'S', 'F', 'Cv'):
            err, lim = abs(float(got[k][b]) - ref[k]), sr.C_SAMPLE * M * sr.EPS32 * ref[k + '_abs']
            if ref[k + '_abs'] > 0:
                print(f'T = {T}: molecule {b} (M = {M}) {k} = {ref[k]:.6e}, observed c {err / lim * sr.C_SAMPLE:.4f}')
            assert err <= lim + TINY32, f'T = {T} molecule {b} {k}: {got[k][b]} vs {ref[k]}, c = {err / max(lim, 1e-300) * sr.C_SAMPLE:.3f}'
    if T > 0:
        assert np.all(got['S'][[1, 3, 4, 5, 6]] > 0) and np.all(got['Cv'][[1, 3, 4, 5, 6]] > 0)


def oracle_parts(sd, z, pos, new_pos, cell, batch, dtype):
    """the oracle in `dtype` at pos [N,3] and at every new_pos[s] [N,3]: E0 [B], g = dE/dpos [N,3], [(E(new_pos[s]) [B], H dx_s [N,3])]
    with dx_s = new_pos[s] - pos (one double backward per sample); everything returned in fp64"""
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    c = cell.to(dtype)
    p = pos.to(dtype).clone().requires_grad_(True)
    e0 = hr.oracle_energy(sdd, z, p, c, batch).reshape(-1)
    (g,) = torch.autograd.grad(e0.sum(), p, create_graph=True)
    out = []
    for xn in new_pos:
        dx = (xn.double() - pos.double()).to(dtype)
        (hd,) = torch.autograd.grad((g * dx).sum(), p, retain_graph=True)
        with torch.no_grad():
            e1 = hr.oracle_energy(sdd, z, xn.to(dtype), c, batch).reshape(-1)
        out.append((e1.double(), hd.double()))
    return e0.detach().double(), g.detach().double(), out


def test_samples_through_the_model_follow_the_harmonic_energy():
    """ethanol + aspirin, random weights, T = 300 K, draws scaled by 1e-2 (displacements of order 1e-3 A).  Per sample
        dE = E(x + dx) - E(x) + F(x) . dx
    of the device model against harmonic_energy for a molecule whose spectrum is all real, else against dx^T H dx / 2 with the
    device's model.hessian.  Allowed: the fp32 resolution of the two energies (util.energy_tol each) + FORCE_MAX_TOL sum |dx| + the
    cubic remainder |dE - dx^T H dx / 2| of the fp64 oracle at the same dx, or 4 x the discrepancy of the fp32 oracle in the same
    check, whichever is larger (the yardstick convention of test_hip_hessian_forms.py).
    The calibrated values (cubic remainder, fp32 oracle discrepancy, device) are printed per sample; they have not been recorded
    here yet because this test has not run on a device."""
    S = 3
    sd = util.load_state('rand')
    z, pos, cell, batch = hr.ethanol_and_aspirin()
    model = make_model(sd)
    args = cuda(z, pos, cell, batch)
    nm = model.normal_modes(*args)
    xi = 1e-2 * torch.randn(S * 3 * pos.shape[0], generator=torch.Generator().manual_seed(0))
    out = nm.sample(S, 300.0, xi=xi.cuda())
    o0 = model(*args)
    e0_d, f_d = o0.energy.detach().cpu().double().reshape(-1), o0.gradient_force.detach().cpu().double()
    e1_d = model(out.z, out.pos, out.cell, out.batch).energy.detach().cpu().double().reshape(-1)
    H_d = model.hessian(*args).cpu().double()
    eh_d, n_skip = out.harmonic_energy.cpu().double(), out.n_skipped_imaginary.tolist()
    counts = [9, 21]
    assert out.pos.shape == (S * 30, 3) and e1_d.shape == (2 * S,)
    # sample s of both molecules as one geometry of the original batch
    new_all = out.pos.cpu()
    new_pos = [torch.cat([new_all[0:27].view(S, 9, 3)[s], new_all[27:].view(S, 21, 3)[s]]) for s in range(S)]
    e0_64, g_64, o64 = oracle_parts(sd, z, pos, new_pos, cell, batch, torch.float64)
    e0_32, g_32, o32 = oracle_parts(sd, z, pos, new_pos, cell, batch, torch.float32)
    for s in range(S):
        dx = new_pos[s].double() - pos.double()
        assert 1e-5 < dx.abs().max() < 2e-2
        for m, idx in enumerate((slice(0, 9), slice(9, 30))):
            d = dx[idx]
            q64 = 0.5 * float((d * o64[s][1][idx]).sum())
            de64 = float(o64[s][0][m] - e0_64[m] - (g_64[idx] * d).sum())
            de32 = float(o32[s][0][m] - e0_32[m] - (g_32[idx] * d).sum())
            cubic, yard = abs(de64 - q64), abs(de32 - q64)
            de_dev = float(e1_d[m * S + s] - e0_d[m] + (f_d[idx] * d).sum())
            q_h = float(eh_d[m * S + s])
            q_H = 0.5 * float(torch.einsum('ia,iajb,jb->', d, H_d[idx, :, idx, :], d))
            target = q_h if n_skip[m] == 0 else q_H
            base = float(util.energy_tol(float(o64[s][0][m])) + util.energy_tol(float(e0_64[m]))) + util.FORCE_MAX_TOL * float(d.abs().sum()) + cubic
            lim = max(base, 4 * yard)
            print(f'sample {s} molecule {m} ({counts[m]} atoms, {n_skip[m]} imaginary modes skipped): harmonic energy {q_h:.4e}, '
                  f'dx^T H dx / 2 device {q_H:.4e} oracle {q64:.4e}; dE device {de_dev:.4e} fp64 oracle {de64:.4e}; cubic remainder '
                  f'{cubic:.2e}, fp32 oracle discrepancy {yard:.2e}, device {abs(de_dev - target):.2e}, allowed {lim:.2e}')
            assert abs(de_dev - target) <= lim


def test_model_and_calculator_interfaces():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    sd = util.load_state('rand')
    z, pos, cell, batch = hr.ethanol_and_aspirin()
    model = make_model(sd)
    args = cuda(z, pos, cell, batch)

    def gen(seed):
        g = torch.Generator(device='cuda')
        g.manual_seed(seed)
        return g
    a = model.sample_displacements(*args, 4, 300.0, generator=gen(1))
    b = model.sample_displacements(*args, 4, 300.0, generator=gen(1))
    c = model.sample_displacements(*args, 4, 300.0, generator=gen(2))
    assert a.pos.shape == (120, 3) and a.z.shape == (120,) and a.batch.shape == (120,) and a.cell.shape == (8, 3, 3)
    assert a.harmonic_energy.shape == (8,) and a.n_skipped_imaginary.shape == (2,) and a.amplitudes.shape == (360,)
    assert torch.equal(a.pos, b.pos) and torch.equal(a.harmonic_energy, b.harmonic_energy) and not torch.equal(a.pos, c.pos)
    assert torch.equal(a.z, torch.cat([args[0][:9].repeat(4), args[0][9:].repeat(4)]))
    assert a.batch.tolist() == [k for k in range(4) for _ in range(9)] + [k for k in range(4, 8) for _ in range(21)]
    e = model(a.z, a.pos, a.cell, a.batch).energy
    assert e.reshape(-1).shape == (8,) and bool(torch.isfinite(e).all())
    w = model.sample_displacements(*args, 2, 0.0, quantum=True, generator=gen(1))
    assert bool((w.harmonic_energy > 0).all())                       # the ground state moves; the classical T = 0 does not
    cold = model.sample_displacements(*args, 2, 0.0, generator=gen(1))
    assert torch.equal(cold.pos, torch.cat([args[1][:9].repeat(2, 1), args[1][9:].repeat(2, 1)])) and not cold.harmonic_energy.any()
    # masses of the caller's
    heavy = model.sample_displacements(*args, 4, 300.0, masses=torch.full((30,), 4.0, device='cuda'), generator=gen(1))
    assert not torch.equal(heavy.pos, a.pos)
    nm = model.normal_modes(*args)
    t = nm.thermochemistry(300.0)
    assert t.U.shape == (2,) and bool((t.U >= nm.zero_point_energy).all()) and bool((t.F <= t.U).all())
    with pytest.raises(ValueError, match='xi is on'):
        nm.sample(2, 300.0, xi=torch.zeros(180))
    with pytest.raises(ValueError, match='xi'):
        nm.sample(2, 300.0, xi=torch.zeros(90, device='cuda'))
    with pytest.raises(ValueError, match='generator'):
        nm.sample(2, 300.0, generator=torch.Generator())
    with pytest.raises(ValueError, match='modes=False'):
        model.normal_modes(*args, modes=False).sample(2, 300.0)
    # the calculator
    calc = MLAseCalculator(util.load_state('rand', torch.float32), properties=['energy', 'forces'], device='cuda')
    atoms = FakeAtoms(z[9:].numpy(), (pos[9:] - 30.0).numpy().astype(np.float64))
    x1, x2, x3 = calc.sample(atoms, 5, 300.0, seed=3), calc.sample(atoms, 5, 300.0, seed=3), calc.sample(atoms, 5, 300.0, seed=4)
    assert x1.shape == (5, 21, 3) and np.array_equal(x1, x2) and not np.array_equal(x1, x3)
    assert np.abs(x1 - atoms.positions[None]).max() < 2.0 and calc.sample(atoms, 2, 300.0, quantum=True).shape == (2, 21, 3)

    class Heavy(FakeAtoms):
        def get_masses(self):
            return np.full(len(self.numbers), 4.0)
    x4 = calc.sample(Heavy(atoms.numbers, atoms.positions), 5, 300.0, seed=3)
    assert x4.shape == (5, 21, 3) and not np.array_equal(x4, x1)


def test_molecule_above_the_bound_is_refused_as_before():
    from newtonnet_amd import hip
    from newtonnet_amd import vibrations as vib
    bound = vib.max_dim()
    z, pos, cell, batch, _ = util.case_inputs('pbc_batch2_rand', torch.float32)
    model = make_model(util.load_state('rand'))
    with pytest.raises(NotImplementedError, match=f'above the {bound} the batched eigensolver'):
        model.sample_displacements(*cuda(z, pos, cell, batch), 2, 300.0)
    # the library's own check (what a C caller meets): NNHIP_E_UNSUPPORTED before any launch
    n = bound // 3 + 1
    mol_host = torch.tensor([0, 3, 3 + n], dtype=torch.int32)
    mol_dev = mol_host.cuda()
    f = lambda k: torch.full((k,), 7.0, device='cuda')             # noqa: E731
    modes, evals, thr, xi, pos, new_pos, en = f(81 + 9 * n * n), f(3 * (n + 3)), f(2), f(3 * (n + 3)), f(3 * (n + 3)), f(3 * (n + 3)), f(2)
    blk_ptr = torch.tensor([0, 81], device='cuda')
    skipped = torch.full((2,), -5, dtype=torch.int32, device='cuda')
    rc = hip.lib().nnhip_mode_sample(modes.data_ptr(), evals.data_ptr(), blk_ptr.data_ptr(), mol_dev.data_ptr(), mol_host.data_ptr(), 2,
                                     None, pos.data_ptr(), thr.data_ptr(), 300.0, 0, 1, xi.data_ptr(), new_pos.data_ptr(),
                                     en.data_ptr(), None, skipped.data_ptr(), hip._stream(modes.device))
    msg = hip.lib().nnhip_last_error().decode()
    assert rc == 2 and str(bound) in msg and 'molecule 1' in msg
    torch.cuda.synchronize()
    assert bool((new_pos == 7.0).all()) and bool((en == 7.0).all()) and bool((skipped == -5).all())     # nothing ran
