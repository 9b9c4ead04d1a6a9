"""Normal-mode / Wigner sampling above 42 atoms on the HIP path: the tiled kernel of csrc/sample_large.hip behind
NormalModes.sample(kernel='tiled' / 'auto'), NewtonNet.sample_displacements(solver=...) and the calculator's sample(solver=...).

Synthetic NormalModes inputs as in tests/test_hip_sampling.py (tests/sample_ref.py: seeded orthonormal mode matrices rounded once to
fp32, spectra with zeros, negatives and values within 2 x of the threshold on both sides, explicit draws xi, masses from
{1.008, 12.011, 15.999}) against the fp64 statement of the same formulas on the SAME fp32 inputs, with that file's bounds.  Per
molecule and sample, with M = 3 n_b, eps32 = 2^-24 and c = 8 (sample_ref.C_SAMPLE):
    |dx - dx_ref|  <= c M eps32 max_k |q_k| / sqrt(m_min)  (+ half an fp32 ulp of |pos + dx|: the kernel returns pos + dx in fp32)
    |q - q_ref|    <= c M eps32 max_k |q_k|
    |E_h - E_h_ref| <= c M eps32 max_k |lambda_k q_k^2 / 2|
An fp32 emulation of the serial k sum on these inputs (unfused multiply-add) gives an observed c of 0.009-0.04 for displacements and
0.0005-0.008 for amplitudes at 43, 86, 171 and 512 atoms in all three modes: the bounds have more than 200 x room, and a failure is a
kernel defect.  The sizes are the smallest that reach each edge of the kernel (column tiles of 256, mode chunks of 128 and 256,
sample tiles of 32):
    43 atoms  M = 129   one ragged column tile; no multiple of any chunk      86 atoms  M = 258   the second column tile holds two columns
    171 atoms M = 513   the third column tile holds one                       512 atoms M = 1536  the bound, all tiles full
    3 atoms   M = 9     far below one tile                                    0 atoms             an empty slot
and S = 33 gives a second sample tile that holds one sample.  The kernel sums over k in the order of csrc/sample.hip's, so wherever
both serve a molecule the results are compared bitwise."""
import functools

import numpy as np
import pytest
import torch

from tests import sample_ref as sr
from tests import util
from tests.test_hip_hessian import cuda, make_model
from tests.test_hip_sampling import pack, pack_draws, per_molecule

pytestmark = pytest.mark.gpu

FIELDS = ('pos', 'amplitudes', 'harmonic_energy', 'n_skipped_imaginary', 'z', 'batch', 'cell')
LARGE_SIZES = (43, 0, 3, 86, 171, 512)
MIXED_SIZES = (3, 43, 0, 21, 86, 9)
MODES = [(False, 300.0), (True, 300.0), (True, 0.0)]       # (quantum, T): classical, Wigner, Wigner ground state


@functools.lru_cache(maxsize=None)
def _molecules(sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        M = 3 * n
        Q = np.linalg.qr(rng.standard_normal((M, M)))[0] if n else np.zeros((0, 0))
        pos = (1.5 * rng.standard_normal((n, 3))).astype(np.float32)
        m = rng.choice(np.array([1.008, 12.011, 15.999], dtype=np.float32), size=n)
        out.append(dict(n=n, lam=sr.synthetic_spectrum(n) if n else np.zeros(0, dtype=np.float32),
                        modes=np.ascontiguousarray(Q.T).astype(np.float32), pos=pos, masses=m))
    return tuple(out)


def molecules(sizes, with_masses=True, seed=13):
    """sample_ref.synthetic_molecules for other sizes: [dict(n, lam, modes, pos, masses)], seeded, built once and never modified"""
    return [dict(m, masses=m['masses'] if with_masses else None) for m in _molecules(tuple(sizes), seed)]


def same(a, b, fields=FIELDS):
    for name in fields:
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def check_against_fp64(mols, draws, thr_dev, out, S, T, quantum, tag):
    """the bounds of the module docstring for every molecule; returns the worst observed constants"""
    worst = dict(dx=0.0, q=0.0, e=0.0)
    for b, (m, xi, (pos_d, q_d, e_d)) in enumerate(zip(mols, draws, per_molecule(out, mols, S))):
        n, M = m['n'], 3 * m['n']
        if n == 0:
            assert int(out.n_skipped_imaginary[b]) == 0
            continue
        thr = float(thr_dev[b])
        ref = sr.sample(m['modes'], m['lam'], thr, m['masses'], m['pos'], xi, T, quantum)
        assert int(out.n_skipped_imaginary[b]) == ref['n_skipped']
        b_dx, b_e = sr.displacement_bound(M, ref['q'], m['masses']), sr.energy_bound(M, m['lam'], thr, ref['q'])
        b_q = sr.C_SAMPLE * M * sr.EPS32 * np.abs(ref['q']).max(axis=1)
        assert np.all(b_q > 0)
        half_ulp = 0.5 * np.spacing(np.abs(ref['pos']).astype(np.float32)).astype(np.float64)
        d_pos = np.abs(pos_d.astype(np.float64) - ref['pos'])
        d_q, d_e = np.abs(q_d - ref['q']).max(axis=1), np.abs(e_d - ref['energy'])
        c = dict(dx=float(np.max((d_pos - half_ulp).max(axis=(1, 2)) / b_dx)) * sr.C_SAMPLE, q=float(np.max(d_q / b_q)) * sr.C_SAMPLE,
                 e=float(np.max(d_e / b_e)) * sr.C_SAMPLE)
        print(f'{tag} molecule {b} (M = {M}, S = {S}, quantum {quantum}, T = {T}): observed c displacement '
              f'{max(c["dx"], 0.0):.4f}, amplitudes {c["q"]:.4f}, energy {c["e"]:.4f} (allowed {sr.C_SAMPLE})')
        assert np.all(d_pos <= b_dx[:, None, None] + half_ulp), f'molecule {b}: displacement c = {c["dx"]:.3f}'
        assert np.all(d_q <= b_q), f'molecule {b}: amplitudes c = {c["q"]:.3f}'
        assert np.all(d_e <= b_e), f'molecule {b}: harmonic energy c = {c["e"]:.3f}'
        dead = np.asarray(m['lam'], dtype=np.float64) <= thr
        assert not q_d[:, dead].any() and np.all(q_d[:, ~dead] != 0)
        for k in worst:
            worst[k] = max(worst[k], c[k])
    return worst


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('quantum,T', MODES)
@pytest.mark.parametrize('S', [1, 33])
@pytest.mark.parametrize('with_masses', [False, True])
def test_tiled_kernel_against_fp64_on_the_same_inputs(with_masses, S, quantum, T):
    mols = molecules(LARGE_SIZES, with_masses)
    draws = sr.synthetic_draws(mols, S)
    nm = pack(mols)
    out = nm.sample(S, T, quantum=quantum, xi=pack_draws(draws), kernel='tiled')
    N, B = sum(m['n'] for m in mols), len(mols)
    assert out.pos.shape == (S * N, 3) and out.harmonic_energy.shape == (B * S,) and out.amplitudes.shape == (3 * S * N,)
    assert out.n_skipped_imaginary.shape == (B,) and out.batch.shape == (S * N,) and out.cell.shape == (B * S, 3, 3)
    thr_dev = nm.threshold.cpu().numpy()
    for b, m in enumerate(mols):
        if m['n']:
            assert thr_dev[b] == sr.default_threshold(3 * m['n'], np.abs(m['lam']).max())
    worst = check_against_fp64(mols, draws, thr_dev, out, S, T, quantum, f'masses {with_masses}')
    print(f'worst observed c: displacement {worst["dx"]:.4f}, amplitudes {worst["q"]:.4f}, energy {worst["e"]:.4f}')


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('quantum', [False, True])
def test_tiled_is_bitwise_the_lds_kernel_where_both_serve(quantum):
    mols = sr.synthetic_molecules(True)                             # 1, 2, 0, 3, 9, 21, 42 atoms
    nm, xi = pack(mols), pack_draws(sr.synthetic_draws(mols, 33))
    same(nm.sample(33, 300.0, quantum=quantum, xi=xi, kernel='tiled'), nm.sample(33, 300.0, quantum=quantum, xi=xi, kernel='lds'))
    plain = pack(sr.synthetic_molecules(False))                     # unit masses
    same(plain.sample(33, 300.0, quantum=quantum, xi=xi, kernel='tiled'), plain.sample(33, 300.0, quantum=quantum, xi=xi))


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('quantum', [False, True])
def test_auto_on_a_mixed_batch(quantum):
    S = 33
    mols = molecules(MIXED_SIZES)
    draws = sr.synthetic_draws(mols, S)
    nm = pack(mols)
    auto = nm.sample(S, 300.0, quantum=quantum, xi=pack_draws(draws), kernel='auto')
    tiled = nm.sample(S, 300.0, quantum=quantum, xi=pack_draws(draws), kernel='tiled')
    small = [b for b, m in enumerate(mols) if m['n'] <= 42]         # 3, 0, 21, 9 atoms: two runs around the large molecules
    alone = pack([mols[b] for b in small]).sample(S, 300.0, quantum=quantum, xi=pack_draws([draws[b] for b in small]), kernel='lds')
    got, big, ref = per_molecule(auto, mols, S), per_molecule(tiled, mols, S), per_molecule(alone, [mols[b] for b in small], S)
    for b, m in enumerate(mols):
        want = ref[small.index(b)] if b in small else big[b]
        n_skip = alone.n_skipped_imaginary[small.index(b)] if b in small else tiled.n_skipped_imaginary[b]
        for x, y, name in zip(got[b], want, ('pos', 'amplitudes', 'harmonic_energy')):
            assert np.array_equal(x, y), (b, m['n'], name)
        assert int(auto.n_skipped_imaginary[b]) == int(n_skip), (b, m['n'])
        if m['n'] >= 3:                                             # every molecule's own count and energies, not a neighbour's
            thr = float(nm.threshold[b])
            assert int(auto.n_skipped_imaginary[b]) == int(np.count_nonzero(m['lam'] < -thr))
            assert np.all(got[b][2] > 0)
    assert len({int(x) for x in auto.n_skipped_imaginary}) > 2      # the counts differ between the molecules: a shifted one shows
    same(auto, tiled, ('z', 'batch', 'cell'))
    check_against_fp64(mols, draws, nm.threshold.cpu().numpy(), auto, S, 300.0, quantum, 'auto')


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------

def test_repeats_are_bitwise_and_a_sample_depends_on_nothing_around_it():
    mols = molecules((43, 86))
    nm = pack(mols)
    d1, d33 = sr.synthetic_draws(mols, 1), sr.synthetic_draws(mols, 33)
    for quantum in (False, True):
        a = nm.sample(33, 300.0, quantum=quantum, xi=pack_draws(d33), kernel='tiled')
        same(a, nm.sample(33, 300.0, quantum=quantum, xi=pack_draws(d33), kernel='tiled'))
        one = nm.sample(1, 300.0, quantum=quantum, xi=pack_draws(d1), kernel='tiled')
        for (p1, q1, e1), (p33, q33, e33) in zip(per_molecule(one, mols, 1), per_molecule(a, mols, 33)):
            assert np.array_equal(p1[0], p33[0]) and np.array_equal(q1[0], q33[0]) and np.array_equal(e1, e33[:1])
        assert torch.equal(one.n_skipped_imaginary, a.n_skipped_imaginary)
    # sample 32 (the second tile's only one) from a run of 33 and as the only sample of a run of its own
    full = nm.sample(33, 300.0, xi=pack_draws(d33), kernel='tiled')
    last = nm.sample(1, 300.0, xi=pack_draws([d[32:] for d in d33]), kernel='tiled')
    for (p1, q1, e1), (p33, q33, e33) in zip(per_molecule(last, mols, 1), per_molecule(full, mols, 33)):
        assert np.array_equal(p1[0], p33[32]) and np.array_equal(q1[0], q33[32]) and np.array_equal(e1, e33[32:])
    # each molecule alone in its batch
    both = per_molecule(full, mols, 33)
    for b in range(2):
        alone = pack([mols[b]]).sample(33, 300.0, xi=pack_draws([d33[b]]), kernel='tiled')
        for x, y in zip(per_molecule(alone, [mols[b]], 33)[0], both[b]):
            assert np.array_equal(x, y)
        assert int(alone.n_skipped_imaginary[0]) == int(full.n_skipped_imaginary[b])


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------

def raw_buffers(counts):
    """device arrays for a direct call of the C entry on molecules of `counts` atoms, every one filled with 7 (n_skipped: -5)"""
    n_atoms = sum(counts)
    mol_host = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    blk = np.concatenate([[0], np.cumsum([9 * n * n for n in counts])])
    f = lambda k: torch.full((k,), 7.0, device='cuda')              # noqa: E731
    return dict(mol_host=mol_host, mol_dev=mol_host.cuda(), blk_ptr=torch.tensor(blk[:-1], device='cuda'), modes=f(int(blk[-1])),
                evals=f(3 * n_atoms), thr=f(len(counts)), xi=f(3 * n_atoms), pos=f(3 * n_atoms), new_pos=f(3 * n_atoms),
                en=f(len(counts)), amp=f(3 * n_atoms), skipped=torch.full((len(counts),), -5, dtype=torch.int32, device='cuda'))


def raw_call(d, min_dim, amplitudes=True):
    from newtonnet_amd import hip
    rc = hip.lib().nnhip_mode_sample_large(d['modes'].data_ptr(), d['evals'].data_ptr(), d['blk_ptr'].data_ptr(), d['mol_dev'].data_ptr(),
                                           d['mol_host'].data_ptr(), d['mol_host'].numel() - 1, None, d['pos'].data_ptr(),
                                           d['thr'].data_ptr(), 300.0, 0, 1, d['xi'].data_ptr(), d['new_pos'].data_ptr(),
                                           d['en'].data_ptr(), d['amp'].data_ptr() if amplitudes else None, d['skipped'].data_ptr(),
                                           min_dim, hip._stream(d['modes'].device))
    torch.cuda.synchronize()
    return rc, hip.lib().nnhip_last_error().decode()


def untouched(d, rows=slice(None), mols=slice(None)):
    return all(bool((d[k][rows] == 7.0).all()) for k in ('new_pos', 'amp')) and bool((d['en'][mols] == 7.0).all()) \
        and bool((d['skipped'][mols] == -5).all())


def test_refusals_and_untouched_memory():
    from newtonnet_amd import vibrations as vib
    nm43 = pack(molecules((43,)))
    with pytest.raises(NotImplementedError, match=str(vib.max_dim())):
        nm43.sample(1, 300.0)                                       # the default kernel refuses as before
    bound = vib.max_dim_sample_large()
    n = bound // 3 + 1
    rng = np.random.default_rng(2)
    over = dict(n=n, lam=np.sort(rng.random(3 * n)).astype(np.float32), modes=np.zeros((3 * n, 3 * n), dtype=np.float32),
                pos=rng.standard_normal((n, 3)).astype(np.float32), masses=np.ones(n, dtype=np.float32))
    nm = pack([molecules((3,))[0], over])
    for kernel in ('tiled', 'auto'):
        with pytest.raises(NotImplementedError, match=f'above the {bound} the tiled'):
            nm.sample(1, 300.0, kernel=kernel)
    # the library's own check (what a C caller meets): NNHIP_E_UNSUPPORTED before any launch
    d = raw_buffers([3, n])
    rc, msg = raw_call(d, 0)
    assert rc == 2 and str(bound) in msg and 'molecule 1' in msg
    assert untouched(d)                                             # nothing ran
    rc, msg = raw_call(raw_buffers([3, 43]), 0, amplitudes=False)
    assert rc == 1 and 'amplitudes' in msg                          # NNHIP_E_INVALID
    # min_dim: a batch of small molecules only is nobody's ...
    d = raw_buffers([3, 9, 21, 42])
    rc, _ = raw_call(d, 127)
    assert rc == 0 and untouched(d)
    # ... and in a mixed batch the kernels decide per molecule on the device: 43 atoms are served, 3 and 42 left alone
    d = raw_buffers([3, 43, 42])
    d['thr'].fill_(1.0)                                             # every mode (lambda = 7) live, sigma^2 = kT / 7
    rc, _ = raw_call(d, 127)
    assert rc == 0 and untouched(d, slice(0, 9), slice(0, 1)) and untouched(d, slice(9 + 129, None), slice(2, 3))
    q = float(np.sqrt(np.float32(sr.K_BOLTZMANN * 300.0) / np.float32(7.0)) * np.float32(7.0))
    assert int(d['skipped'][1]) == 0 and torch.allclose(d['amp'][9:9 + 129], torch.full((129,), q, device='cuda'), rtol=1e-6)
    assert bool(torch.isfinite(d['new_pos'][9:9 + 129]).all()) and bool((d['new_pos'][9:9 + 129] != 7.0).all())
    assert abs(float(d['en'][1]) - 0.5 * 129 * 7.0 * q * q) <= 1e-5 * float(d['en'][1])


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------

def test_model_end_to_end_above_the_old_bound():
    from tests.test_hip_eig_large import pbc_result                 # 216 and 125 atoms through solver='auto': computed once, shared
    r = pbc_result()
    model, args, nm = r['model'], r['args'], r['nm']

    def gen(seed):
        g = torch.Generator(device='cuda')
        g.manual_seed(seed)
        return g
    a = model.sample_displacements(*args, 2, 300.0, solver='auto', generator=gen(1))
    b = model.sample_displacements(*args, 2, 300.0, solver='auto', generator=gen(1))
    same(a, b)
    N = 216 + 125
    assert a.pos.shape == (2 * N, 3) and a.z.shape == (2 * N,) and a.batch.shape == (2 * N,) and a.cell.shape == (4, 3, 3)
    assert a.harmonic_energy.shape == (4,) and a.n_skipped_imaginary.shape == (2,) and a.amplitudes.shape == (6 * N,)
    assert a.batch.tolist() == [k for k in range(2) for _ in range(216)] + [k for k in range(2, 4) for _ in range(125)]
    e = model(a.z, a.pos, a.cell, a.batch).energy
    assert e.reshape(-1).shape == (4,) and bool(torch.isfinite(e).all())
    # the kernels on the device's own modes against fp64 on copies of them
    S = 2
    xi = torch.randn(3 * N * S, generator=torch.Generator().manual_seed(5))
    out = nm.sample(S, 300.0, kernel='auto', xi=xi.cuda())
    lam, modes, masses, pos = (t.cpu().numpy() for t in (nm.eigenvalues, nm.modes, nm.masses, nm.pos))
    mols, draws, a0, q0 = [], [], 0, 0
    for n in (216, 125):
        M = 3 * n
        mols.append(dict(n=n, lam=lam[3 * a0:3 * a0 + M], modes=modes[q0:q0 + M * M].reshape(M, M), masses=masses[a0:a0 + n],
                         pos=pos[a0:a0 + n]))
        draws.append(xi[3 * S * a0:3 * S * (a0 + n)].numpy().reshape(S, M))
        a0, q0 = a0 + n, q0 + M * M
    check_against_fp64(mols, draws, nm.threshold.cpu().numpy(), out, S, 300.0, False, 'pbc_batch2_rand')


def test_calculator_samples_above_the_old_bound():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    z, pos, cell, batch, _ = util.case_inputs('aspirin8_rand', torch.float32)
    calc = MLAseCalculator(util.load_state('rand', torch.float32), properties=['energy', 'forces'], device='cuda')
    # two aspirins 6 A apart and a hydrogen atom: 43 atoms in one frame (the frame of test_hip_eig_large.py)
    p = torch.cat([pos[batch == 0], pos[batch == 1] + torch.tensor([6.0, 0.0, 0.0]), torch.tensor([[3.0, 4.0, 0.5]])])
    numbers = torch.cat([z[batch == 0], z[batch == 1], torch.tensor([1])])
    frame = FakeAtoms(numbers.numpy(), p.numpy().astype(np.float64))
    x1, x2 = calc.sample(frame, 3, 300.0, seed=3, solver='auto'), calc.sample(frame, 3, 300.0, seed=3, solver='auto')
    assert x1.shape == (3, 43, 3) and np.array_equal(x1, x2) and np.all(np.isfinite(x1))
    assert 0 < np.abs(x1 - frame.positions[None]).max()
    with pytest.raises(NotImplementedError, match='126'):
        calc.sample(frame, 3, 300.0, seed=3)
