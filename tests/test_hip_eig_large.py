"""The blocked eigensolver on the GPU (csrc/eig_large.hip; solver='auto' / 'blocked' of newtonnet_amd/vibrations.py).

The bounds are those of tests/test_hip_vibrations.py (check_solver is imported from there): against fp64 eigh of the SAME fp32
blocks after the same symmetrisation, mass-weighting and projection in fp64, with M = 3 n_b, s = ||A||_2, eps32 = 2^-24, c = 8:
    max |lambda - lambda_ref| <= c M eps32 s,   max |A v - lambda v| <= c M eps32 s,   max |V V^T - I| <= c M eps32.
check_solver prints the observed constants per molecule.  Where two solvers are compared their eigenvalues may differ by the sum of
their two bounds.  Everything else (routing, batch independence, repeatability, untouched outputs) is bitwise."""
import functools

import numpy as np
import pytest
import torch

from tests import sample_ref as sr
from tests import util
from tests import vib_ref as vr
from tests.test_hip_hessian import cuda, make_model
from tests.test_hip_vibrations import check_solver, table

pytestmark = pytest.mark.gpu

N_BIG = 43                      # the smallest molecule above the one-workgroup bound: M = 129, padded to 192 = 6 blocks of 32
TINY32 = float(np.finfo(np.float32).tiny)


@functools.lru_cache(maxsize=None)
def big_block(seed=129):
    """(H fp32 [129, 129] random symmetric, pos fp32 [43, 3]) -- seeded; never modified by a test"""
    rng = np.random.default_rng(seed)
    H = vr.random_symmetric(3 * N_BIG, rng)
    pos = (rng.standard_normal((N_BIG, 3)) * 3.0).astype(np.float32)
    return H, pos


def one_big(seed=129):
    H, pos = big_block(seed)
    return (torch.from_numpy(H.reshape(-1).copy()), torch.zeros(1, dtype=torch.long), torch.zeros(N_BIG, dtype=torch.long),
            torch.from_numpy(pos.copy()), torch.zeros(1, 3, 3))


@functools.lru_cache(maxsize=None)
def pbc_result():
    """pbc_batch2_rand (216 and 125 atoms, periodic) through the model with solver='auto': computed once, shared, left unchanged"""
    z, pos, cell, batch, _ = util.case_inputs('pbc_batch2_rand', torch.float32)
    model = make_model(util.load_state('rand'))
    args = cuda(z, pos, cell, batch)
    nm = model.normal_modes(*args, solver='auto')
    blocks, ptr = model.hessian(*args, blocks=True)
    return dict(model=model, args=args, nm=nm, blocks=blocks.cpu().double().numpy(), ptr=ptr.cpu().tolist(), z=z, pos=pos, cell=cell,
                batch=batch)


@functools.lru_cache(maxsize=None)
def mixed_blocks():
    """the device's Hessian blocks of mixed_rand (M = 63, 27, 3, 6) with the inputs they belong to"""
    sd = util.load_state('rand')
    z, pos, cell, batch, _ = util.case_inputs('mixed_rand', torch.float32)
    model = make_model(sd)
    blocks, ptr = model.hessian(*cuda(z, pos, cell, batch), blocks=True)
    return dict(z=z, pos=pos, cell=cell, batch=batch, blocks=blocks.cpu(), ptr=ptr.cpu(), masses=table(z))


def mixed_plus_big():
    """mixed_rand's molecules 0, 1 | the 43-atom synthetic one | molecules 2, 3: two runs of small molecules around the large one.
    Returns (eig_blocks arguments on the host, atom slices per molecule in the new order)"""
    m = mixed_blocks()
    H, pos_big = big_block()
    counts = torch.bincount(m['batch']).tolist()
    off = np.concatenate([[0], np.cumsum(counts)])
    boff = m['ptr'].tolist() + [m['blocks'].numel()]
    order = [0, 1, 'big', 2, 3]
    blocks, pos, masses, batch, cell, sizes = [], [], [], [], [], []
    for k, b in enumerate(order):
        if b == 'big':
            blocks.append(torch.from_numpy(H.reshape(-1).copy()))
            pos.append(torch.from_numpy(pos_big.copy()))
            masses.append(torch.ones(N_BIG))
            cell.append(torch.zeros(3, 3))
            n = N_BIG
        else:
            blocks.append(m['blocks'][boff[b]:boff[b + 1]])
            pos.append(m['pos'][off[b]:off[b + 1]])
            masses.append(m['masses'][off[b]:off[b + 1]])
            cell.append(m['cell'][b])
            n = counts[b]
        batch.append(torch.full((n,), k, dtype=torch.long))
        sizes.append(n)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([9 * n * n for n in sizes])[:-1]]), dtype=torch.long)
    return (torch.cat(blocks).contiguous(), ptr, torch.cat(batch), torch.cat(pos).contiguous(), torch.stack(cell),
            torch.cat(masses).contiguous()), sizes


def solve(host_args, **kw):
    from newtonnet_amd import vibrations as vib
    blocks, ptr, batch, pos, cell, masses = host_args
    return vib.eig_blocks(blocks.cuda(), ptr.cuda(), batch.cuda(), pos.cuda(), cell.cuda(), None if masses is None else masses.cuda(), **kw)


def same(a, b, modes=True):
    ok = torch.equal(a.eigenvalues, b.eigenvalues) and torch.equal(a.sweeps, b.sweeps) and torch.equal(a.status, b.status)
    return ok and (not modes or torch.equal(a.modes, b.modes))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('project', [False, True])
def test_smallest_size_above_the_old_bound(project):
    blocks, ptr, batch, pos, cell = one_big()
    nm = solve((blocks, ptr, batch, pos, cell, None), project=project, solver='auto')
    # check_solver: status 0, n_projected, ascending eigenvalues, the sign rule, the three bounds (constants printed)
    check_solver(nm, blocks.double().numpy(), [0], None, pos, cell, batch, None, project, f'M = {3 * N_BIG} auto')
    assert nm.n_projected.tolist() == ([6] if project else [0])
    assert nm.eigenvalues.shape == (3 * N_BIG,) and nm.molecule(0)[1].shape == (3 * N_BIG, N_BIG, 3)
    assert 1 <= int(nm.sweeps[0]) <= 30


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------

def check_bounds(nm, blocks_host, ptr_host, pos, cell, batch, masses, project, label):
    """check_solver for a model's own Hessian of a large molecule.  The same reference and the same three bounds, status,
    n_projected, ordering and sign rule.  check_solver also counts the eigenvalues inside the bound and wants exactly n_projected
    of them, which needs a spectrum with a gap above zero (its synthetic inputs are built with one).  A 216-atom periodic cell
    of a model with random weights has genuine eigenvalues inside c M eps32 s, so here that count is asserted only where the
    REFERENCE spectrum has nothing but its projected zeros within twice the bound."""
    lam_all = nm.eigenvalues.cpu().double().numpy()
    b_all = batch.cpu()
    for m in range(int(b_all.max()) + 1):
        idx = (b_all == m).nonzero().reshape(-1)
        n = idx.numel()
        M = 3 * n
        Hb = blocks_host[ptr_host[m]:ptr_host[m] + 9 * n * n].reshape(M, M)
        ref = vr.analyse(Hb, pos[idx].double().numpy(), masses[idx].double().numpy(), project=project,
                         periodic=bool(cell[m].abs().max() > 0))
        s, bound = ref['s'], vr.solver_bound(M, ref['s'])
        lam = lam_all[3 * idx[0].item():3 * idx[0].item() + M]
        V32 = nm.molecule(m)[1].cpu().numpy().reshape(M, M)
        V = V32.astype(np.float64)
        assert int(nm.status[m]) == 0, f'{label} molecule {m}: sweep cap hit ({int(nm.sweeps[m])} sweeps)'
        assert int(nm.n_projected[m]) == ref['n_proj']
        assert np.all(np.diff(lam) >= 0), 'eigenvalues are not ascending'
        assert np.all(V32[np.arange(M), np.argmax(np.abs(V32), axis=1)] > 0)
        assert s > 0
        orth = np.abs(V @ V.T - np.eye(M)).max()
        d_ev = np.abs(lam - ref['evals']).max()
        resid = np.abs(ref['A'] @ V.T - V.T * lam[None, :]).max()
        inside_ref = np.count_nonzero(np.abs(ref['evals']) <= 2 * bound)
        print(f'{label} molecule {m} (M = {M}, project {project}): sweeps {int(nm.sweeps[m])}, c eigenvalues {d_ev / (M * vr.EPS32 * s):.3f}, '
              f'c residual {resid / (M * vr.EPS32 * s):.3f}, c orthonormality {orth / (M * vr.EPS32):.3f}; reference eigenvalues within '
              f'twice the bound: {inside_ref} (n_projected {ref["n_proj"]})')
        assert orth <= vr.C_SOLVER * M * vr.EPS32, f'{label} molecule {m}: orthonormality c = {orth / (M * vr.EPS32):.2f}'
        assert d_ev <= bound, f'{label} molecule {m}: eigenvalues c = {d_ev / (M * vr.EPS32 * s):.2f}'
        assert resid <= bound, f'{label} molecule {m}: residual c = {resid / (M * vr.EPS32 * s):.2f}'
        if project and inside_ref == ref['n_proj']:
            assert np.count_nonzero(np.abs(lam) <= bound) == ref['n_proj']


def test_the_fixture_the_old_solver_refuses():
    r = pbc_result()
    nm = r['nm']
    assert nm.n_projected.tolist() == [3, 3]
    assert nm.ptr.tolist() == [0, 648, 648 + 375] and nm.ptr.dtype == torch.int64
    for b, n in enumerate((216, 125)):
        f, m = nm.molecule(b)
        assert f.shape == (3 * n,) and m.shape == (3 * n, n, 3)
    check_bounds(nm, r['blocks'], r['ptr'], r['pos'], r['cell'], r['batch'], table(r['z']), True, 'pbc_batch2_rand auto')
    assert torch.equal(r['model'].frequencies(*r['args'], solver='auto'), nm.frequencies)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------

def test_blocked_against_lds_on_mixed_rand():
    m = mixed_blocks()
    host = (m['blocks'], m['ptr'], m['batch'], m['pos'], m['cell'], m['masses'])
    lds, blk = solve(host, solver='lds'), solve(host, solver='blocked')
    assert torch.equal(lds.n_projected, blk.n_projected) and lds.n_projected.tolist() == [6, 6, 3, 5]
    bh, ph = m['blocks'].double().numpy(), m['ptr'].tolist()
    for nm, label in ((lds, 'mixed_rand lds'), (blk, 'mixed_rand blocked')):
        check_solver(nm, bh, ph, m['z'], m['pos'], m['cell'], m['batch'], m['masses'], True, label)
    counts = torch.bincount(m['batch']).tolist()
    assert [3 * n for n in counts] == [63, 27, 3, 6]
    o = 0
    for b, n in enumerate(counts):
        idx = torch.arange(o, o + n)
        ref = vr.analyse(bh[ph[b]:ph[b] + 9 * n * n].reshape(3 * n, 3 * n), m['pos'][idx].double().numpy(), m['masses'][idx].double().numpy(),
                         project=True, periodic=bool(m['cell'][b].abs().max() > 0))
        d = (lds.eigenvalues[3 * o:3 * (o + n)] - blk.eigenvalues[3 * o:3 * (o + n)]).abs().max().item()
        print(f'mixed_rand molecule {b} (M = {3 * n}): |lambda_lds - lambda_blocked| = {d:.3e}, two bounds {2 * vr.solver_bound(3 * n, ref["s"]):.3e}; '
              f'sweeps lds {int(lds.sweeps[b])}, blocked (outer) {int(blk.sweeps[b])}')
        assert d <= 2 * vr.solver_bound(3 * n, ref['s'])
        o += n
    # the single atom (M = 3, all of it projected): nothing to do
    assert int(blk.sweeps[2]) == 0 and torch.count_nonzero(blk.eigenvalues[90:93]) == 0


# ---- 4, 5 ------------------------------------------------------------------------------------------------------------------------

def test_routing_and_batch_independence():
    host, sizes = mixed_plus_big()
    assert sizes == [21, 9, N_BIG, 1, 2]
    auto = solve(host, solver='auto')
    m = mixed_blocks()
    small = solve((m['blocks'], m['ptr'], m['batch'], m['pos'], m['cell'], m['masses']), solver='lds')
    blocks, ptr, batch, pos, cell = one_big()
    alone = solve((blocks, ptr, batch, pos, cell, torch.ones(N_BIG)), solver='auto')
    assert auto.status.tolist() == [0] * 5
    # small molecules: bitwise what the one-workgroup solver gives on the small-only batch (new index -> index there)
    for new, old in ((0, 0), (1, 1), (3, 2), (4, 3)):
        fa, ma = auto.molecule(new)
        fs, ms = small.molecule(old)
        assert torch.equal(fa, fs) and torch.equal(ma, ms) and int(auto.sweeps[new]) == int(small.sweeps[old])
        assert int(auto.n_projected[new]) == int(small.n_projected[old])
    lo = 3 * (sizes[0] + sizes[1])
    assert torch.equal(auto.eigenvalues[:lo], small.eigenvalues[:lo]) and torch.equal(auto.eigenvalues[lo + 3 * N_BIG:], small.eigenvalues[lo:])
    # the large one: bitwise what it gives alone
    fa, ma = auto.molecule(2)
    fs, ms = alone.molecule(0)
    assert torch.equal(fa, fs) and torch.equal(ma, ms) and int(auto.sweeps[2]) == int(alone.sweeps[0])
    assert torch.equal(auto.eigenvalues[lo:lo + 3 * N_BIG], alone.eigenvalues) and int(auto.n_projected[2]) == 6
    # and with every molecule in the blocked solver the large one is the same again
    allb = solve(host, solver='blocked')
    assert torch.equal(allb.molecule(2)[1], ma) and torch.equal(allb.eigenvalues[lo:lo + 3 * N_BIG], alone.eigenvalues)


def test_repeatable_and_modes_false_bitwise():
    host, _ = mixed_plus_big()
    for solver in ('auto', 'blocked'):
        a, b = solve(host, solver=solver), solve(host, solver=solver)
        assert same(a, b)
        c = solve(host, solver=solver, modes=False)
        assert c.modes is None and same(a, c, modes=False) and c.molecule(2)[1] is None


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------

def two_big():
    H0, p0 = big_block(129)
    H1, p1 = big_block(130)
    blocks = torch.from_numpy(np.concatenate([H0.reshape(-1), H1.reshape(-1)]))
    ptr = torch.tensor([0, 9 * N_BIG * N_BIG])
    batch = torch.cat([torch.zeros(N_BIG, dtype=torch.long), torch.ones(N_BIG, dtype=torch.long)])
    return blocks, ptr, batch, torch.from_numpy(np.concatenate([p0, p1])), torch.zeros(2, 3, 3)


def test_status_bits():
    from newtonnet_amd import hip
    blocks, ptr, batch, pos, cell = two_big()
    M = 3 * N_BIG
    good = solve((blocks, ptr, batch, pos, cell, None), solver='auto')
    assert good.status.tolist() == [0, 0]
    # one NaN: that molecule runs to the cap and says so; its neighbour is what it was
    bad = blocks.clone()
    bad[5 * M + 77] = float('nan')
    nm = solve((bad, ptr, batch, pos, cell, None), solver='auto')
    assert nm.status.tolist() == [1, 0] and nm.sweeps.tolist() == [30, int(good.sweeps[1])]
    assert torch.equal(nm.eigenvalues[M:], good.eigenvalues[M:]) and torch.equal(nm.molecule(1)[1], good.molecule(1)[1])
    # a zero mass in molecule 1: bit 2, nothing of it computed
    masses = torch.ones(2 * N_BIG)
    masses[N_BIG + 7] = 0.0
    nm = solve((blocks, ptr, batch, pos, cell, masses), solver='auto')
    assert nm.status.tolist() == [0, 4]
    assert torch.count_nonzero(nm.eigenvalues[M:]) == 0 and torch.count_nonzero(nm.molecule(1)[1]) == 0
    assert torch.equal(nm.eigenvalues[:M], good.eigenvalues[:M])
    # the C entry with a mol_ptr that claims more atoms (50) for molecule 1 than mol_ptr_host (43): skipped with bit 1
    L = hip.lib()
    mol_host = torch.tensor([0, N_BIG, 2 * N_BIG], dtype=torch.int32)
    mol_dev = torch.tensor([0, N_BIG, N_BIG + 50], dtype=torch.int32, device='cuda')
    bd, pd_, posd, celld = blocks.cuda(), ptr.cuda(), torch.zeros(N_BIG + 50, 3, device='cuda'), cell.cuda()
    ev = torch.full((3 * (N_BIG + 50),), 7.0, device='cuda')
    ints = torch.full((6,), -1, dtype=torch.int32, device='cuda')
    ws_bytes = int(L.nnhip_eig_large_ws_bytes(mol_host.data_ptr(), 2, 0))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    rc = L.nnhip_eig_blocks_large(bd.data_ptr(), pd_.data_ptr(), mol_dev.data_ptr(), mol_host.data_ptr(), 2, posd.data_ptr(),
                                  celld.data_ptr(), None, 0, ev.data_ptr(), None, ints[0:2].data_ptr(), ints[2:4].data_ptr(),
                                  ints[4:6].data_ptr(), None, ws.data_ptr(), ws_bytes, hip._stream(bd.device))
    torch.cuda.synchronize()
    assert rc == 0 and ints[4:6].tolist() == [0, 2]
    assert bool((ev[M:] == 7.0).all()) and torch.equal(ev[:M], solve((blocks, ptr, batch, pos, cell, None), solver='auto', project=False).eigenvalues[:M])


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------

def test_refusal_above_the_large_bound():
    from newtonnet_amd import hip
    from newtonnet_amd import vibrations as vib
    bound = vib.max_dim_large()
    assert bound >= 1536
    n = bound // 3 + 1
    blocks = torch.zeros(9 * n * n + 81, device='cuda')
    ptr = torch.tensor([0, 81], device='cuda')
    batch = torch.cat([torch.zeros(3, dtype=torch.long), torch.ones(n, dtype=torch.long)]).cuda()
    pos, cell = torch.randn(n + 3, 3, device='cuda'), torch.zeros(2, 3, 3, device='cuda')
    for solver in ('auto', 'blocked'):
        with pytest.raises(NotImplementedError, match=f'above the {bound} the blocked'):
            vib.eig_blocks(blocks, ptr, batch, pos, cell, solver=solver)
    L = hip.lib()
    mol_host = torch.tensor([0, 3, 3 + n], dtype=torch.int32)
    mol_dev = mol_host.cuda()
    ev = torch.full((3 * (n + 3),), 7.0, device='cuda')
    ints = torch.full((6,), -1, dtype=torch.int32, device='cuda')
    ws = torch.full((1 << 20,), 9, dtype=torch.uint8, device='cuda')
    rc = L.nnhip_eig_blocks_large(blocks.data_ptr(), ptr.data_ptr(), mol_dev.data_ptr(), mol_host.data_ptr(), 2, pos.data_ptr(),
                                  cell.data_ptr(), None, 1, ev.data_ptr(), None, ints[0:2].data_ptr(), ints[2:4].data_ptr(),
                                  ints[4:6].data_ptr(), None, ws.data_ptr(), ws.numel(), hip._stream(blocks.device))
    msg = L.nnhip_last_error().decode()
    assert rc == 2 and str(bound) in msg and 'molecule 1' in msg
    torch.cuda.synchronize()
    assert bool((ev == 7.0).all()) and bool((ints == -1).all()) and bool((ws == 9).all())          # nothing ran


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------

def test_downstream_quantities_on_the_large_result():
    from newtonnet_amd import vibrations as vib
    nm = pbc_result()['nm']
    lam_all = nm.eigenvalues.cpu().double().numpy()
    thr = nm.threshold.cpu().numpy()
    t300 = nm.thermochemistry(300.0)
    got = {k: getattr(t300, k).cpu().numpy() for k in ('U', 'S', 'F', 'Cv')}
    for b, (lo, hi) in enumerate(((0, 648), (648, 1023))):
        lam, M = lam_all[lo:hi], hi - lo
        assert int(nm.n_imaginary[b]) == np.count_nonzero(lam < -float(thr[b]))
        zero = sr.thermochemistry(lam, float(thr[b]), 0.0)
        err, lim = abs(float(nm.zero_point_energy[b]) - zero['U']), sr.C_SAMPLE * M * sr.EPS32 * zero['U_abs']
        print(f'molecule {b} (M = {M}): zero-point energy {zero["U"]:.6e} eV, observed c {err / max(lim, 1e-300) * sr.C_SAMPLE:.4f}, '
              f'n_imaginary {int(nm.n_imaginary[b])}')
        assert err <= lim + TINY32
        ref = sr.thermochemistry(lam, float(thr[b]), 300.0)
        for k in ('U', 'S', 'F', 'Cv'):
            err, lim = abs(float(got[k][b]) - ref[k]), sr.C_SAMPLE * M * sr.EPS32 * ref[k + '_abs']
            print(f'molecule {b} {k} = {ref[k]:.6e}, observed c {err / max(lim, 1e-300) * sr.C_SAMPLE:.4f}')
            assert err <= lim + TINY32
    # sampling stays with the one-workgroup bound: its kernel stages the mode matrix in LDS
    with pytest.raises(NotImplementedError, match=str(vib.max_dim())):
        nm.sample(1, 300.0)
    assert nm.cartesian(1).shape == (375, 125, 3)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------

def test_calculator_vibrations_above_the_old_bound():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    z, pos, cell, batch, _ = util.case_inputs('aspirin8_rand', torch.float32)
    sd = util.load_state('rand', torch.float32)
    calc = MLAseCalculator(sd, properties=['energy', 'forces'], device='cuda')
    # two aspirins 6 A apart and a hydrogen atom: 43 atoms in one frame
    p = torch.cat([pos[batch == 0], pos[batch == 1] + torch.tensor([6.0, 0.0, 0.0]), torch.tensor([[3.0, 4.0, 0.5]])])
    numbers = torch.cat([z[batch == 0], z[batch == 1], torch.tensor([1])])
    frame = FakeAtoms(numbers.numpy(), p.numpy().astype(np.float64))
    f, m = calc.vibrations(frame, solver='auto')
    assert f.shape == (129,) and m.shape == (129, 43, 3) and f.dtype == np.float32 and np.all(np.isfinite(f))
    with pytest.raises(NotImplementedError, match='126'):
        calc.vibrations(frame)
