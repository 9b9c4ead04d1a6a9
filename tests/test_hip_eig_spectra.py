"""The batched Jacobi solver (csrc/eig.hip) through vibrations.eig_blocks on SYNTHETIC blocks: every size in one launch, the
spectra and scales a Jacobi sweep meets worst, the Gram-Schmidt drop rule of the projection, an empty molecule slot and status
bit 0.  The physical Hessians of tests/test_hip_vibrations.py reach none of these.

Blocks are built in fp64 on the host (seeded, tests/vib_ref.py), rounded ONCE to fp32, and judged by check_solver of
tests/test_hip_vibrations.py against vib_ref.analyse on those same fp32 blocks, with that module's bounds (c M eps32 s, c = 8)."""
import numpy as np
import pytest
import torch

from tests import vib_ref as vr
from tests.test_hip_vibrations import check_solver

pytestmark = pytest.mark.gpu


def pack(mats, pos_list, periodic=False):
    """blocks fp32 [sum M^2], ptr int64 [B], batch [N], pos fp32 [N,3], cell [B,3,3] of one batch (host tensors)"""
    sizes = [p.shape[0] for p in pos_list]
    for A, n in zip(mats, sizes):
        assert A.shape == (3 * n, 3 * n) and A.dtype == np.float32
    blocks = torch.from_numpy(np.concatenate([A.reshape(-1) for A in mats] or [np.zeros(0, np.float32)]))
    sq = torch.tensor([9 * n * n for n in sizes], dtype=torch.long)
    ptr = torch.cumsum(sq, 0) - sq
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    pos = torch.from_numpy(np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1, 3) for p in pos_list]))
    cell = torch.zeros(len(sizes), 3, 3)
    if periodic:
        cell[:] = 30.0 * torch.eye(3)
    return blocks, ptr, batch, pos, cell


def solve(packed, masses=None, project=False):
    from newtonnet_amd import vibrations as vib
    blocks, ptr, batch, pos, cell = packed
    return vib.eig_blocks(blocks.cuda(), ptr.cuda(), batch.cuda(), pos.cuda(), cell.cuda(),
                          None if masses is None else masses.cuda(), project=project)


def judge(nm, packed, masses, project, label):
    blocks, ptr, batch, pos, cell = packed
    return check_solver(nm, blocks.double().numpy(), ptr.tolist(), None, pos, cell, batch, masses, project, label)


def of_molecule(nm, packed, m):
    """(eigenvalues, modes, sweeps, status, n_projected) of molecule m as host tensors"""
    blocks, ptr, batch, pos, cell = packed
    idx = (batch == m).nonzero().reshape(-1)
    n = idx.numel()
    o = 3 * int(idx[0]) if n else 0
    q = int(ptr[m])
    return (nm.eigenvalues[o:o + 3 * n].cpu(), nm.modes[q:q + 9 * n * n].cpu(), int(nm.sweeps[m]), int(nm.status[m]),
            int(nm.n_projected[m]))


def one_block(A, seed=0):
    n = A.shape[0] // 3
    return pack([A], [np.random.default_rng(seed).standard_normal((n, 3)) * 3.0])


@pytest.mark.parametrize('masses_project', ['unit_free', 'mixed_projected'])
def test_every_size_in_one_launch_and_in_any_order(masses_project):
    """42 molecules of 1 .. 42 atoms (M = 3 .. 126, odd and even interleaved: an odd M idles on the padding index) in ONE launch,
    whose LDS carve-up is sized by the largest molecule while each molecule strides by its own Mp.  Once in ascending and once in
    shuffled order -- other blk_ptr / mol_ptr and another workgroup for the largest molecule: per molecule the eigenvalues, sweeps
    and modes must be bitwise the same."""
    project = masses_project == 'mixed_projected'
    sizes, mats, poss, m_np = vr.every_size_batch(project)
    m_of = [torch.from_numpy(m) if project else None for m in m_np]
    results = {}
    for order_name, order in (('ascending', list(range(42))), ('shuffled', list(np.random.default_rng(7).permutation(42)))):
        packed = pack([mats[k] for k in order], [poss[k] for k in order])
        masses = torch.cat([m_of[k] for k in order]) if project else None
        nm = solve(packed, masses, project)
        worst = judge(nm, packed, masses, project, f'{masses_project} {order_name}')
        print(f'{masses_project} {order_name}: worst constants {worst}')
        results[order_name] = {k: of_molecule(nm, packed, slot) for slot, k in enumerate(order)}
        assert int(nm.sweeps.max()) < 30 and nm.status.tolist() == [0] * 42
        if project:
            want = [3 if sizes[k] == 1 else 5 if sizes[k] == 2 else 6 for k in order]
            assert nm.n_projected.tolist() == want
    for k in range(42):
        a, b = results['ascending'][k], results['shuffled'][k]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:], f'molecule of {sizes[k]} atoms depends on its slot'


@pytest.mark.parametrize('M', [63, 126])
def test_hard_spectra(M):
    """Exact and near degeneracies, rank one, a graded spectrum, a negative definite matrix, matrices that are already diagonal
    (0 sweeps: the sort path alone) and 2 x 2 couplings of 1e-30 of the diagonal gap, where tau^2 overflows and the rotation
    must be the identity.  (With EVERY coupling that small the matrix meets the stopping rule before any sweep, so a second
    matrix mixes them with ordinary couplings: the sweeps run and the overflow branch is taken.)  Unit masses, no projection,
    all of them in one launch."""
    cases = vr.hard_spectra(M)
    names = list(cases)
    rng = np.random.default_rng(M)
    packed = pack([cases[k][2] for k in names], [rng.standard_normal((M // 3, 3)) * 3.0 for _ in names])
    nm = solve(packed)
    assert bool(torch.isfinite(nm.eigenvalues).all()) and bool(torch.isfinite(nm.modes).all())
    worst = judge(nm, packed, None, False, f'hard spectra M = {M}')
    print(f'hard spectra M = {M}: worst constants {worst}')
    got = {k: of_molecule(nm, packed, slot) for slot, k in enumerate(names)}
    for k in names:
        lam, _, A32 = cases[k]
        print(f'M = {M} {k}: sweeps {got[k][2]}')
        if lam is not None:    # the planted spectrum, through the rounding of A to fp32 (Weyl: ||A32 - A64||_2) and the solver bound
            s = np.abs(lam).max()
            lim = np.linalg.norm(A32.astype(np.float64) - cases[k][1], 2) + vr.solver_bound(M, s)
            assert np.abs(got[k][0].double().numpy() - lam).max() <= lim
    ev, modes, sweeps, _, _ = got['equal']
    assert sweeps == 0 and torch.equal(ev, torch.full((M,), 2.0)) and torch.equal(modes.view(M, M), torch.eye(M))
    ev, modes, sweeps, _, _ = got['diagonal_descending']
    assert sweeps == 0 and torch.equal(ev, torch.arange(1, M + 1).float())
    assert torch.equal(modes.view(M, M), torch.eye(M).flip(0))          # a permutation, every sign positive
    ev, modes, sweeps, _, _ = got['tiny_coupling']
    assert sweeps == 0 and torch.equal(ev, torch.from_numpy(np.diag(cases['tiny_coupling'][2]).copy()))
    assert got['tiny_and_plain_coupling'][2] >= 1
    assert (got['negative'][0] < 0).all()


def test_powers_of_two_scale_exactly():
    """The same random block x 2^k: every operation of the kernel is exact under a power-of-two scale away from denormals (the
    rotation angles are ratios, the stopping rule is homogeneous), so eigenvalues are exactly 2^k times those of k = 0 and the
    modes and sweep counts are bitwise the same."""
    M = 63
    A = vr.random_symmetric(M, np.random.default_rng(11))
    ks = [-60, -20, 0, 20, 40]
    mats = [(A * np.float32(2.0) ** k).astype(np.float32) for k in ks]
    for k, B in zip(ks, mats):
        assert np.array_equal(B.astype(np.float64), A.astype(np.float64) * 2.0 ** k)
    pos = np.random.default_rng(12).standard_normal((M // 3, 3))
    packed = pack(mats, [pos] * len(ks))
    nm = solve(packed)
    judge(nm, packed, None, False, 'scaled')
    base = of_molecule(nm, packed, ks.index(0))
    for slot, k in enumerate(ks):
        ev, modes, sweeps, status, _ = of_molecule(nm, packed, slot)
        assert torch.equal(ev.double(), base[0].double() * 2.0 ** k), f'k = {k}'
        assert torch.equal(modes, base[1]) and sweeps == base[2] and status == 0, f'k = {k}'


@pytest.mark.parametrize('periodic', [False, True])
def test_projection_drop_rule(periodic):
    """Collinear atoms along (1, 2, 2)/3, bent a decade or more either side of EIG_DROP_TOL, and a planar molecule
    (vib_ref.drop_rule_molecules): n_projected as stated there, equal to the yardstick's, and that many zero eigenvalues."""
    mols = vr.drop_rule_molecules()
    rng = np.random.default_rng(5)
    m_np = [np.array(([15.999, 1.008] * 2)[:p.shape[0]], dtype=np.float32) for _, p, _ in mols]
    packed = pack([vr.gapped_symmetric(p.shape[0], rng, m) for (_, p, _), m in zip(mols, m_np)], [p for _, p, _ in mols], periodic)
    masses = torch.from_numpy(np.concatenate(m_np))
    nm = solve(packed, masses, True)
    print('n_projected', dict(zip([k for k, _, _ in mols], nm.n_projected.tolist())))
    assert nm.n_projected.tolist() == [3 if periodic else n for _, _, n in mols]
    judge(nm, packed, masses, True, f'drop rule periodic {periodic}')


def test_empty_molecule_slots():
    """a batch whose second and last slots hold no atoms: their outputs stay zero, the others are what they are alone"""
    rng = np.random.default_rng(3)
    mats = [vr.gapped_symmetric(9, rng), np.zeros((0, 0), np.float32), vr.gapped_symmetric(5, rng), np.zeros((0, 0), np.float32)]
    poss = [rng.standard_normal((9, 3)), np.zeros((0, 3)), rng.standard_normal((5, 3)), np.zeros((0, 3))]
    packed = pack(mats, poss)
    nm = solve(packed, None, True)
    judge(nm, packed, None, True, 'empty slots')
    assert nm.n_projected.tolist() == [6, 0, 6, 0] and nm.sweeps[[1, 3]].tolist() == [0, 0] and nm.status.tolist() == [0] * 4
    assert nm.n_imaginary[[1, 3]].tolist() == [0, 0] and nm.zero_point_energy[[1, 3]].tolist() == [0.0, 0.0]
    f, m = nm.molecule(1)
    assert f.numel() == 0 and m.numel() == 0 and m.shape == (0, 0, 3)
    alone = pack([mats[2]], [poss[2]])
    one = solve(alone, None, True)
    assert torch.equal(of_molecule(nm, packed, 2)[0], of_molecule(one, alone, 0)[0])


@pytest.mark.parametrize('project', [False, True])
def test_non_finite_blocks_set_status_and_leave_the_other_molecules_alone(project):
    """A NaN in one molecule's block and an Inf in another's: 30 sweeps at most (the sweep loop is bounded whatever the data),
    then status bit 0 -- a matrix with a non-finite norm never counts as converged.  Every other molecule of the batch is bitwise
    what the clean batch gives.  Nothing else is asserted of the two bad molecules."""
    rng = np.random.default_rng(9)
    sizes = [4, 7, 3, 9, 5]
    mats = [vr.random_symmetric(3 * n, rng) for n in sizes]
    poss = [rng.standard_normal((n, 3)) * 2.0 for n in sizes]
    clean = pack(mats, poss)
    good = solve(clean, None, project)
    bad = [A.copy() for A in mats]
    bad[1][5, 2] = np.nan
    bad[3][4, 4] = np.inf
    dirty = pack(bad, poss)
    nm = solve(dirty, None, project)
    status = nm.status.tolist()
    print(f'project {project}: status {status}, sweeps {nm.sweeps.tolist()}')
    assert status[1] != 0 and status[3] != 0
    assert max(nm.sweeps.tolist()) <= 30
    for m in (0, 2, 4):
        a, b = of_molecule(nm, dirty, m), of_molecule(good, clean, m)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]
