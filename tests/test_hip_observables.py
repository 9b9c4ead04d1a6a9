"""Trajectory observables on the HIP path (newtonnet_amd/observables.py, csrc/observables.hip).

Histogram: the counts must EQUAL the fp32 statement of tests/observables_ref.py (the neighbour list's pair_disp, bin edges as thresholds
on r2), on a batch that mixes system sizes around the 64-atom tile, cell forms, species selections, bin counts and per-frame cells;
pairs at the floats either side of every edge; additivity over blocks and repeatability.  Correlations: against the fp64 statement on
the same fp32 inputs within 4 x 2^-24 x A, A = sum |term| (each term carries at most 3 fp32 roundings), bitwise repeatable, added to.
End to end: the Trajectory methods give what the classes give on the recorded tensors, NPT with the cell of every frame."""
import numpy as np
import pytest
import torch

from tests import observables_ref as R
from tests import util
from tests.test_hip_hessian import cuda, make_model, mol_subset
from tests.test_observables_host import DIAGONAL, SYMMETRIC

pytestmark = pytest.mark.gpu

f32 = np.float32
U = 2.0 ** -24


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. counts against the fp32 statement ---------------------------------------------------------------------------------------

SIZES = (1, 2, 63, 0, 64, 65, 130)          # around the kernel's 64-atom i / j tile, two and three tiles, an empty system
CELLS = ('none', 'diagonal', 'symmetric', 'diagonal', 'none', 'diagonal', 'symmetric')
Z_POOL = np.array([1, 6, 8, 7])
R_MAX = 5.5


def _batch(n_frames, seed):
    """(z, batch, mol_ptr, pos [F,N,3], cell [F,B,3,3]): unwrapped positions; the cells breathe from frame to frame"""
    rng = np.random.default_rng(seed)
    B, N = len(SIZES), sum(SIZES)
    mol_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    batch = np.repeat(np.arange(B), SIZES)
    z = rng.choice(Z_POOL, N)
    base = np.stack([{'none': np.zeros((3, 3), f32), 'diagonal': DIAGONAL, 'symmetric': SYMMETRIC}[c] for c in CELLS])
    cell = np.stack([(base.astype(np.float64) * (1.0 + 0.01 * f)).astype(f32) for f in range(n_frames)])
    pos = np.zeros((n_frames, N, 3), f32)
    for f in range(n_frames):
        for b in range(B):
            s, e = mol_ptr[b], mol_ptr[b + 1]
            if CELLS[b] == 'none':
                pos[f, s:e] = rng.uniform(-4.0, 4.0, (e - s, 3))                # a ball of pairs inside and outside r_max
            else:
                pos[f, s:e] = rng.uniform(-1.0, 2.0, (e - s, 3)) @ cell[f, b].astype(np.float64)
    return z, batch, mol_ptr, pos, cell


@pytest.mark.parametrize('n_frames', [1, 3])
@pytest.mark.parametrize('n_bins', [1, 7, 300])
@pytest.mark.parametrize('species', [[1], [6, 1], [8, 1, 6]])
def test_counts_equal_the_fp32_statement(species, n_bins, n_frames):
    from newtonnet_amd import observables as ob
    z, batch, mol_ptr, pos, cell = _batch(n_frames, 11)
    S = len(species)
    kind = np.full(len(z), -1, np.int32)
    for k, s in enumerate(species):
        kind[z == s] = k
    assert (kind < 0).any() and all((kind == k).any() for k in range(S))
    want, (_, _, tie) = R.histogram(pos, cell, mol_ptr, kind, S, R_MAX, n_bins, with_pairs=True)
    assert tie.sum() == 0                            # no pair's image hangs on the last bit of a general cell's inverse
    t = [torch.from_numpy(x).cuda() for x in (z, batch, pos, cell)]
    rdf = ob.RadialDistribution(t[0], t[1], R_MAX, n_bins, cell=t[3][0], species=species)
    assert rdf.pairs == [(species[a], species[b]) for a in range(S) for b in range(a, S)]
    rdf.add(t[2], t[3])
    got = _np(rdf.counts)
    print(f'S {S}, {n_bins} bins, {n_frames} frames: {int(want.sum())} pairs counted, {int((got != want).sum())} counters differ')
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert want.sum() > 100 * n_frames and not got[3].any() and not got[0].any()         # the empty and the one-atom system
    assert rdf.n_frames == n_frames
    vol = np.abs(np.linalg.det(cell.astype(np.float64))).mean(0)
    assert np.allclose(_np(rdf.mean_volume), vol, rtol=1e-12)
    g = _np(rdf.g())
    assert np.isnan(g[[0, 4]]).all() and np.isfinite(g[[2, 5, 6]]).all()
    if n_frames == 1:   # one frame [N,3] with the constructor's cell is the same call
        one = ob.RadialDistribution(t[0], t[1], R_MAX, n_bins, cell=t[3][0], species=species).add(t[2][0])
        assert torch.equal(one.counts, rdf.counts)


def test_pairs_at_the_floats_either_side_of_every_edge():
    """Two atoms on the x axis, one system per pair, no cell: r2 = fl(x x).  x_hi = the smallest float with fl(x x) >= edge2[k] lands in
    bin k (k = n_bins: not counted), the float below it in bin k - 1; coincident atoms land in bin 0."""
    from newtonnet_amd import observables as ob
    r_max, n_bins = 3.5, 7
    _, edge2 = R.bin_table(r_max, n_bins)
    xs, want_bin, exact = [f32(0)], [0], 0
    for k in range(1, n_bins + 1):
        x = f32(np.sqrt(edge2[k]))
        while f32(x * x) >= edge2[k]:
            x = np.nextafter(x, f32(0))
        while f32(x * x) < edge2[k]:
            x = np.nextafter(x, f32(np.inf))
        below = np.nextafter(x, f32(0))
        assert f32(x * x) >= edge2[k] > f32(below * below)
        exact += int(f32(x * x) == edge2[k])
        xs += [x, below]
        want_bin += [k if k < n_bins else -1, k - 1]
    print(f'{exact} of {n_bins} edges are met exactly by a square')
    B = len(xs)
    pos = np.zeros((B, 2, 3), f32)
    pos[:, 1, 0] = xs
    pos[:, :, 1:] = f32(1.25)               # (equal y and z: they cancel exactly)
    want = np.zeros((B, 1, n_bins), np.int64)
    for b, k in enumerate(want_bin):
        if k >= 0:
            want[b, 0, k] = 1
    mol_ptr = np.arange(0, 2 * B + 1, 2)
    assert np.array_equal(want, R.histogram(pos.reshape(1, -1, 3), np.zeros((B, 3, 3), f32), mol_ptr, np.zeros(2 * B, np.int32), 1,
                                            r_max, n_bins))
    z = torch.ones(2 * B, dtype=torch.long, device='cuda')
    batch = torch.arange(B, device='cuda').repeat_interleave(2)
    rdf = ob.RadialDistribution(z, batch, r_max, n_bins).add(torch.from_numpy(pos.reshape(-1, 3)).cuda())
    assert np.array_equal(_np(rdf.counts), want)


def test_blocks_add_up_and_calls_repeat():
    from newtonnet_amd import observables as ob
    z, batch, _, pos, cell = _batch(5, 12)
    z, batch, pos, cell = (torch.from_numpy(x).cuda() for x in (z, batch, pos, cell))
    whole = ob.RadialDistribution(z, batch, R_MAX, 300).add(pos, cell)
    again = ob.RadialDistribution(z, batch, R_MAX, 300).add(pos, cell)
    parts = ob.RadialDistribution(z, batch, R_MAX, 300).add(pos[:3], cell[:3]).add(pos[3:], cell[3:])
    assert torch.equal(whole.counts, again.counts)
    assert torch.equal(whole.counts, parts.counts) and parts.n_frames == 5
    assert torch.allclose(whole.mean_volume, parts.mean_volume, rtol=1e-14)       # (fp64 sums of five volumes, grouped differently)
    again.add(pos, cell)
    assert torch.equal(again.counts, 2 * whole.counts)                       # counts is added to


def test_the_library_refuses_what_its_histogram_cannot_hold():
    from newtonnet_amd import hip
    pos = torch.zeros(1, 4, 3, device='cuda')
    ptr = torch.tensor([0, 4], dtype=torch.int32, device='cuda')
    kind = torch.zeros(4, dtype=torch.int32, device='cuda')
    cell = torch.zeros(1, 3, 3, device='cuda')
    L = hip.lib()
    args = lambda S, nb: (pos.data_ptr(), 12, 1, cell.data_ptr(), 0, ptr.data_ptr(), 1, 4, 4, kind.data_ptr(), S,    # noqa: E731
                          torch.zeros(nb + 1, device='cuda').data_ptr(), nb,
                          torch.zeros(S * (S + 1) // 2 * nb, dtype=torch.int64, device='cuda').data_ptr(), None)
    for S, nb in ((9, 10), (1, 4097), (8, 456)):
        assert L.nnhip_rdf_accumulate(*args(S, nb)) == 1                     # NNHIP_E_INVALID, nothing launched
        assert b'LDS histogram' in L.nnhip_last_error()
    x = torch.zeros(5, 4, 3, device='cuda')
    sums = torch.zeros(1, 1, 6, dtype=torch.float64, device='cuda')
    bad = dict(lag=(5, 1, 0), every=(2, 0, 0), mode=(2, 1, 2))
    for lag, every, mode in bad.values():
        assert L.nnhip_time_correlation(x.data_ptr(), 12, 5, ptr.data_ptr(), 1, 4, kind.data_ptr(), 1, None, mode, lag, every,
                                        sums.data_ptr(), None) == 1
    torch.cuda.synchronize()
    assert not sums.any()


# ---- 2. correlations against fp64 ------------------------------------------------------------------------------------------------

TC_SIZES = (1, 5, 70)


def _frames(n_frames, seed):
    rng = np.random.default_rng(seed)
    N = sum(TC_SIZES)
    mol_ptr = np.concatenate([[0], np.cumsum(TC_SIZES)]).astype(np.int32)
    x = rng.standard_normal((n_frames, N, 3)).astype(f32)
    kind = rng.integers(0, 2, N).astype(np.int32)
    kind[0] = 1
    kind[7] = -1                                   # one atom of no kind
    w = rng.uniform(1.0, 16.0, N).astype(f32)
    return mol_ptr, x, kind, w


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n_frames, max_lag, every', [(37, 12, 1), (37, 12, 5), (150, 70, 3)])
def test_correlations_against_the_fp64_statement(n_frames, max_lag, every, mode, weighted):
    """(150, 70, 3): more than one origin block of 64 frames and two tiles of 64 lags"""
    from newtonnet_amd import hip
    mol_ptr, x, kind, w = _frames(n_frames, 21)
    want, A = R.correlation(x, mol_ptr, kind, 2, mode, max_lag, every, w if weighted else None)
    xt, pt, kt = torch.from_numpy(x).cuda(), torch.from_numpy(mol_ptr).cuda(), torch.from_numpy(kind).cuda()
    wt = torch.from_numpy(w).cuda() if weighted else None
    B = len(TC_SIZES)
    sums = torch.zeros(B, 2, max_lag + 1, dtype=torch.float64, device='cuda')
    hip.time_correlation(xt, pt, kt, 2, mode, max_lag, sums, origin_every=every, weight=wt)
    got = _np(sums)
    err, bound = np.abs(got - want), 4.0 * U * A
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f'F {n_frames}, L {max_lag}, every {every}, mode {mode}, weights {weighted}: worst err / bound {ratio:.4f}')
    assert np.all(err <= bound)
    assert np.abs(want).max() > 1.0 and not got[0, 0].any()                  # system 0 has one atom, of kind 1
    second = torch.zeros_like(sums)
    hip.time_correlation(xt, pt, kt, 2, mode, max_lag, second, origin_every=every, weight=wt)
    assert torch.equal(sums.view(torch.int64), second.view(torch.int64))      # bitwise repeatable
    hip.time_correlation(xt, pt, kt, 2, mode, max_lag, second, origin_every=every, weight=wt)
    assert torch.equal(second, 2 * sums)                                      # added to
    # frames with a stride: a view into a wider recording gives the same bits
    wide = torch.zeros(n_frames, x.shape[1] + 3, 3, device='cuda')
    wide[:, :x.shape[1]] = xt
    third = torch.zeros_like(sums)
    hip.time_correlation(wide[:, :x.shape[1]], pt, kt, 2, mode, max_lag, third, origin_every=every, weight=wt)
    assert torch.equal(third, sums)


def test_exact_cases():
    """x = v t with v and the frame spacing powers of two: every difference, square and sum is exact, MSD(l) = |v|^2 (l h)^2.
    Constant velocities: a flat autocorrelation."""
    from newtonnet_amd import observables as ob
    from newtonnet_amd.dynamics import FS
    n_frames, L, h = 40, 15, 0.5
    v = np.array([[0.5, 0.25, 1.0], [2.0, -0.5, 0.125], [-1.0, 4.0, 0.25], [0.5, 0.25, 1.0], [2.0, -0.5, 0.125]], f32)
    z = torch.tensor([1, 8, 8, 1, 8], device='cuda')
    batch = torch.tensor([0, 0, 0, 1, 1], device='cuda')
    t = np.arange(n_frames, dtype=f32)[:, None, None] * f32(h)
    x = torch.from_numpy((v[None] * t).astype(f32)).cuda()
    msd = ob.mean_squared_displacement(x, z, batch, 2.0, L, origin_every=3)
    assert msd.species == [1, 8] and msd.time.tolist() == [2.0 * l for l in range(L + 1)]
    v2 = (v.astype(np.float64) ** 2).sum(1)
    want = np.array([[v2[0], (v2[1] + v2[2]) / 2], [v2[3], v2[4]]])[:, :, None] * (np.arange(L + 1) * h) ** 2
    assert np.array_equal(_np(msd.msd), want)
    assert msd.n_origins.tolist() == [len(range(0, n_frames - l, 3)) for l in range(L + 1)]
    vel = torch.from_numpy(np.broadcast_to(v[None], (n_frames, 5, 3)).copy()).cuda()
    vacf = ob.velocity_autocorrelation(vel, z, batch, 2.0, L)
    c = _np(vacf.vacf)
    assert np.array_equal(c, np.broadcast_to(c[:, :, :1], c.shape)) and np.all(_np(vacf.normalized) == 1.0)
    assert np.allclose(c[:, :, 0], want[:, :, 1] / h ** 2 * FS * FS, rtol=1e-15)
    assert np.allclose(_np(vacf.diffusion()), c[:, :, 0] * L * 2.0 / 3.0, rtol=1e-14)
    # a second block averages in: the same block again leaves the mean where it was
    assert torch.equal(msd.add(x).msd, torch.from_numpy(want).cuda())


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------

def test_trajectory_methods_on_four_aspirins():
    from newtonnet_amd import observables as ob
    z, pos, cell, batch = cuda(*mol_subset(*util.case_inputs('aspirin8_rand', torch.float32)[:4], [0, 1, 2, 3]))
    model = make_model(util.load_state('rand'))
    dyn = model.dynamics(z, pos, cell, batch, temperature=300.0, timestep=0.5, generator=torch.Generator(device='cuda').manual_seed(3))
    traj = dyn.run(20, record_every=2)
    assert traj.pos.shape == (10, 84, 3)
    rdf = traj.radial_distribution(6.0, 120)
    assert isinstance(rdf, ob.RadialDistribution) and rdf.n_frames == 10 and rdf.pairs == [(1, 1), (1, 6), (1, 8), (6, 6), (6, 8), (8, 8)]
    direct = ob.RadialDistribution(z, batch, 6.0, 120).add(traj.pos)
    assert torch.equal(rdf.counts, direct.counts) and int(rdf.counts.sum()) > 0
    kind = np.searchsorted([1, 6, 8], _np(z)).astype(np.int32)
    want = R.histogram(_np(traj.pos), np.zeros((4, 3, 3), f32), np.arange(0, 85, 21), kind, 3, 6.0, 120)
    assert np.array_equal(_np(rdf.counts), want)
    assert torch.allclose(rdf.distance_distribution().sum(dim=2), torch.ones(4, 6, dtype=torch.float64, device='cuda'))
    vacf = traj.velocity_autocorrelation(4)
    free = ob.velocity_autocorrelation(traj.vel, z, batch, 1.0, 4)
    assert isinstance(vacf, ob.VACF) and vacf.dt == 1.0 and torch.equal(vacf.vacf, free.vacf) and vacf.vacf.shape == (4, 3, 5)
    assert bool((vacf.vacf[..., 0] > 0).all())
    weighted = traj.velocity_autocorrelation(4, mass_weighted=True)
    assert torch.equal(weighted.vacf, ob.velocity_autocorrelation(traj.vel, z, batch, 1.0, 4, masses=dyn.masses).vacf)
    msd = traj.mean_squared_displacement(4)
    assert isinstance(msd, ob.MSD) and torch.equal(msd.msd, ob.mean_squared_displacement(traj.pos, z, batch, 1.0, 4).msd)
    assert bool((msd.msd[..., 0] == 0).all()) and bool((msd.msd[..., 1:] > 0).all())
    wn, dens = vacf.spectrum()
    assert wn.shape == (17,) and dens.shape == (4, 3, 17)
    with pytest.raises(ValueError, match='choose n_steps a multiple of record_every'):
        dyn.run(7, record_every=2).mean_squared_displacement(1)


def test_an_npt_trajectory_is_binned_under_the_cell_of_every_frame():
    z, pos, cell, batch = cuda(*mol_subset(*util.case_inputs('pbc_batch2_rand', torch.float32)[:4], [1]))
    model = make_model(util.load_state('rand'), props=('energy', 'gradient_force', 'virial'))
    dyn = model.constant_pressure(z, pos, cell, batch, pressure=1.0, temperature=100.0, compressibility=4.5e-4, barostat_time=200.0,
                                  timestep=0.5, generator=torch.Generator(device='cuda').manual_seed(5))
    traj = dyn.run(20, record_every=2)
    assert traj.cell.shape == (10, 1, 3, 3) and not torch.equal(traj.cell[0], traj.cell[-1])
    r_max, n_bins = 4.0, 400
    rdf = traj.radial_distribution(r_max, n_bins)
    species = sorted(set(_np(z).tolist()))
    kind = np.searchsorted(species, _np(z)).astype(np.int32)
    ptr = np.array([0, len(kind)])
    per_frame = R.histogram(_np(traj.pos), _np(traj.cell), ptr, kind, len(species), r_max, n_bins)
    first_only = R.histogram(_np(traj.pos), _np(traj.cell[0]), ptr, kind, len(species), r_max, n_bins)
    got = _np(rdf.counts)
    print(f'NPT: {int(got.sum())} pairs, {int(np.abs(per_frame - first_only).sum())} counter moves between per-frame and first-cell binning')
    assert np.array_equal(got, per_frame)
    assert not np.array_equal(got, first_only)
    assert np.allclose(_np(rdf.mean_volume), _np(traj.volume.double().mean(0)), rtol=1e-5)
    assert np.isfinite(_np(rdf.g())[0, 0]).all()
