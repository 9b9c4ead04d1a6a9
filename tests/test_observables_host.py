"""Host-side checks of the trajectory observables (no device): the fp32 statement of the pair-distance histogram
(tests/observables_ref.py) against an fp64 brute force over many images, the normalisations on a simple cubic lattice, the spectrum
of a synthetic autocorrelation, every refusal that must come before the device is touched, and the ABI symbols."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from newtonnet_amd import dynamics as dyn
from newtonnet_amd import hip
from newtonnet_amd import observables as ob
from newtonnet_amd import phonons as ph
from tests import graph_ref as G
from tests import observables_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

DIAGONAL = np.diag([12.0, 13.0, 14.0]).astype(f32)
SYMMETRIC = np.array([[12.0, 1.0, 0.8], [1.0, 13.0, 1.1], [0.8, 1.1, 14.0]], f32)


# ---- the fp32 statement against fp64 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name, cell, seed', [('diagonal', DIAGONAL, 0), ('symmetric', SYMMETRIC, 1)])
def test_fp32_statement_against_the_fp64_brute_force(name, cell, seed):
    """216 atoms, unwrapped over three cells per axis, r_max 5.5 A, 300 bins: the bin of the statement and the bin of the fp64 minimum
    image over 7^3 translations may differ only where the fp64 distance is within 1e-5 A of an edge, on at most 0.5 % of the pairs
    in range."""
    r_max, n_bins, n = 5.5, 300, 216
    assert r_max <= 0.5 * ph.perpendicular_widths(cell).min()
    rng = np.random.default_rng(seed)
    pos = ((rng.uniform(-1.0, 2.0, (n, 3))) @ cell.astype(np.float64)).astype(f32)
    mol_ptr, kind = np.array([0, n]), np.zeros(n, np.int32)
    counts, (r2, k32, tie) = R.histogram(pos[None], cell[None], mol_ptr, kind, 1, r_max, n_bins, with_pairs=True)
    ii, jj, _ = R.pairs_of(mol_ptr, kind)
    d64 = R.brute_force_distances(pos, cell, ii, jj, images=3)
    dr = r_max / n_bins
    k64 = np.floor(d64 / dr).astype(np.int64)
    k64 = np.where(k64 < n_bins, k64, -1)
    near = np.abs(d64 / dr - np.rint(d64 / dr)) * dr <= 1e-5
    differ = k32 != k64
    in_range = int((k64 >= 0).sum())
    print(f'{name}: {in_range} pairs in range, {int(near.sum())} within 1e-5 A of an edge, {int(differ.sum())} bins differ, '
          f'{int((differ & ~near).sum())} of them elsewhere, ties {int(tie.sum())}')
    assert in_range > 5000
    assert not (differ & ~near).any()
    assert (near & (k64 >= 0)).sum() <= 0.005 * in_range
    assert counts.sum() == (k32 >= 0).sum()
    if name == 'symmetric':
        assert tie.sum() == 0


def test_the_wrapper_forms_the_edges_of_the_statement():
    for r_max, n_bins in ((5.5, 300), (6.0, 7), (1.0, 1), (9.73, 4096)):
        r, edge2 = ob.bin_edges(r_max, n_bins)
        r_ref, edge2_ref = R.bin_table(r_max, n_bins)
        assert r.dtype == f32 and edge2.dtype == f32
        assert np.array_equal(r, r_ref) and np.array_equal(edge2, edge2_ref)
        assert edge2[0] == 0 and np.all(np.diff(edge2) > 0)
        # the threshold property, at the floats either side of every edge
        assert np.all(np.sqrt(edge2) >= r) and np.all(np.sqrt(np.nextafter(edge2[1:], f32(0))) < r[1:])


# ---- normalisations ------------------------------------------------------------------------------------------------------------

def test_normalisation_on_a_simple_cubic_lattice():
    a, m, r_max, n_bins = 3.0, 4, 5.5, 55
    grid = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing='ij'), -1).reshape(-1, 3)
    pos = (a * grid).astype(f32)
    n = len(pos)
    cell = (a * m * np.eye(3)).astype(f32)
    counts = R.histogram(pos[None], cell[None], np.array([0, n]), np.zeros(n, np.int32), 1, r_max, n_bins)
    r_edges = R.bin_table(r_max, n_bins)[0].astype(np.float64)
    kind_counts = torch.tensor([[n]])
    cn = ob.coordination_of_counts(torch.from_numpy(counts), 1, kind_counts)[0, 0].numpy()
    outer = r_edges[1:]
    first, second = (outer > 3.2) & (outer < 4.1), (outer > 4.4) & (outer < 5.1)
    assert first.sum() >= 5 and second.sum() >= 5
    assert np.all(cn[outer < 2.9] == 0.0) and np.all(cn[first] == 6.0) and np.all(cn[second] == 18.0)
    # the counts a uniform density gives: g = 1 in every bin, for one species and for two
    kc = torch.tensor([[40, 24], [7, 0]])
    vol = torch.tensor([1728.0, 0.0], dtype=torch.float64)
    shell = 4.0 * math.pi / 3.0 * (torch.tensor(r_edges[1:]) ** 3 - torch.tensor(r_edges[:-1]) ** 3)
    n_ab = ob.pair_numbers(kc)
    assert n_ab.tolist() == [[780.0, 960.0, 276.0], [21.0, 0.0, 0.0]]
    uniform = 5 * n_ab[:, :, None] * shell[None, None, :] / 1728.0
    g = ob.g_of_counts(uniform, 5, kc, vol, r_edges)
    assert torch.allclose(g[0], torch.ones_like(g[0]), rtol=1e-12, atol=0)
    assert torch.isnan(g[1]).all()                                   # no cell: no g(r)
    d = ob.distribution_of_counts(torch.from_numpy(counts))
    assert abs(float(d.sum()) - 1.0) < 1e-12
    assert ob.coordination_of_counts(uniform, 5, kc, reverse=True)[0, 1, -1] == pytest.approx(float(uniform[0, 1].sum()) / 5 / 24)


def test_diffusion_and_green_kubo_on_exact_curves():
    t = torch.arange(101, dtype=torch.float64) * 2.0
    msd = (6.0 * 0.25 * t + 3.0)[None, None, :]
    assert ob.slope_of(t, msd, (50.0, 200.0)).item() / 6.0 == pytest.approx(0.25, rel=1e-12)
    assert ob.slope_of(t, msd).item() / 6.0 == pytest.approx(0.25, rel=1e-12)
    assert ob.diffusion_in_cm2_per_s(1e-3) == pytest.approx(1e-4)
    assert ob.trapezoid_of(torch.ones(1, 1, 11, dtype=torch.float64), 0.5).item() == pytest.approx(5.0)
    assert ob.origins_per_lag(37, 12, 5).tolist() == [len(range(0, 37 - lag, 5)) for lag in range(13)]


def test_spectrum_of_a_cosine_peaks_in_its_bin():
    dt, L, wn0 = 1.0, 1000, 1000.0
    f0 = wn0 * ob.SPEED_OF_LIGHT_CM_PER_FS
    c = torch.cos(2.0 * math.pi * f0 * dt * torch.arange(L + 1, dtype=torch.float64))
    for pad in (1, 4):
        wn, dens = ob.spectrum_of(torch.stack([c, 2 * c])[None], dt, 'hann', pad)
        assert dens.shape == (1, 2, pad * L + 1) and wn.shape == (pad * L + 1,)
        spacing = float(wn[1] - wn[0])
        assert spacing == pytest.approx(1.0 / (2 * pad * L * dt * ob.SPEED_OF_LIGHT_CM_PER_FS))
        k = int(dens[0, 0].argmax())
        assert abs(float(wn[k]) - wn0) <= spacing
        assert torch.allclose(dens[0, 1], 2 * dens[0, 0])
    with pytest.raises(ValueError, match='window'):
        ob.spectrum_of(c, dt, 'boxcar')


# ---- refusals before the device is touched (every tensor here is on the CPU) ------------------------------------------------------

def _box(n=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.tensor([8, 1, 1] * n)[:n]
    return z, torch.zeros(n, dtype=torch.long), torch.rand(3, n, 3, generator=g) * 10.0


def test_a_cell_that_is_not_symmetric_is_refused():
    z, batch, pos = _box()
    cell = torch.tensor([[[12.0, 0.0, 0.0], [2.5, 12.0, 0.0], [0.0, 0.0, 12.0]]])
    with pytest.raises(ValueError, match=r'frame 0, system 0: the cell is not a symmetric matrix.*phonons\.symmetric_cell'):
        ob.RadialDistribution(z, batch, 3.0, 10, cell=cell).add(pos)
    # per-frame cells: the first offending frame is named
    good = torch.diag(torch.tensor([12.0, 12.0, 12.0]))[None]
    cells = torch.stack([good, good, cell])
    with pytest.raises(ValueError, match='frame 2, system 0: the cell is not a symmetric'):
        ob.RadialDistribution(z, batch, 3.0, 10).add(pos, cells)


def test_r_max_above_the_half_width_is_refused_with_frame_and_system():
    z = torch.tensor([8, 1, 1, 8, 1, 1])
    batch = torch.tensor([0, 0, 0, 1, 1, 1])
    pos = torch.rand(2, 6, 3)
    wide, tight = torch.tensor(SYMMETRIC), torch.diag(torch.tensor([12.0, 9.0, 12.0]))
    cells = torch.stack([torch.stack([wide, wide]), torch.stack([wide, tight])])
    with pytest.raises(ValueError, match=r'frame 1, system 1: r_max = 5\.0000 A is above half the smallest perpendicular width.*4\.5000 A'):
        ob.RadialDistribution(z, batch, 5.0, 10).add(pos, cells)
    half = 0.5 * ph.perpendicular_widths(SYMMETRIC).min()
    with pytest.raises(ValueError, match='frame 0, system 0: r_max'):
        ob.RadialDistribution(z, batch, half * 1.001, 10, cell=torch.stack([wide, wide])).add(pos)
    # at the bound itself, and without a cell, the checks pass: the call gets as far as the device
    with pytest.raises(RuntimeError, match='MI355X'):
        ob.RadialDistribution(z, batch, half * 0.999, 10, cell=torch.stack([wide, wide])).add(pos)
    with pytest.raises(RuntimeError, match='MI355X'):
        ob.RadialDistribution(z, batch, 50.0, 10).add(pos)


def test_the_limits_of_the_histogram_are_refused():
    z, batch, pos = _box(9)
    z9 = torch.arange(1, 10)
    with pytest.raises(ValueError, match='9 species: at most 8'):
        ob.RadialDistribution(z9, batch, 3.0, 10)
    with pytest.raises(ValueError, match='4097 bins are outside'):
        ob.RadialDistribution(z, batch, 3.0, 4097)
    with pytest.raises(ValueError, match='n_kinds \\(n_kinds \\+ 1\\) / 2 \\* n_bins <= 16384'):
        ob.RadialDistribution(z9[:8], batch[:8], 3.0, 456)           # 36 x 456 = 16416
    ob.RadialDistribution(z9[:8], batch[:8], 3.0, 455)               # 36 x 455 = 16380
    assert ob.RadialDistribution(z, batch, 3.0, 10, species=[1]).pairs == [(1, 1)]
    assert ob.RadialDistribution(z, batch, 3.0, 10).pairs == [(1, 1), (1, 8), (8, 8)]
    assert (hip.RDF_MAX_KINDS, hip.RDF_MAX_BINS, hip.RDF_MAX_COUNTERS) == (8, 4096, 16384)


def test_a_lag_of_all_the_frames_is_refused():
    z, batch, pos = _box()
    with pytest.raises(ValueError, match='max_lag: an integer in 0 .. n_frames - 1 = 2'):
        ob.mean_squared_displacement(pos, z, batch, 1.0, 3)
    with pytest.raises(ValueError, match='max_lag'):
        ob.velocity_autocorrelation(pos, z, batch, 1.0, 7)
    with pytest.raises(ValueError, match='origin_every'):
        ob.mean_squared_displacement(pos, z, batch, 1.0, 2, origin_every=0)
    with pytest.raises(RuntimeError, match='MI355X'):
        ob.mean_squared_displacement(pos, z, batch, 1.0, 2)


def test_unevenly_recorded_steps_are_refused():
    z, batch, pos = _box()
    traj = dyn.Trajectory(torch.tensor([3, 6, 7]), pos, pos.clone(), torch.zeros(3, 1), torch.zeros(3, 1), torch.tensor([8]))
    traj._system = (z, batch, torch.zeros(1, 3, 3), torch.ones(8), 0.5)
    for call in (lambda: traj.mean_squared_displacement(1), lambda: traj.velocity_autocorrelation(1)):
        with pytest.raises(ValueError, match='choose n_steps a multiple of record_every'):
            call()
    traj.step = torch.tensor([3, 6, 9])
    assert traj._frame_spacing() == 1.5
    with pytest.raises(RuntimeError, match='MI355X'):
        traj.radial_distribution(3.0, 10)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------

def test_the_two_entry_points_are_declared_bound_and_built():
    from newtonnet_amd import abi
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for name in ('nnhip_rdf_accumulate', 'nnhip_time_correlation'):
        assert name in declared and name in abi.FUNCTIONS and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bobservables\b.*\)', f.read(), re.M)
    # one copy of the pair predicate: graph.hip and observables.hip include it
    csrc = os.path.join(ROOT, 'newtonnet_amd', 'csrc')
    holders = [n for n in sorted(os.listdir(csrc)) if n.endswith(('.hip', '.h'))
               and re.search(r'float\s+pair_disp\s*\(', open(os.path.join(csrc, n)).read())]
    assert holders == ['pair_disp.h']
    for n in ('graph.hip', 'observables.hip'):
        assert '#include "pair_disp.h"' in open(os.path.join(csrc, n)).read()
