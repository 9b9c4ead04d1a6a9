"""Observables of molecular-dynamics trajectories on the HIP path: the radial distribution function, the mean squared displacement and
the velocity autocorrelation with its spectrum, from the [F,N,3] device tensors a `Trajectory` holds (or any others): no model is needed
and no frame leaves the device.

Two kernels (csrc/observables.hip; the arithmetic is written out in include/newtonnet_hip.h):

    nnhip_rdf_accumulate     the histogram of pair distances per system and pair of species, under the model's own minimum image: r2
                             of a pair is bit for bit the r2 of the neighbour list (pair_disp), and the bin edges are thresholds on
                             r2 formed here on the host (the neighbour list's cut2_of construction), so a pair sits in bin k exactly
                             when r_k <= sqrt_rn(r2) < r_{k+1}.  Integer counts: independent of scheduling.
    nnhip_time_correlation   sum over origins and atoms of x(t0) . x(t0 + l) or |x(t0 + l) - x(t0)|^2 per system, species and lag:
                             fp32 terms, fp64 sums in a fixed order, evaluated directly (O(F L N); no FFT).

The normalisations (g(r), coordination numbers, diffusion constants, the spectrum) are plain torch functions of the small arrays the
kernels leave; they also run on CPU tensors.

Blocks.  `add` may be called with one block of frames after another (a long run recorded in pieces): counts, sums and origins add up,
so the result is the average over all blocks.  A block is a trajectory of its own: no lag crosses a block boundary, and the frames of
one block are evenly spaced.

Units: Angstrom, fs, amu.  Velocities are taken in the library's internal unit (Angstrom per Angstrom sqrt(amu / eV), what
`Trajectory.vel` holds) and the autocorrelation is returned in Angstrom^2 / fs^2.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from newtonnet_amd import hip
from newtonnet_amd.dynamics import FS, _mol_ptr

A2_PER_FS_IN_CM2_PER_S = 0.1                 # 1 Angstrom^2 / fs = 1e-16 cm^2 / 1e-15 s
SPEED_OF_LIGHT_CM_PER_FS = 2.99792458e-5


def diffusion_in_cm2_per_s(d):
    """a diffusion constant in Angstrom^2 / fs (what `diffusion()` returns) in cm^2 / s"""
    return d * A2_PER_FS_IN_CM2_PER_S


# ------------------------------------------------------------------------------------------------------------------------------
# what both observables need of the system
# ------------------------------------------------------------------------------------------------------------------------------
def _species_kinds(z: torch.Tensor, species):
    """(species list, kind int32 [N] on the device of z): the index of every atom's species, -1 for an atom of none of them.
    species None: every species present, ascending (one host read of z)."""
    if not isinstance(z, torch.Tensor) or z.dim() != 1:
        raise ValueError('z: a tensor [N] of atomic numbers expected')
    if species is None:
        species = sorted(set(z.detach().cpu().tolist()))
    species = [int(s) for s in species]
    if len(set(species)) != len(species) or not species:
        raise ValueError(f'species: distinct atomic numbers, at least one, expected (got {species})')
    if len(species) > hip.RDF_MAX_KINDS:
        raise ValueError(f'{len(species)} species: at most {hip.RDF_MAX_KINDS} are counted at once; name the ones you want '
                         f'(species=[...]), the others are ignored')
    kind = torch.full((z.numel(),), -1, dtype=torch.int32, device=z.device)
    for k, s in enumerate(species):
        kind[z == s] = k
    return species, kind


def _system(z, batch, n_mol, species):
    """(species, kind int32 [N], mol_ptr int32 [B+1], atoms per system and species int64 [B,S], B)"""
    if not isinstance(batch, torch.Tensor) or batch.shape != z.shape or batch.device != z.device:
        raise ValueError('z and batch: tensors [N] on one device expected')
    species, kind = _species_kinds(z, species)
    B = int(n_mol) if n_mol is not None else (int(batch.max()) + 1 if batch.numel() else 0)
    S = len(species)
    ok = kind >= 0
    per = torch.zeros(B * S, dtype=torch.int64, device=z.device)
    if batch.numel():
        per.index_add_(0, (batch.long() * S + kind.long().clamp(min=0))[ok], torch.ones_like(batch, dtype=torch.int64)[ok])
    return species, kind, _mol_ptr(batch, B), per.view(B, S), B


def _need_device(t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError('newtonnet_amd observables run on an MI355X (ROCm) device only: move the frames to "cuda"')


# ------------------------------------------------------------------------------------------------------------------------------
# radial distribution
# ------------------------------------------------------------------------------------------------------------------------------
def bin_edges(r_max: float, n_bins: int):
    """(r fp32 [n_bins + 1], edge2 fp32 [n_bins + 1]) as numpy: r_k = fl32(k r_max / n_bins) and edge2[k] = the smallest float T with
    sqrt_rn(T) >= r_k (numpy's float32 sqrt is correctly rounded): r2 >= edge2[k] exactly when sqrt_rn(r2) >= r_k."""
    r = (np.arange(n_bins + 1, dtype=np.float64) * float(r_max) / n_bins).astype(np.float32)
    t = (r * r).astype(np.float32)
    zero, inf = np.float32(0), np.float32(np.inf)
    while True:
        down = (t > 0) & (np.sqrt(t) >= r)
        if not down.any():
            break
        t = np.where(down, np.nextafter(t, zero), t)
    while True:
        up = np.sqrt(t) < r
        if not up.any():
            break
        t = np.where(up, np.nextafter(t, inf), t)
    return r, t.astype(np.float32)


def pair_kinds(species):
    """the pairs (Z_a, Z_b), a <= b in the order of `species`, in the order of the histogram's second axis"""
    return [(species[a], species[b]) for a in range(len(species)) for b in range(a, len(species))]


def _pair_index(S: int):
    return [(a, b) for a in range(S) for b in range(a, S)]


def pair_numbers(kind_counts: torch.Tensor) -> torch.Tensor:
    """[B,P] (fp64): N_a N_b pairs of two species, N_a (N_a - 1) / 2 of one"""
    n = kind_counts.double()
    return torch.stack([n[:, a] * n[:, b] if a != b else n[:, a] * (n[:, a] - 1) / 2 for a, b in _pair_index(n.shape[1])], dim=1)


def g_of_counts(counts, n_frames, kind_counts, volume, r_edges) -> torch.Tensor:
    """g(r) [B,P,n_bins] (fp64) = <count> <V> / (N_ab shell_k): counts int64 [B,P,n_bins] summed over n_frames frames, kind_counts
    [B,S], volume [B] (the mean volume; NaN or 0 = not periodic: the row is NaN), r_edges [n_bins + 1]."""
    r = torch.as_tensor(r_edges, dtype=torch.float64, device=counts.device)
    shell = 4.0 * math.pi / 3.0 * (r[1:] ** 3 - r[:-1] ** 3)
    vol = torch.as_tensor(volume, dtype=torch.float64, device=counts.device)
    vol = torch.where(vol > 0, vol, torch.full_like(vol, float('nan')))
    mean = counts.double() / max(int(n_frames), 1)
    return mean * vol[:, None, None] / (pair_numbers(kind_counts)[:, :, None] * shell[None, None, :])


def coordination_of_counts(counts, n_frames, kind_counts, reverse: bool = False) -> torch.Tensor:
    """[B,P,n_bins] (fp64): the running number of neighbours of species b within the bin's outer edge around one atom of species a,
    for the pair (a, b) of every row (reverse: of a around one b).  A pair of one species is two neighbour relations."""
    n = kind_counts.double()
    idx = _pair_index(n.shape[1])
    per_atom = torch.stack([(2.0 if a == b else 1.0) / n[:, b if reverse else a] for a, b in idx], dim=1)
    return torch.cumsum(counts.double() / max(int(n_frames), 1), dim=2) * per_atom[:, :, None]


def distribution_of_counts(counts) -> torch.Tensor:
    """[B,P,n_bins] (fp64): the counts of every (system, pair) normalised to sum 1 (0 where there is none): the distribution of pair
    distances of a molecule"""
    c = counts.double()
    return c / c.sum(dim=2, keepdim=True).clamp(min=1.0)


def _cell_checks(cells: torch.Tensor, r_max: float):
    """cells fp32 [F',B,3,3].  Raises ValueError for the first (frame, system) whose cell the single-image shift cannot serve; returns
    the volumes fp64 [F',B] (0 for a system without a cell).  Torch ops where the cells live, then one host read."""
    c = cells.detach().double()
    amax = c.abs().amax(dim=(2, 3))
    periodic = amax > 0
    off = c - torch.diag_embed(torch.diagonal(c, dim1=2, dim2=3))
    diagonal = off.abs().amax(dim=(2, 3)) == 0
    asym = (c - c.transpose(2, 3)).abs().amax(dim=(2, 3)) > 1e-5 * amax
    vol = torch.linalg.det(c).abs()
    cross = torch.stack([torch.linalg.cross(c[:, :, (k + 1) % 3], c[:, :, (k + 2) % 3], dim=2).norm(dim=2) for k in range(3)], dim=2)
    width = (vol[:, :, None] / cross.clamp(min=1e-300)).amin(dim=2)                # [F',B] smallest perpendicular width
    bad_sym = periodic & ~diagonal & asym
    bad_width = periodic & ~(float(r_max) <= 0.5 * width)
    flags = torch.stack([bad_sym, bad_width]).cpu()                                 # (the one host read)
    if bool(flags[0].any()):
        f, b = torch.nonzero(flags[0])[0].tolist()
        raise ValueError(f'frame {f}, system {b}: the cell is not a symmetric matrix.  The model shifts a pair to its minimum image by '
                         f'cell @ round(frac), as the reference writes it, which is a lattice vector only when cell = cell^T.  Rotate '
                         f'the system first: phonons.symmetric_cell(pos, cell)')
    if bool(flags[1].any()):
        f, b = torch.nonzero(flags[1])[0].tolist()
        raise ValueError(f'frame {f}, system {b}: r_max = {float(r_max):.4f} A is above half the smallest perpendicular width of the '
                         f'cell, {0.5 * float(width[f, b]):.4f} A (phonons.perpendicular_widths): beyond it the single-image shift of '
                         f'the neighbour list is not the minimum image.  Lower r_max or use a larger cell')
    return torch.where(periodic, vol, torch.zeros_like(vol))


class RadialDistribution:
    """Pair-distance histograms of B systems, per pair of species, accumulated on the device over any number of frames.

    z, batch: [N] as for the model; r_max in Angstrom, n_bins equal bins on [0, r_max).  cell: fp32 [B,3,3] for every frame that
    `add` is given without cells (None: no system is periodic).  species: the atomic numbers to count (None: all present, ascending);
    atoms of other species are ignored.  At most hip.RDF_MAX_KINDS species, hip.RDF_MAX_BINS bins and hip.RDF_MAX_COUNTERS counters
    per system (pairs x bins).

    counts       int64 [B,P,n_bins] on the device: pairs i < j of one system and frame with r_k <= r < r_{k+1}, r under the model's
                 single-image shift
    pairs        [(Z_a, Z_b)] of each of the P = S (S + 1) / 2 rows
    r, r_edges   bin centres [n_bins] and edges [n_bins + 1], fp64, on the device of z
    n_frames     frames added so far;  mean_volume fp64 [B] (0: the system has no cell);  kind_counts int64 [B,S]

    Blocks: add(frames[:k]); add(frames[k:]) leaves exactly the counts of add(frames)."""

    def __init__(self, z, batch, r_max, n_bins, cell=None, species=None):
        if int(n_bins) != n_bins or n_bins < 1:
            raise ValueError(f'n_bins: an integer >= 1 expected (got {n_bins!r})')
        if not (float(r_max) > 0.0 and math.isfinite(float(r_max))):
            raise ValueError(f'r_max: a finite value > 0 Angstrom expected (got {r_max!r})')
        n_mol = None
        if cell is not None:
            if not isinstance(cell, torch.Tensor) or cell.dim() != 3 or tuple(cell.shape[1:]) != (3, 3) or cell.dtype != torch.float32:
                raise ValueError('cell: a float32 tensor [B,3,3] expected')
            n_mol = cell.shape[0]
        self.species, self._kind, self._mol_ptr, self.kind_counts, self.n_mol = _system(z, batch, n_mol, species)
        self.r_max, self.n_bins = float(r_max), int(n_bins)
        hip.check_histogram_size(len(self.species), self.n_bins)
        dev = z.device
        self.pairs = pair_kinds(self.species)
        r32, edge2 = bin_edges(self.r_max, self.n_bins)
        self._edge2 = torch.from_numpy(edge2).to(dev)
        self.r_edges = torch.from_numpy(r32.astype(np.float64)).to(dev)
        self.r = 0.5 * (self.r_edges[1:] + self.r_edges[:-1])
        self._cell = cell.detach().contiguous() if cell is not None else torch.zeros(self.n_mol, 3, 3, dtype=torch.float32, device=dev)
        self._max_atoms = int((self._mol_ptr[1:] - self._mol_ptr[:-1]).max()) if self.n_mol else 0
        self.counts = torch.zeros(self.n_mol, len(self.pairs), self.n_bins, dtype=torch.int64, device=dev)
        self._volume_sum = torch.zeros(self.n_mol, dtype=torch.float64, device=dev)
        self.n_frames = 0

    def add(self, pos, cell=None):
        """Count the pairs of one frame pos [N,3] or of a block [F,N,3] (fp32, on the device).  cell: None (the constructor's), [B,3,3]
        (every frame of the block) or [F,B,3,3] (per frame: what NPTTrajectory.cell holds).  Refused before any launch: a periodic
        cell that is neither diagonal nor symmetric, and r_max above half the smallest perpendicular width of any frame's cell."""
        N, B = self._kind.numel(), self.n_mol
        if not isinstance(pos, torch.Tensor) or pos.dtype != torch.float32 or pos.dim() not in (2, 3) or tuple(pos.shape[-2:]) != (N, 3):
            raise ValueError(f'pos: a float32 tensor [{N},3] or [F,{N},3] expected')
        frames = pos.detach().reshape(-1, N, 3)
        F = frames.shape[0]
        cells = self._cell if cell is None else cell
        if not isinstance(cells, torch.Tensor) or cells.dtype != torch.float32 or tuple(cells.shape) not in ((B, 3, 3), (F, B, 3, 3)):
            raise ValueError(f'cell: a float32 tensor [{B},3,3] or [{F},{B},3,3] expected')
        if cells.device != frames.device or frames.device != self._kind.device:
            raise ValueError(f'pos and cell: on {self._kind.device} expected')
        cells = cells.detach().contiguous()
        vol = _cell_checks(cells.reshape(-1, B, 3, 3), self.r_max)
        if F == 0:
            return self
        _need_device(frames)
        hip.rdf_accumulate(frames.contiguous(), cells, self._mol_ptr, self._kind, len(self.species), self._edge2, self.counts,
                           self._max_atoms)
        self._volume_sum += vol.sum(dim=0) * (F if vol.shape[0] == 1 else 1)
        self.n_frames += F
        return self

    @property
    def mean_volume(self):
        return self._volume_sum / max(self.n_frames, 1)

    def g(self):
        """g(r) fp64 [B,P,n_bins] = <count> <V> / (N_ab shell_k); the rows of a system without a cell are NaN"""
        return g_of_counts(self.counts, self.n_frames, self.kind_counts, self.mean_volume, self.r_edges)

    def coordination(self, reverse: bool = False):
        """fp64 [B,P,n_bins]: running number of b neighbours of an a atom for the row's pair (a, b) (reverse: a around b)"""
        return coordination_of_counts(self.counts, self.n_frames, self.kind_counts, reverse)

    def distance_distribution(self):
        """fp64 [B,P,n_bins]: the counts of every row normalised to 1 (molecules: no volume is involved)"""
        return distribution_of_counts(self.counts)


# ------------------------------------------------------------------------------------------------------------------------------
# lagged correlations
# ------------------------------------------------------------------------------------------------------------------------------
def origins_per_lag(n_frames: int, max_lag: int, origin_every: int) -> torch.Tensor:
    """int64 [max_lag + 1]: origins t0 = 0, origin_every, ... with t0 + l < n_frames"""
    lag = torch.arange(max_lag + 1, dtype=torch.int64)
    return (n_frames - lag + origin_every - 1) // origin_every


class _Lagged:
    """sums of a lagged correlation per (system, species, lag) over one or more blocks of frames"""
    _mode = hip.TC_PRODUCT

    def __init__(self, z, batch, dt, max_lag, origin_every=1, species=None, weight=None, n_mol=None):
        if not (float(dt) > 0.0 and math.isfinite(float(dt))):
            raise ValueError(f'dt: the time between two frames, a finite value > 0 fs, expected (got {dt!r})')
        if int(max_lag) != max_lag or max_lag < 0:
            raise ValueError(f'max_lag: an integer >= 0 expected (got {max_lag!r})')
        if int(origin_every) != origin_every or origin_every < 1:
            raise ValueError(f'origin_every: an integer >= 1 expected (got {origin_every!r})')
        self.species, self._kind, self._mol_ptr, self.kind_counts, self.n_mol = _system(z, batch, n_mol, species)
        self.dt, self.max_lag, self.origin_every = float(dt), int(max_lag), int(origin_every)
        dev = z.device
        if weight is not None:
            if not isinstance(weight, torch.Tensor) or weight.numel() != z.numel() or weight.device != dev:
                raise ValueError(f'masses: a tensor of {z.numel()} values on {dev} expected')
            weight = weight.detach().float().reshape(-1).contiguous()
        self._weight = weight
        self.time = torch.arange(self.max_lag + 1, dtype=torch.float64, device=dev) * self.dt
        self.sums = torch.zeros(self.n_mol, len(self.species), self.max_lag + 1, dtype=torch.float64, device=dev)
        self.n_origins = torch.zeros(self.max_lag + 1, dtype=torch.int64, device=dev)

    def add(self, x):
        """one block of evenly spaced frames x [F,N,3] (fp32, on the device), F > max_lag"""
        N = self._kind.numel()
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 3 or tuple(x.shape[1:]) != (N, 3):
            raise ValueError(f'frames: a float32 tensor [F,{N},3] expected')
        F = x.shape[0]
        hip.check_correlation(F, self.max_lag, self.origin_every, self._mode)
        if x.device != self._kind.device:
            raise ValueError(f'frames: on {self._kind.device} expected')
        _need_device(x)
        hip.time_correlation(x.detach().contiguous(), self._mol_ptr, self._kind, len(self.species), self._mode, self.max_lag, self.sums,
                             origin_every=self.origin_every, weight=self._weight)
        self.n_origins += origins_per_lag(F, self.max_lag, self.origin_every).to(self.n_origins.device)
        return self

    def _mean(self):
        """sums / (origins x atoms of the species): NaN where a system has no atom of a species"""
        n = self.kind_counts.double()
        n = torch.where(n > 0, n, torch.full_like(n, float('nan')))
        return self.sums / (self.n_origins.double().clamp(min=1)[None, None, :] * n[:, :, None])


def slope_of(time, y, fit=None) -> torch.Tensor:
    """least-squares slope of y [..., L+1] against time [L+1] over fit = (t_lo, t_hi) (inclusive; None: the upper half of the lags)"""
    t = torch.as_tensor(time, dtype=torch.float64, device=y.device)
    lo, hi = (0.5 * float(t[-1]), float(t[-1])) if fit is None else (float(fit[0]), float(fit[1]))
    use = (t >= lo) & (t <= hi)
    if int(use.sum()) < 2:
        raise ValueError(f'fit = ({lo}, {hi}) fs holds fewer than two lags')
    tt = t[use] - t[use].mean()
    return (y[..., use].double() * tt).sum(dim=-1) / (tt * tt).sum()


class MSD(_Lagged):
    """Mean squared displacement <|x(t0 + t) - x(t0)|^2> per system and species, of UNWRAPPED positions (what Trajectory.pos holds).

    time fp64 [L+1] in fs;  msd fp64 [B,S,L+1] in Angstrom^2;  n_origins int64 [L+1];  species, kind_counts [B,S].
    add(pos) averages a further block in; no lag crosses a block boundary."""
    _mode = hip.TC_DISPLACEMENT

    @property
    def msd(self):
        return self._mean()

    def diffusion(self, fit=None):
        """fp64 [B,S], Angstrom^2 / fs: the least-squares slope of msd over fit = (t_lo, t_hi) in fs (None: the upper half of the
        lags), divided by 6 (diffusion_in_cm2_per_s converts)"""
        return slope_of(self.time, self.msd, fit) / 6.0


def trapezoid_of(y, dt) -> torch.Tensor:
    return (y[..., 1:] + y[..., :-1]).sum(dim=-1) * (0.5 * float(dt))


def spectrum_of(vacf, dt, window: Optional[str] = 'hann', pad: int = 4):
    """(wavenumber fp64 [M/2 + 1] in cm^-1, density fp64 [..., M/2 + 1]): the cosine transform of a correlation vacf [..., L+1] sampled
    every dt fs, I(f) = dt sum_l w_l c_l cos(2 pi f l dt) over the even extension l = -L .. L, by one real FFT of length M = 2 pad L.
    window: 'hann' (w_l = (1 + cos(pi l / L)) / 2, zero at the last lag) or None.  pad >= 1 zero-pads: a finer frequency grid."""
    c = torch.as_tensor(vacf).double()
    L = c.shape[-1] - 1
    if L < 1:
        raise ValueError('a spectrum needs at least two lags')
    if int(pad) != pad or pad < 1:
        raise ValueError(f'pad: an integer >= 1 expected (got {pad!r})')
    if window == 'hann':
        c = c * (0.5 * (1.0 + torch.cos(math.pi * torch.arange(L + 1, dtype=torch.float64, device=c.device) / L)))
    elif window is not None:
        raise ValueError(f"window: 'hann' or None expected (got {window!r})")
    M = 2 * int(pad) * L
    y = torch.zeros(c.shape[:-1] + (M,), dtype=torch.float64, device=c.device)
    y[..., :L + 1] = c
    y[..., M - L:] = torch.flip(c[..., 1:], dims=(-1,))
    density = torch.fft.rfft(y, dim=-1).real * float(dt)
    freq = torch.arange(M // 2 + 1, dtype=torch.float64, device=c.device) / (M * float(dt))      # 1 / fs
    return freq / SPEED_OF_LIGHT_CM_PER_FS, density


class VACF(_Lagged):
    """Velocity autocorrelation <v(t0) . v(t0 + t)> per system and species.

    time fp64 [L+1] in fs;  vacf fp64 [B,S,L+1] in Angstrom^2 / fs^2, or amu Angstrom^2 / fs^2 (mass-weighted: <m v . v>) when masses
    were given;  normalized = vacf / vacf[..., :1];  n_origins int64 [L+1].  add(vel) averages a further block in; no lag crosses a
    block boundary."""
    _mode = hip.TC_PRODUCT

    @property
    def vacf(self):
        return self._mean() * (FS * FS)

    @property
    def normalized(self):
        c = self.vacf
        return c / c[..., :1]

    def diffusion(self):
        """fp64 [B,S], Angstrom^2 / fs: Green-Kubo, a third of the trapezoid integral of the (unweighted) vacf over the lags"""
        if self._weight is not None:
            raise ValueError('diffusion() needs the plain velocity autocorrelation: make it without masses')
        return trapezoid_of(self.vacf, self.dt) / 3.0

    def spectrum(self, window: Optional[str] = 'hann', pad: int = 4):
        """(wavenumber [K] in cm^-1, density [B,S,K]): spectrum_of(vacf): with masses the vibrational density of states"""
        return spectrum_of(self.vacf, self.dt, window, pad)


def mean_squared_displacement(pos, z, batch, dt, max_lag, origin_every=1, species=None, n_mol=None) -> MSD:
    """MSD of one block of evenly spaced frames pos [F,N,3] (unwrapped, fp32, on the device), dt fs apart, for lags 0 .. max_lag and
    origins 0, origin_every, ...; species as for RadialDistribution; n_mol: the number of systems (None: batch.max() + 1)."""
    return MSD(z, batch, dt, max_lag, origin_every, species, None, n_mol).add(pos)


def velocity_autocorrelation(vel, z, batch, dt, max_lag, masses=None, origin_every=1, species=None, n_mol=None) -> VACF:
    """VACF of one block of evenly spaced frames vel [F,N,3] (the library's velocity unit, fp32, on the device), dt fs apart;
    masses [N] (amu): mass-weighted.  The rest as for mean_squared_displacement."""
    return VACF(z, batch, dt, max_lag, origin_every, species, masses, n_mol).add(vel)
