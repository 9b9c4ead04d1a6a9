"""Batched phonon dispersion, density of states and harmonic thermochemistry of crystals on the HIP path.

normal_modes treats a periodic system as a molecule at Gamma.  Here B primitive cells go through the finite-displacement-free
supercell method: the analytic Hessian columns of the home atoms on a supercell (nnhip_hessian_blocks with n_dirs = 3 n_b) are
the force constants Phi(i, J); ONE launch of nnhip_phonon_bands (csrc/phonon.hip) then assembles the dynamical matrix D(q) and
diagonalises the complex Hermitian d x d problem (d = 3 n_b) for every crystal and every wave vector of a path or a mesh.
That form keeps a problem in the LDS of one workgroup and serves primitive cells up to max_dim() = 96 coordinates (32 atoms);
solver='auto' sends larger ones, up to max_dim_large() = 768 coordinates (256 atoms), through the blocked solver
nnhip_phonon_bands_large (csrc/phonon_large.hip), which keeps D(q) in a torch-owned workspace in HBM.

Convention.  Supercell atom J = R n_b + j is the copy of home atom j at lattice offset R (the home cell R = 0 first, then the
offsets in lexicographic order, last index fastest).  For each (i, J) the image table holds the supercell-lattice translations
T in {-1, 0, 1}^3 that minimise |r_J + T - r_i| (ties at relative 1e-8, m_iJ of them), stored as r_J + T - r_i in units of the
primitive lattice vectors, and
    D_ij(q) = (m_i m_j)^-1/2 sum_{J in copies of j} Phi(i, J) (1 / m_iJ) sum_T exp(i q . (r_J + T - r_i)),   then (D + D^H) / 2.
It is Hermitian at any q and reproduces the supercell's spectrum exactly over the commensurate q.  q is given in units of the
primitive reciprocal vectors (q_frac . x_frac = q . r / 2 pi).

Units as in vibrations.py: eigenvalues in eV / (A^2 amu), frequencies in cm^-1 (x 521.4709, negative = imaginary).

Group velocities (frequencies / band_structure / mesh with velocities=True): one more launch, nnhip_phonon_velocities
(csrc/phonon_velocity.hip; one per crystal from band_structure, whose segment directions depend on the cell), takes d lambda / d q_cart = e^H (dD/dq) e of every mode from the force constants, the image table and
the modes the solver left on the device, with degenerate perturbation theory along a direction inside groups of (nearly) equal
eigenvalues; v = d lambda / (2 sqrt|lambda|) in A/ps.  PhononMesh.transport_tensor sums C_v v v over such a mesh.

Mode Grueneisen parameters and thermal expansion are newtonnet_amd/gruneisen.py: the same launch shape with the derivative of D taken
along strain (csrc/phonon_gruneisen.hip), on planes of force-constant derivatives made with _force_constants below.

Left out: the non-analytic LO-TO correction (it needs Born charges, which the model has not got), symmetry reduction of meshes
and paths, primitive cells above max_dim_large() coordinates; of the velocities: the Gamma limit of the acoustic branches,
degenerate groups above MAX_DEGENERATE modes, and the split inside a subgroup the direction leaves degenerate.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from newtonnet_amd import hessian as _hessian
from newtonnet_amd import hip
from newtonnet_amd import vibrations as _v

TIE_TOL = 1e-8          # relative tolerance at which two images count as equally near
EPS32 = _v.EPS32
SOLVERS = _v.SOLVERS
LARGE_WORKSPACE_BYTES = 1 << 30   # the wave vectors of a blocked call are chunked so that a chunk's workspace stays within this
IMAGE_TABLE_BYTES = 1 << 28       # image_table walks the home atoms in chunks whose candidate array stays within this
MAX_DEGENERATE = 16               # largest group of (nearly) equal eigenvalues nnhip_phonon_velocities rotates (status bit 3 above)
STATUS_GROUP = hip.abi.CONSTANTS['NNHIP_PHONON_STATUS_GROUP']
STATUS_NONFINITE = hip.abi.CONSTANTS['NNHIP_PHONON_STATUS_NONFINITE']
# sqrt(eV / amu) in A / ps: omega (rad / s) of a unit eigenvalue is 2 pi c x its wavenumber; 98.227
ANGSTROM_PER_PS_PER_SQRT_EV_AMU = _v.WAVENUMBER_PER_SQRT_EIGENVALUE * 2.0 * math.pi * _v._C_LIGHT * 1e-12
# eV / (K A ps) in W / (m K): kappa / tau of transport_tensor per ps of relaxation time; 1602.18
WATT_PER_M_K_PER_PS = _v._E_CHARGE * 1e10 * 1e12


def max_dim() -> int:
    """Largest d = 3 n_b of a primitive cell nnhip_phonon_bands serves (nnhip_phonon_max_dim): the dynamical matrix and its
    eigenvectors of one (crystal, q) problem live in the LDS of one workgroup."""
    return int(hip.lib().nnhip_phonon_max_dim())


def max_dim_large() -> int:
    """Largest d = 3 n_b the blocked solver serves (nnhip_phonon_large_max_dim; solver='auto' / 'blocked'): the size its accuracy
    bound has been verified at; the workspace takes about 16 Mp^2 bytes per (crystal, q) problem with modes."""
    return int(hip.lib().nnhip_phonon_large_max_dim())


def _check_solver(solver) -> str:
    if solver not in SOLVERS:
        raise ValueError(f"solver: one of 'lds', 'auto', 'blocked' expected (got {solver!r})")
    return solver


def plan_q_chunks(n_q: int, bytes_per_q: int, budget: int):
    """[(start, stop)]: the wave vectors 0 .. n_q - 1 in order, in chunks of as many as fit `budget` bytes of workspace at
    bytes_per_q each, one at least."""
    step = max(1, int(budget) // max(1, int(bytes_per_q)))
    return [(a, min(a + step, n_q)) for a in range(0, n_q, step)]


# ---- host helpers (numpy, fp64) ----------------------------------------------------------------------------------------------

def lattice_offsets(supercell) -> np.ndarray:
    """int [S1 S2 S3, 3]: the lattice offsets of the supercell's copies, the home cell (0, 0, 0) first, last index fastest."""
    a, b, c = (int(s) for s in supercell)
    return np.array([(i, j, k) for i in range(a) for j in range(b) for k in range(c)], dtype=np.int64).reshape(-1, 3)


def build_supercell(z, pos, cell, supercell):
    """(z [N], pos [N,3] fp64, cell [3,3] fp64) of the supercell of one primitive cell (z [n], pos [n,3], cell [3,3] with the
    lattice vectors as rows): atom R n + j is home atom j moved by offset R of lattice_offsets."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    L = lattice_offsets(supercell).astype(np.float64)
    big = (pos[None, :, :] + (L @ cell)[:, None, :]).reshape(-1, 3)
    return np.tile(np.asarray(z).reshape(-1), len(L)), big, np.asarray(supercell, dtype=np.float64).reshape(3, 1) * cell


def perpendicular_widths(cell) -> np.ndarray:
    """[3]: distance between the two faces of the cell that lattice vector k connects, V / |a_l x a_m|."""
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    vol = abs(np.linalg.det(cell))
    return np.array([vol / np.linalg.norm(np.cross(cell[(k + 1) % 3], cell[(k + 2) % 3])) for k in range(3)])


_T27 = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64)


def image_table(pos, cell, supercell, tol: float = TIE_TOL):
    """(start int32 [n N + 1], offsets fp64 [n_img, 3]) of one crystal: pair (i, J) owns offsets[start[i N + J]:start[i N + J + 1]],
    the nearest images r_J + T - r_i in units of the primitive lattice vectors, T in lexicographic order."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    S = np.asarray(supercell, dtype=np.float64).reshape(3)
    frac = pos @ np.linalg.inv(cell)
    n = len(pos)
    fJ = (lattice_offsets(supercell).astype(np.float64)[:, None, :] + frac[None, :, :]).reshape(-1, 3)
    # the home atoms in chunks (every row is independent, so the output does not depend on the chunk): x and x @ cell take
    # 2 x 27 x 3 x 8 bytes per pair
    rows = max(1, IMAGE_TABLE_BYTES // (1296 * max(1, len(fJ))))
    counts, kept = [], []
    for i0 in range(0, n, rows):
        x = fJ[None, :, None, :] - frac[i0:i0 + rows, None, None, :] + (_T27 * S)[None, None, :, :]      # [rows, N, 27, 3]
        dist = np.linalg.norm(x @ cell, axis=-1)
        keep = dist <= dist.min(axis=-1, keepdims=True) * (1.0 + tol)
        counts.append(keep.sum(axis=-1).reshape(-1))
        kept.append(x[keep])
    start = np.zeros(n * len(fJ) + 1, dtype=np.int64)
    if counts:
        np.cumsum(np.concatenate(counts), out=start[1:])
    if start[-1] >= 2 ** 31:
        raise NotImplementedError('image table above 2^31 entries')
    return start.astype(np.int32), np.ascontiguousarray(np.concatenate(kept) if kept else np.zeros((0, 3)))


def monkhorst_pack(n1: int, n2: int, n3: int, shift: bool = False) -> np.ndarray:
    """fp64 [n1 n2 n3, 3]: the full regular grid q_c = (k_c + s) / n_c, k_c = 0 .. n_c - 1, folded into [-1/2, 1/2); s = 0
    (the grid holds Gamma; mesh(S1, S2, S3) is the set commensurate with an S1 x S2 x S3 supercell) or s = 1/2 (shift=True).  Last
    index fastest, no symmetry reduction."""
    ns = []
    for n in (n1, n2, n3):
        if int(n) != n or int(n) < 1:
            raise ValueError(f'mesh: positive integers expected (got {(n1, n2, n3)!r})')
        ns.append(int(n))
    axes = [(np.arange(n, dtype=np.float64) + (0.5 if shift else 0.0)) / n for n in ns]
    axes = [u - np.floor(u + 0.5) for u in axes]
    g = np.stack(np.meshgrid(*axes, indexing='ij'), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(g)


def band_path(points, n_per_segment: int):
    """(q fp64 [Q, 3], ticks): the piecewise-linear path through `points` ([P, 3], fractional reciprocal coordinates) with
    n_per_segment points per segment (the start of a segment included, its end not) plus the last point; ticks[k] is the index
    of points[k] in q."""
    p = np.asarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 2 or not np.isfinite(p).all():
        raise ValueError('points: at least two finite [3] wave vectors expected')
    if int(n_per_segment) != n_per_segment or int(n_per_segment) < 1:
        raise ValueError(f'n_per_segment: a positive integer expected (got {n_per_segment!r})')
    m = int(n_per_segment)
    t = np.arange(m, dtype=np.float64)[:, None] / m
    q = [p[k][None, :] + t * (p[k + 1] - p[k])[None, :] for k in range(len(p) - 1)]
    q.append(p[-1:])
    return np.concatenate(q), [m * k for k in range(len(p))]


def path_length(q, cell) -> np.ndarray:
    """fp64 [Q]: cumulative length in 1 / Angstrom of the path q (fractional) in the reciprocal lattice 2 pi inv(cell)^T."""
    recip = 2.0 * np.pi * np.linalg.inv(np.asarray(cell, dtype=np.float64).reshape(3, 3)).T
    step = np.linalg.norm(np.diff(np.asarray(q, dtype=np.float64), axis=0) @ recip, axis=1)
    return np.concatenate([[0.0], np.cumsum(step)])


def _check_direction(direction, n_q: int):
    """None, or the unit fp64 [n_q, 3] of an explicit Cartesian direction ([3] or [n_q, 3], finite, non-zero)."""
    if direction is None:
        return None
    n = direction.detach().double().cpu().numpy() if isinstance(direction, torch.Tensor) else np.asarray(direction, dtype=np.float64)
    if n.shape not in ((3,), (n_q, 3)):
        raise ValueError(f'direction: [3] or [{n_q}, 3] Cartesian components expected (got shape {tuple(n.shape)})')
    n = np.broadcast_to(n, (n_q, 3))
    if not np.isfinite(n).all():
        raise ValueError('direction: finite components expected')
    norm = np.linalg.norm(n, axis=1, keepdims=True)
    if not (norm > 0.0).all():
        raise ValueError('direction: a non-zero vector expected')
    return np.ascontiguousarray(n / norm)


class _PerCrystal(list):
    """unit directions [Q, 3] per crystal: what band_structure hands frequencies in place of one direction for all crystals"""


def _check_degeneracy_tol(tol):
    if tol is not None and not (float(tol) >= 0.0 and math.isfinite(float(tol))):
        raise ValueError(f'degeneracy_tol: a finite value >= 0 (relative to max |lambda|) expected (got {tol!r})')
    return None if tol is None else float(tol)


def segment_directions(points, n_per_segment: int, cell) -> np.ndarray:
    """fp64 [Q, 3]: for every point of band_path(points, n_per_segment) the unit Cartesian direction of the segment it lies on in
    the reciprocal lattice of `cell`; a tick belongs to the segment it starts, the last point to the last segment."""
    p = np.asarray(points, dtype=np.float64)
    recip = 2.0 * np.pi * np.linalg.inv(np.asarray(cell, dtype=np.float64).reshape(3, 3)).T
    seg = (p[1:] - p[:-1]) @ recip
    norm = np.linalg.norm(seg, axis=1, keepdims=True)
    if not (norm > 0.0).all():
        raise ValueError('points: a segment of zero length has no direction (velocities=True)')
    seg = seg / norm
    m = int(n_per_segment)
    return np.ascontiguousarray(np.concatenate([np.repeat(seg, m, axis=0), seg[-1:]]))


def symmetric_cell(pos, cell):
    """(pos', cell') of one crystal (pos [n,3], cell [3,3], numpy fp64) rotated rigidly so that cell' is a symmetric matrix: the
    polar decomposition cell = P Q (P symmetric positive definite, Q a rotation for a right-handed cell), cell' = P and
    pos' = pos Q^T.  The form phonons() needs of a non-orthogonal cell (see there)."""
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    u, s, vh = np.linalg.svd(cell)
    return np.asarray(pos, dtype=np.float64).reshape(-1, 3) @ (u @ vh).T, (u * s[None, :]) @ u.T


def _supercells(supercell, n_cry: int) -> np.ndarray:
    s = supercell.detach().cpu().numpy() if isinstance(supercell, torch.Tensor) else np.asarray(supercell)
    if s.dtype.kind not in 'iu' or s.shape not in ((3,), (n_cry, 3)):
        raise ValueError(f'supercell: three integers, or an integer [{n_cry}, 3], expected (got {supercell!r})')
    s = np.broadcast_to(s.astype(np.int64), (n_cry, 3)).copy()
    if (s < 1).any():
        raise ValueError(f'supercell: every entry must be at least 1 (got {s.tolist()})')
    return s


def _cells(cell) -> np.ndarray:
    c = cell.detach().double().cpu().numpy().reshape(-1, 3, 3)
    for b in range(len(c)):
        if not np.isfinite(c[b]).all() or not (np.abs(c[b]).max() > 0) or abs(np.linalg.det(c[b])) <= 1e-12 * np.abs(c[b]).max() ** 3:
            raise ValueError(f'crystal {b}: a zero (or singular) cell has no phonon dispersion; use normal_modes for a molecule')
    return c


def _counts(batch, n_cry: int, n_atoms: int):
    counts = torch.bincount(batch.long().reshape(-1).cpu(), minlength=n_cry).tolist() if n_atoms else [0] * n_cry
    if len(counts) != n_cry:
        raise ValueError('batch names more crystals than cell holds')
    b = batch.long().reshape(-1).cpu()
    if n_atoms and bool((b[1:] < b[:-1]).any()):
        raise ValueError('batch: the atoms of a crystal must be contiguous and the crystals ascending')
    return counts


def _check_bound(counts, solver: str = 'lds'):
    bound, large = max_dim(), max_dim_large()
    for b, n in enumerate(counts):
        if 3 * n > large:
            raise NotImplementedError(f'crystal {b} has 3 x {n} = {3 * n} coordinates per primitive cell, above the {large} of '
                                      f'phonons.max_dim_large() (nnhip_phonon_large_max_dim), the bound of every solver')
        if solver == 'lds' and 3 * n > bound:
            raise NotImplementedError(f'crystal {b} has 3 x {n} = {3 * n} coordinates per primitive cell, above the {bound} of '
                                      f'phonons.max_dim() (nnhip_phonon_max_dim)')


# ---- results -------------------------------------------------------------------------------------------------------------------

class PhononBands:
    """Spectra of B crystals at Q wave vectors, packed per crystal (crystal b owns [Q, d_b] values at Q ptr[b]).

    eigenvalues  fp32 [Q sum d_b]   eV / (A^2 amu), ascending per (b, q)
    frequencies  fp32 [Q sum d_b]   cm^-1 = sign(lambda) sqrt(|lambda|) x 521.4709; negative = imaginary
    modes        complex64 [Q sum d_b^2] or None: per (b, q) a [d_b, d_b] matrix, ROW k = mode k (mass-weighted, unit norm, the
                 component of largest magnitude real and positive)
    dynamical_matrix  complex64, laid out like modes, or None
    sweeps, status    int32 [B, Q]  Jacobi sweeps used; status bit 0 = the sweep cap was hit (a non-finite force constant ends
                 there too), bit 1 = the device's cry_ptr gives the crystal more atoms than the host copy the launch was sized
                 from (a C caller's mismatch; a Phonons keeps the two equal), bit 2 = a mass that is not positive and finite.
                 With bit 1 or 2 nothing else of the problem is written
    q            fp64 numpy [Q, 3]; path (band_structure only): fp64 numpy [B, Q] cumulative length in 1 / Angstrom, ticks
    With velocities=True (None otherwise):
    group_velocities  fp32 [Q sum d_b, 3]  A / ps (= 100 m / s), Cartesian: the gradient of the signed frequency the library reports,
                 d lambda / d q_cart / (2 sqrt|lambda|).  Modes whose eigenvalues lie within the degeneracy tolerance of each other
                 are rotated so that the perturbation along the problem's direction n is diagonal (eigenvalues of n . dD/dq
                 ascending), which is what follows a band through a crossing along n.  Inside a subgroup that n . dD/dq leaves
                 degenerate the individual values depend on the basis; their sum over the subgroup does not.
    velocity_defined  bool [Q sum d_b]  False (and v = 0) for |lambda| <= the zero tolerance -- the acoustic modes at Gamma, whose limit
                 depends on the direction -- and for the modes of a group above MAX_DEGENERATE (status bit 3 = STATUS_GROUP).
                 status bit 4 = STATUS_NONFINITE: a non-finite eigenvalue or mode, nothing of the problem is defined
    degenerate_group  int32 [Q sum d_b]  per mode, the index (within its [d_b]) of the first mode of its group
    eigenvalue_gradients  fp32 [Q sum d_b, 3]  d lambda / d q_cart in eV / (A amu), what the velocities are made of (also where
                 velocity_defined is False for a zero mode; zero for a group above the cap)
    """

    def __init__(self, **kw):
        self.path = None
        self.ticks = None
        self.group_velocities = None
        self.velocity_defined = None
        self.degenerate_group = None
        self.eigenvalue_gradients = None
        self.__dict__.update(kw)

    def crystal(self, b: int):
        """(eigenvalues [Q, d], frequencies [Q, d], modes [Q, d, d] or None) of crystal b: views, no copy."""
        Q, d, o = len(self.q), self._dims[b], self._offsets[b]
        ev = self.eigenvalues[Q * o:Q * (o + d)].view(Q, d)
        fr = self.frequencies[Q * o:Q * (o + d)].view(Q, d)
        return ev, fr, self._square(self.modes, b)

    def _square(self, x, b):
        if x is None:
            return None
        Q, d, o = len(self.q), self._dims[b], self._sq_offsets[b]
        return x[Q * o:Q * (o + d * d)].view(Q, d, d)

    def velocities(self, b: int):
        """(group velocities [Q, d, 3] in A / ps, velocity_defined [Q, d]) of crystal b: views (velocities=True only)."""
        if self.group_velocities is None:
            raise ValueError('no group velocities: ask for them with velocities=True')
        Q, d, o = len(self.q), self._dims[b], self._offsets[b]
        return self.group_velocities[Q * o:Q * (o + d)].view(Q, d, 3), self.velocity_defined[Q * o:Q * (o + d)].view(Q, d)

    def dynamical(self, b: int):
        """D(q) of crystal b as complex64 [Q, d, d] (frequencies(..., dynamical_matrix=True) only)."""
        return self._square(self.dynamical_matrix, b)


class PhononDOS:
    """frequencies fp32 [n_bins] (bin centres, cm^-1), dos fp32 [B, n_bins] in states per cm^-1 per primitive cell (it
    integrates to d_b over the range), counts int32 [B, n_bins] or None (histogram form), bin_width."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class PhononThermochemistry:
    """ZPE, U, F (eV) and S, Cv (eV / K) per primitive cell, fp32 [B], at `temperature` (K), averaged over the mesh;
    n_skipped_zero / n_skipped_imaginary int64 [B]: the (q, mode) pairs of the mesh left out."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class PhononMesh:
    """The spectra of a regular mesh (Phonons.mesh): `bands` (a PhononBands over the mesh points, equal weights)."""

    def __init__(self, bands: PhononBands, phonons: 'Phonons'):
        self.bands = bands
        self._ph = phonons

    def dos(self, n_bins: int, width: Optional[float] = None, lo: Optional[float] = None, hi: Optional[float] = None) -> PhononDOS:
        """Density of states over n_bins equal bins of [lo, hi] cm^-1 (nnhip_phonon_dos: one thread per bin walks the mesh's
        modes in a fixed order).  width=None: the plain histogram, integer counts / (Q bin_width); width (cm^-1): every mode
        a unit Gaussian of that standard deviation, evaluated at the bin centres.  lo / hi default to the spectrum's range over
        the whole batch, widened by a thousandth of it (by 5 widths for the Gaussian form) so that nothing falls outside."""
        if int(n_bins) != n_bins or int(n_bins) < 1:
            raise ValueError(f'n_bins: a positive integer expected (got {n_bins!r})')
        if width is not None and not (float(width) > 0.0 and math.isfinite(float(width))):
            raise ValueError(f'width: a finite value > 0 cm^-1 expected (got {width!r})')
        bands, ph = self.bands, self._ph
        f = bands.frequencies
        if lo is None or hi is None:
            fmin, fmax = (float(f.min()), float(f.max())) if f.numel() else (0.0, 1.0)
            pad = 5.0 * float(width) if width is not None else 1e-3 * max(fmax - fmin, 1.0)
            lo = fmin - pad if lo is None else lo
            hi = fmax + pad if hi is None else hi
        lo, hi = float(lo), float(hi)
        if not (hi > lo and math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f'lo < hi, both finite, expected (got {lo!r}, {hi!r})')
        n_bins, Q, B, dev = int(n_bins), len(bands.q), len(ph.counts), f.device
        val_ptr = (Q * 3 * ph.cry_ptr.long()).contiguous()
        counts = torch.zeros(B, n_bins, dtype=torch.int32, device=dev) if width is None else None
        dens = torch.zeros(B, n_bins, dtype=torch.float32, device=dev) if width is not None else None
        hip._check(hip.lib().nnhip_phonon_dos(hip._ptr(f), hip._ptr(val_ptr), B, lo, hi, n_bins, 0.0 if width is None else float(width),
                                              hip._ptr(counts), hip._ptr(dens), hip._stream(dev)), 'nnhip_phonon_dos')
        # the bins as the kernel sees them (fp32)
        lo32, hi32 = np.float32(lo), np.float32(hi)
        wbin = float((hi32 - lo32) / np.float32(n_bins))
        centres = torch.tensor(lo32 + (np.arange(n_bins, dtype=np.float32) + np.float32(0.5)) * np.float32(wbin), device=dev)
        dos = counts.float() / (Q * wbin) if width is None else dens / Q
        return PhononDOS(frequencies=centres, dos=dos, counts=counts, bin_width=wbin, lo=float(lo32), hi=float(hi32))

    def threshold(self, tol_zero: Optional[float] = None) -> torch.Tensor:
        """fp32 [B]: tol_zero max |lambda| over the crystal's mesh (default tol_zero: 8 x 2 d x 2^-24, the solver's bound for a
        complex d x d problem).  A mode is live iff lambda > threshold and imaginary iff lambda < -threshold."""
        bands, ph = self.bands, self._ph
        out = []
        for b, n in enumerate(ph.counts):
            ev = bands.crystal(b)[0]
            tol = 8.0 * EPS32 * 6 * n if tol_zero is None else float(tol_zero)
            out.append(tol * ev.abs().max() if ev.numel() else ev.new_zeros(()))
        return torch.stack(out) if out else torch.zeros(0, device=bands.eigenvalues.device)

    def thermochemistry(self, temperature: float, tol_zero: Optional[float] = None) -> PhononThermochemistry:
        """Harmonic thermochemistry per primitive cell at `temperature` (K): the per-mode terms of
        NormalModes.thermochemistry (x = eps / k_B T, eps = hbar omega)
            ZPE = eps / 2,  U = eps / 2 + eps / (e^x - 1),  S = k_B (x / (e^x - 1) - ln(1 - e^-x)),
            F = eps / 2 + k_B T ln(1 - e^-x),  C_v = k_B x^2 e^-x / (1 - e^-x)^2
        summed over the live modes of every mesh point and divided by the number of points.  Modes with |lambda| <= threshold
        (the three acoustic ones at Gamma) and imaginary ones are skipped and counted.  Elementwise torch ops in fp64 on the
        device; T = 0 returns U = F = ZPE and S = C_v = 0."""
        T = _v._temperature(temperature)
        bands, ph = self.bands, self._ph
        Q, dev = len(bands.q), bands.eigenvalues.device
        thr = self.threshold(tol_zero)
        rows, n_zero, n_imag = [], [], []
        for b in range(len(ph.counts)):
            ev = bands.crystal(b)[0].reshape(-1).double()
            live, imag = ev > thr[b], ev < -thr[b]
            n_imag.append(imag.sum())
            n_zero.append((~live & ~imag).sum())
            eps = _v.EV_PER_SQRT_EIGENVALUE * torch.where(live, ev, torch.ones_like(ev)).sqrt()
            if T == 0.0:
                terms = torch.stack([0.5 * eps] + [torch.zeros_like(eps)] * 4, dim=1)
            else:
                kT = _v.K_BOLTZMANN * T
                x = (eps / kT).clamp(max=100.0)
                em, om = torch.exp(-x), -torch.expm1(-x)
                occ, ln = em / om, torch.log(om)
                terms = torch.stack([0.5 * eps, eps * occ, _v.K_BOLTZMANN * (x * occ - ln), kT * ln,
                                     _v.K_BOLTZMANN * x * x * em / (om * om)], dim=1)
            rows.append(torch.where(live[:, None], terms, torch.zeros_like(terms)).sum(dim=0) / max(Q, 1))
        s = torch.stack(rows) if rows else torch.zeros(0, 5, dtype=torch.float64, device=dev)
        zpe = s[:, 0]
        return PhononThermochemistry(ZPE=zpe.float(), U=(zpe + s[:, 1]).float(), S=s[:, 2].float(), F=(zpe + s[:, 3]).float(),
                                     Cv=s[:, 4].float(), temperature=T, threshold=thr,
                                     n_skipped_zero=torch.stack(n_zero) if n_zero else torch.zeros(0, dtype=torch.long, device=dev),
                                     n_skipped_imaginary=torch.stack(n_imag) if n_imag else torch.zeros(0, dtype=torch.long, device=dev))


    def transport_tensor(self, temperature: float, tol_zero: Optional[float] = None) -> torch.Tensor:
        """fp32 [B, 3, 3]: (1 / (Q V)) sum_{q, s} C_v(omega_qs, T) v_a v_b over the live modes (lambda > threshold(tol_zero), as
        thermochemistry selects and counts them) whose velocity is defined, V the volume of the primitive cell: kappa / tau of
        the constant-relaxation-time approximation, in W / (m K) per ps of relaxation time.  fp64 torch ops on the device.
        Needs a mesh made with velocities=True (ValueError otherwise)."""
        bands, ph = self.bands, self._ph
        if bands.group_velocities is None:
            raise ValueError('transport_tensor needs group velocities: make the mesh with velocities=True')
        T = _v._temperature(temperature)
        Q, dev = len(bands.q), bands.eigenvalues.device
        thr = self.threshold(tol_zero)
        out = []
        for b in range(len(ph.counts)):
            ev = bands.crystal(b)[0].reshape(-1).double()
            v, ok = bands.velocities(b)
            v, live = v.reshape(-1, 3).double(), (ev > thr[b]) & ok.reshape(-1)
            if T == 0.0:
                cv = torch.zeros_like(ev)
            else:
                eps = _v.EV_PER_SQRT_EIGENVALUE * torch.where(live, ev, torch.ones_like(ev)).sqrt()
                x = (eps / (_v.K_BOLTZMANN * T)).clamp(max=100.0)
                em, om = torch.exp(-x), -torch.expm1(-x)
                cv = _v.K_BOLTZMANN * x * x * em / (om * om)
            w = torch.where(live, cv, torch.zeros_like(cv))
            vol = abs(float(np.linalg.det(ph._cells[b])))
            out.append((w[:, None, None] * v[:, :, None] * v[:, None, :]).sum(dim=0) * (WATT_PER_M_K_PER_PS / (max(Q, 1) * vol)))
        return (torch.stack(out) if out else torch.zeros(0, 3, 3, dtype=torch.float64, device=dev)).float()


class Phonons:
    """Force constants of B crystals on their supercells, ready for any number of wave vectors.

    fc           fp32, packed [n_b, 3, N_b, 3] per crystal at fc_ptr[b] (force_constants(b) is the view)
    counts, sc_counts   atoms per primitive cell n_b / per supercell N_b (lists)
    supercell    int numpy [B, 3]
    masses       fp32 [n] amu;  z, pos, cell: the primitive cells
    solver       'lds' | 'auto' | 'blocked': the default of frequencies / band_structure / mesh (see frequencies)
    """

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def force_constants(self, b: int) -> torch.Tensor:
        o, n, N = self._fc_offsets[b], self.counts[b], self.sc_counts[b]
        return self.fc[o:o + 9 * n * N].view(n, 3, N, 3)

    @classmethod
    def from_force_constants(cls, fc, z, pos, cell, supercell, masses=None, batch=None, device=None,
                             solver: str = 'lds') -> 'Phonons':
        """A Phonons from force constants the caller has: fc is one [n, 3, N, 3] array / tensor, a list of them (one per
        crystal), or the packed 1-d tensor; z [n_total], pos [n_total, 3], cell [B, 3, 3] (or [3, 3]) are the primitive cells,
        batch [n_total] their crystal index (None: one crystal).  N_b must be n_b x prod(supercell_b), the supercell atoms in the
        order of build_supercell.  masses: amu per home atom (None: standard atomic weights of z).  No width check and no
        acoustic sum rule: the force constants are taken as they are.  device: where the tables go (default: that of fc when
        it is a tensor, else of pos when it is one, else 'cuda').  solver: see frequencies; 'lds' refuses a primitive cell above
        max_dim() coordinates here, every solver one above max_dim_large()."""
        _check_solver(solver)
        if device is None:
            src = fc if isinstance(fc, torch.Tensor) else fc[0] if isinstance(fc, (list, tuple)) and fc and \
                isinstance(fc[0], torch.Tensor) else pos if isinstance(pos, torch.Tensor) else None
            device = src.device if src is not None else torch.device('cuda')
        device = torch.device(device)
        pos_t = torch.as_tensor(np.asarray(pos) if not isinstance(pos, torch.Tensor) else pos).detach().reshape(-1, 3)
        cell_t = torch.as_tensor(np.asarray(cell) if not isinstance(cell, torch.Tensor) else cell).detach().reshape(-1, 3, 3)
        z_t = torch.as_tensor(np.asarray(z) if not isinstance(z, torch.Tensor) else z).detach().reshape(-1).long()
        n_total, B = pos_t.shape[0], cell_t.shape[0]
        if z_t.numel() != n_total:
            raise ValueError(f'z: {z_t.numel()} values for {n_total} atoms')
        if batch is None:
            if B != 1:
                raise ValueError(f'batch: needed with {B} crystals')
            batch_t = torch.zeros(n_total, dtype=torch.long)
        else:
            batch_t = torch.as_tensor(np.asarray(batch) if not isinstance(batch, torch.Tensor) else batch).detach().reshape(-1).long()
            if batch_t.numel() != n_total:
                raise ValueError(f'batch: {batch_t.numel()} values for {n_total} atoms')
        cells = _cells(cell_t)
        S = _supercells(supercell, B)
        counts = _counts(batch_t, B, n_total)
        sc_counts = [n * int(np.prod(S[b])) for b, n in enumerate(counts)]
        sizes = [9 * n * N for n, N in zip(counts, sc_counts)]
        if isinstance(fc, (list, tuple)) or (hasattr(fc, 'ndim') and fc.ndim == 4):
            parts = [fc] if not isinstance(fc, (list, tuple)) else list(fc)
            if len(parts) != B:
                raise ValueError(f'fc: {len(parts)} blocks for {B} crystals')
            flat = []
            for b, p in enumerate(parts):
                p = torch.as_tensor(np.asarray(p) if not isinstance(p, torch.Tensor) else p).detach()
                if tuple(p.shape) != (counts[b], 3, sc_counts[b], 3):
                    raise ValueError(f'fc of crystal {b}: [{counts[b]}, 3, {sc_counts[b]}, 3] expected (got {tuple(p.shape)})')
                flat.append(p.to(device=device, dtype=torch.float32).reshape(-1))
            fc_t = torch.cat(flat) if flat else torch.zeros(0, dtype=torch.float32, device=device)
        else:
            fc_t = torch.as_tensor(fc).detach()
            if fc_t.dim() != 1 or fc_t.numel() != sum(sizes):
                raise ValueError(f'fc: packed 1-d with {sum(sizes)} values expected (got {tuple(fc_t.shape)})')
            fc_t = hip._f32c(fc_t, 'fc').to(device)
        _check_bound(counts, solver)
        if masses is None:
            m_t = _v.table_masses(z_t)
        else:
            m_t = torch.as_tensor(np.asarray(masses) if not isinstance(masses, torch.Tensor) else masses).detach().reshape(-1)
            if m_t.numel() != n_total:
                raise ValueError(f'masses: {m_t.numel()} values for {n_total} atoms')
        return cls._assemble(fc_t.contiguous(), z_t, pos_t, cell_t, cells, S, counts, sc_counts, m_t, device, solver)

    @classmethod
    def _assemble(cls, fc_t, z_t, pos_t, cell_t, cells, S, counts, sc_counts, m_t, device, solver: str = 'lds') -> 'Phonons':
        """the image tables (host, fp64, once per crystal) and the offset arrays of nnhip_phonon_bands"""
        B = len(counts)
        pos_h = pos_t.detach().double().cpu().numpy()
        cry = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(counts, out=cry[1:])
        starts, offs, img_ptr, n_off = [], [], [], 0
        for b in range(B):
            st, off = image_table(pos_h[cry[b]:cry[b + 1]], cells[b], S[b])
            img_ptr.append(sum(len(s) for s in starts))
            starts.append(st.astype(np.int64) + n_off)
            offs.append(off)
            n_off += len(off)
        if n_off >= 2 ** 31:
            raise NotImplementedError('image tables above 2^31 entries in one batch')
        sizes = np.array([9 * n * N for n, N in zip(counts, sc_counts)], dtype=np.int64)
        sq = np.array([9 * n * n for n in counts], dtype=np.int64)

        def dev(a, dtype):
            return torch.tensor(np.asarray(a), dtype=dtype).to(device)
        cry_host = torch.tensor(cry, dtype=torch.int32)
        return cls(fc=fc_t, fc_ptr=dev(np.cumsum(sizes) - sizes, torch.int64), _fc_offsets=(np.cumsum(sizes) - sizes).tolist(),
                   counts=list(counts), sc_counts=list(sc_counts), supercell=S, masses=m_t.to(device=device, dtype=torch.float32).contiguous(),
                   z=z_t.to(device), pos=pos_t.to(device), cell=cell_t.to(device), _cells=cells,
                   cry_ptr=cry_host.to(device), _cry_host=cry_host, sc_atoms=dev(sc_counts, torch.int32),
                   img_ptr=dev(img_ptr, torch.int64),
                   img_start=dev(np.concatenate(starts) if starts else np.zeros(0), torch.int32),
                   img_off=dev(np.concatenate(offs) if offs else np.zeros((0, 3)), torch.float64).contiguous(),
                   out_ptr=dev(np.cumsum(sq) - sq, torch.int64), _sq_offsets=(np.cumsum(sq) - sq).tolist(),
                   _offsets=(3 * cry[:-1]).tolist(), _dims=[3 * n for n in counts], solver=solver)

    # ---- wave vectors ---------------------------------------------------------------------------------------------------------
    def frequencies(self, q, modes: bool = False, dynamical_matrix: bool = False, solver: Optional[str] = None,
                    workspace_bytes: Optional[int] = None, velocities: bool = False, direction=None,
                    degeneracy_tol: Optional[float] = None) -> PhononBands:
        """The spectra at the wave vectors q ([Q, 3], units of the primitive reciprocal vectors, shared by all crystals).
        modes=True also returns the eigenvectors; the eigenvalues are bitwise the same either way, and those of a q do not
        depend on the other q of the call.  dynamical_matrix=True also returns D(q).
        solver (None: the object's): 'lds' -- one launch of nnhip_phonon_bands, NotImplementedError above max_dim() = 96
        coordinates; 'auto' -- crystals up to max_dim() through nnhip_phonon_bands, bitwise as under 'lds', the others through the
        blocked solver nnhip_phonon_bands_large (up to max_dim_large() = 768 coordinates; sweeps counts its OUTER sweeps);
        'blocked' -- every crystal through the blocked solver.  All land in one packed PhononBands.  The blocked solver works in
        a torch-owned workspace; the wave vectors are served in chunks whose workspace stays within workspace_bytes (None:
        LARGE_WORKSPACE_BYTES; a chunk holds one q at least) -- the result does not depend on the chunking.
        velocities=True also returns the group velocities (PhononBands.group_velocities, velocity_defined, degenerate_group): the
        modes are computed (and dropped again unless modes=True) and ONE launch of nnhip_phonon_velocities follows, whatever the
        solver (band_structure's per-crystal directions: one launch per crystal); everything else of the result is bitwise what it is without the option.  direction: the Cartesian direction n
        along which degenerate groups are split, [3] or [Q, 3], normalised here (None: that of q itself, q_cart / |q_cart|, and
        (1, 0, 0) at q = 0).  degeneracy_tol: consecutive eigenvalues no more than degeneracy_tol max |lambda| apart (the maximum
        over the crystal's spectra of the call) form a group; None: 8 x 2 d x 2^-24, the formula of PhononMesh.threshold, which is
        also the tolerance below which |lambda| counts as zero.  Both tolerances are one number per crystal and call (the ABI
        takes them per crystal), so they depend on which q share the call: the arithmetic of a (crystal, q) does not, but a gap or
        an eigenvalue that lies between the tolerances of two calls is grouped, or flagged as zero, in one and not in the other."""
        solver = _check_solver(self.solver if solver is None else solver)
        qh = q.detach().double().cpu().numpy() if isinstance(q, torch.Tensor) else np.asarray(q, dtype=np.float64)
        qh = np.ascontiguousarray(qh.reshape(-1, 3) if qh.size else qh.reshape(0, 3))
        if not np.isfinite(qh).all():
            raise ValueError('q: finite wave vectors expected')
        dirs = direction if isinstance(direction, _PerCrystal) else _check_direction(direction, len(qh))
        degeneracy_tol = _check_degeneracy_tol(degeneracy_tol)
        want_modes, modes = modes, bool(modes or velocities)
        _check_bound(self.counts, solver)
        dev = self.fc.device
        if dev.type != 'cuda':
            raise RuntimeError('newtonnet_amd phonons run on an MI355X (ROCm) device only: build the Phonons on "cuda"')
        Q, B = len(qh), len(self.counts)
        n_val, n_sq = 3 * sum(self.counts), sum(9 * n * n for n in self.counts)
        evals = torch.zeros(Q * n_val, dtype=torch.float32, device=dev)
        vec = torch.zeros(Q * n_sq, 2, dtype=torch.float32, device=dev) if modes else None
        dm = torch.zeros(Q * n_sq, 2, dtype=torch.float32, device=dev) if dynamical_matrix else None
        sweeps, status = (torch.zeros(B, Q, dtype=torch.int32, device=dev) for _ in range(2))
        q_dev = torch.tensor(qh, dtype=torch.float64).to(dev)
        if B and Q and n_val:
            bound = max_dim()
            large = [False] * B if solver == 'lds' else [n > 0 and (solver == 'blocked' or 3 * n > bound) for n in self.counts]
            b = 0
            while b < B:   # nnhip_phonon_bands on every run of consecutive crystals it serves: the same call, the per-crystal pointers moved up
                if large[b]:
                    b += 1
                    continue
                e = b
                while e < B and not large[e]:
                    e += 1
                if sum(self.counts[b:e]):
                    rc = hip.lib().nnhip_phonon_bands(hip._ptr(self.fc), self.fc_ptr.data_ptr() + 8 * b, self.cry_ptr.data_ptr() + 4 * b,
                                                      self._cry_host.data_ptr() + 4 * b, self.sc_atoms.data_ptr() + 4 * b,
                                                      self.img_ptr.data_ptr() + 8 * b, hip._ptr(self.img_start), hip._ptr(self.img_off),
                                                      hip._ptr(self.masses), self.out_ptr.data_ptr() + 8 * b, e - b, hip._ptr(q_dev), Q,
                                                      hip._ptr(evals), hip._ptr(vec), hip._ptr(dm), sweeps.data_ptr() + 4 * Q * b,
                                                      status.data_ptr() + 4 * Q * b, hip._stream(dev))
                    if rc == 2:
                        raise NotImplementedError(hip.lib().nnhip_last_error().decode())
                    hip._check(rc, 'nnhip_phonon_bands')
                b = e
            if any(large):
                self._bands_large(large, q_dev, evals, vec, dm, sweeps, status,
                                  LARGE_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes))
        freq = torch.sign(evals) * evals.abs().sqrt() * _v.WAVENUMBER_PER_SQRT_EIGENVALUE
        extra = self._velocities(q_dev, evals, vec, status, dirs, degeneracy_tol) if velocities else {}
        return PhononBands(eigenvalues=evals, frequencies=freq,
                           modes=None if vec is None or not want_modes else torch.view_as_complex(vec),
                           dynamical_matrix=None if dm is None else torch.view_as_complex(dm), sweeps=sweeps, status=status, q=qh,
                           _dims=self._dims, _offsets=self._offsets, _sq_offsets=self._sq_offsets, **extra)

    def _velocities(self, q_dev, evals, vec, status, dirs, degeneracy_tol):
        """nnhip_phonon_velocities on the assembled spectra of a call: ONE launch (dirs None or one [Q, 3] for all crystals), or one
        per crystal (dirs a _PerCrystal of [Q, 3]: band_structure's segment directions depend on the crystal's cell).  status takes the
        new bits."""
        dev, B, Q = self.fc.device, len(self.counts), q_dev.shape[0]
        n_val = 3 * sum(self.counts)
        vel, dlam = (torch.zeros(Q * n_val, 3, dtype=torch.float32, device=dev) for _ in range(2))
        group = torch.zeros(Q * n_val, dtype=torch.int32, device=dev)
        defined = torch.zeros(Q * n_val, dtype=torch.uint8, device=dev)
        vstatus = torch.zeros(B, Q, dtype=torch.int32, device=dev)
        if B and Q and n_val:
            # max |lambda| per crystal over the call: one segmented reduction (a crystal without atoms gives 0)
            lengths = torch.tensor([Q * d for d in self._dims], dtype=torch.int64).to(dev)
            scale = torch.segment_reduce(evals.abs(), 'max', lengths=lengths, unsafe=True).clamp_min(0.0)
            default = torch.tensor([8.0 * EPS32 * 2 * d for d in self._dims], dtype=torch.float32, device=dev)
            zero_tol = (default * scale).contiguous()
            deg_tol = zero_tol if degeneracy_tol is None else (degeneracy_tol * scale).contiguous()
            cells = torch.tensor(np.asarray(self._cells, dtype=np.float64).reshape(B, 3, 3), dtype=torch.float64).to(dev).contiguous()
            runs = [(0, B, dirs)] if not isinstance(dirs, _PerCrystal) else [(b, b + 1, dirs[b]) for b in range(B) if self.counts[b]]
            for b, e, n in runs:
                n_dev = None if n is None else torch.tensor(n, dtype=torch.float64).to(dev).contiguous()
                rc = hip.lib().nnhip_phonon_velocities(
                    hip._ptr(self.fc), self.fc_ptr.data_ptr() + 8 * b, self.cry_ptr.data_ptr() + 4 * b, self._cry_host.data_ptr() + 4 * b,
                    self.sc_atoms.data_ptr() + 4 * b, self.img_ptr.data_ptr() + 8 * b, hip._ptr(self.img_start), hip._ptr(self.img_off),
                    hip._ptr(self.masses), self.out_ptr.data_ptr() + 8 * b, e - b, cells.data_ptr() + 72 * b, hip._ptr(q_dev), Q,
                    hip._ptr(n_dev), hip._ptr(evals), hip._ptr(vec), deg_tol.data_ptr() + 4 * b, zero_tol.data_ptr() + 4 * b,
                    hip._ptr(vel), hip._ptr(dlam), hip._ptr(group), hip._ptr(defined), vstatus.data_ptr() + 4 * Q * b, hip._stream(dev))
                if rc == 2:
                    raise NotImplementedError(hip.lib().nnhip_last_error().decode())
                hip._check(rc, 'nnhip_phonon_velocities')
            status |= vstatus
        return dict(group_velocities=vel * ANGSTROM_PER_PS_PER_SQRT_EV_AMU, velocity_defined=defined.bool(), degenerate_group=group,
                    eigenvalue_gradients=dlam)

    def _bands_large(self, large, q_dev, evals, vec, dm, sweeps, status, budget: int):
        """nnhip_phonon_bands_large on the crystals `large` selects, the wave vectors in chunks (plan_q_chunks).  A chunk that is not
        the whole call writes outputs of its own, which are copied into place: the kernels lay a crystal's values out by the
        number of wave vectors of their call."""
        L, dev, B, Q = hip.lib(), self.fc.device, len(self.counts), q_dev.shape[0]
        select = torch.tensor(large, dtype=torch.uint8)
        want = 0 if vec is None else 1

        def ws_bytes(n_q):
            return int(L.nnhip_phonon_large_ws_bytes(self._cry_host.data_ptr(), B, n_q, want, select.data_ptr()))

        def run(q_c, n_q, ev_c, vec_c, dm_c, sw_c, st_c):
            nbytes = ws_bytes(n_q)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rc = L.nnhip_phonon_bands_large(hip._ptr(self.fc), hip._ptr(self.fc_ptr), hip._ptr(self.cry_ptr), self._cry_host.data_ptr(),
                                            hip._ptr(self.sc_atoms), hip._ptr(self.img_ptr), hip._ptr(self.img_start),
                                            hip._ptr(self.img_off), hip._ptr(self.masses), hip._ptr(self.out_ptr), B, hip._ptr(q_c), n_q,
                                            hip._ptr(ev_c), hip._ptr(vec_c), hip._ptr(dm_c), hip._ptr(sw_c), hip._ptr(st_c),
                                            select.data_ptr(), hip._ptr(ws), nbytes, hip._stream(dev))
            if rc == 2:
                raise NotImplementedError(L.nnhip_last_error().decode())
            hip._check(rc, 'nnhip_phonon_bands_large')

        chunks = plan_q_chunks(Q, ws_bytes(1), budget)
        if len(chunks) == 1:
            run(q_dev, Q, evals, vec, dm, sweeps, status)
            return
        n_val, n_sq = 3 * sum(self.counts), sum(9 * n * n for n in self.counts)
        for q0, q1 in chunks:
            C = q1 - q0
            ev_c = torch.zeros(C * n_val, dtype=torch.float32, device=dev)
            vec_c = None if vec is None else torch.zeros(C * n_sq, 2, dtype=torch.float32, device=dev)
            dm_c = None if dm is None else torch.zeros(C * n_sq, 2, dtype=torch.float32, device=dev)
            sw_c, st_c = (torch.zeros(B, C, dtype=torch.int32, device=dev) for _ in range(2))
            run(q_dev[q0:q1].contiguous(), C, ev_c, vec_c, dm_c, sw_c, st_c)
            for b in range(B):
                if not large[b]:
                    continue
                d, o, so = self._dims[b], self._offsets[b], self._sq_offsets[b]
                evals[Q * o:Q * (o + d)].view(Q, d)[q0:q1] = ev_c[C * o:C * (o + d)].view(C, d)
                for full, part in ((vec, vec_c), (dm, dm_c)):
                    if full is not None:
                        full[Q * so:Q * (so + d * d)].view(Q, d * d, 2)[q0:q1] = part[C * so:C * (so + d * d)].view(C, d * d, 2)
                sweeps[b, q0:q1] = sw_c[b]
                status[b, q0:q1] = st_c[b]

    def band_structure(self, points, n_per_segment: int = 20, modes: bool = False, solver: Optional[str] = None,
                       velocities: bool = False) -> PhononBands:
        """frequencies() along the piecewise-linear path through `points` (band_path); the result also holds `path`, the
        cumulative length in 1 / Angstrom per crystal [B, Q], and `ticks`, the indices of the given points.  velocities=True:
        the group velocities, degenerate groups split along the Cartesian direction of the segment a point lies on (a tick belongs
        to the segment it starts, the last point to the last segment)."""
        q, ticks = band_path(points, n_per_segment)
        if velocities:
            dirs = _PerCrystal(segment_directions(points, n_per_segment, c) for c in self._cells)
            bands = self.frequencies(q, modes=modes, solver=solver, velocities=True, direction=dirs)
        else:
            bands = self.frequencies(q, modes=modes, solver=solver)
        bands.path = np.stack([path_length(q, c) for c in self._cells]) if len(self._cells) else np.zeros((0, len(q)))
        bands.ticks = ticks
        return bands

    def mesh(self, n1: int, n2: int, n3: int, shift: bool = False, solver: Optional[str] = None, velocities: bool = False) -> PhononMesh:
        """The spectra on the full n1 x n2 x n3 grid of monkhorst_pack (no symmetry reduction), eigenvalues only; velocities=True:
        with the group velocities (direction=None: groups split along q itself), which PhononMesh.transport_tensor needs."""
        if not velocities:
            return PhononMesh(self.frequencies(monkhorst_pack(n1, n2, n3, shift), solver=solver), self)
        return PhononMesh(self.frequencies(monkhorst_pack(n1, n2, n3, shift), solver=solver, velocities=True), self)


# ---- from a model ----------------------------------------------------------------------------------------------------------------

def _validate_model(model):
    if model.training:
        raise NotImplementedError('phonons run in eval mode only (training on Hessian labels is not supported): call model.eval()')
    if 'energy' not in list(model.output_properties):
        raise NotImplementedError("the force constants are the energy's: the model needs the 'energy' head (output_properties)")


def acoustic_sum_rule(phi: torch.Tensor) -> torch.Tensor:
    """Phi(i, i) <- Phi(i, i) - sum_J Phi(i, J) over ALL supercell atoms J (i itself included), then that 3 x 3 block symmetrised;
    phi is [n, 3, N, 3] with the home atoms first (returns a new tensor)."""
    phi = phi.clone()
    n = phi.shape[0]
    s = phi.double().sum(dim=2)                                    # [n, 3, 3]
    idx = torch.arange(n, device=phi.device)
    blk = phi[idx, :, idx, :].double() - s
    phi[idx, :, idx, :] = (0.5 * (blk + blk.transpose(1, 2))).to(phi.dtype)
    return phi


def phonons(model, z, pos, cell, batch, supercell, masses: Optional[torch.Tensor] = None, asr: bool = True,
            solver: str = 'lds') -> Phonons:
    """Force constants of every primitive cell of the batch on its supercell at the current parameters (see the module text).
    supercell: three integers, or an integer [B, 3].  Every perpendicular width of a supercell must be at least twice the
    model's cutoff (its neighbour list takes one minimum image): ValueError otherwise, before any kernel.  A cell that is not
    orthogonal must be given as a symmetric matrix (symmetric_cell rotates any crystal into that form): the model's minimum-image
    shift is a lattice vector for such cells only.  masses: fp32 [N] amu
    (None: standard atomic weights of z).  asr: impose the acoustic sum rule on the fp32 force constants.  solver: 'lds' (default:
    primitive cells up to max_dim() = 96 coordinates), 'auto' or 'blocked' (up to max_dim_large() = 768): kept on the result as
    the default of its frequencies / band_structure / mesh (see Phonons.frequencies)."""
    _check_solver(solver)
    cells, S, counts = _checked_crystals(model, z, pos, cell, batch, supercell, lambda c: _check_bound(c, solver))
    n_atoms = pos.shape[0]
    if masses is not None and masses.numel() != n_atoms:
        raise ValueError(f'masses: {masses.numel()} values for {n_atoms} atoms')
    m = _v.table_masses(z) if masses is None else masses.detach().reshape(-1)
    if not pos.is_cuda:
        raise RuntimeError('newtonnet_amd phonons run on an MI355X (ROCm) device only: move the model and the inputs to "cuda"')
    dev = pos.device
    fc_t, sc_counts = _force_constants(model, z, pos, cells, S, counts, asr, dev)
    return Phonons._assemble(fc_t, z.detach().reshape(-1).long(), pos.detach(), cell.detach(), cells, S, counts, sc_counts, m, dev,
                             solver)


def _force_constants(model, z, pos, cells, S, counts, asr: bool, dev):
    """(fc fp32 packed [n_b, 3, N_b, 3] per crystal, atoms per supercell): the force-constant body of phonons(), shared with
    newtonnet_amd/gruneisen.py, which runs it at strained cells.  cells, S, counts: what _checked_crystals returned."""
    z_sc, pos_sc, cell_sc, batch_sc, sc_counts = _supercell_batch(z, pos, cells, S, counts, dev)
    with torch.no_grad():
        blocks, blk_ptr, _ = _hessian.hessian_blocks_counts(model, z_sc, pos_sc, cell_sc, batch_sc, n_dirs=3 * max(counts))
    ptr = blk_ptr.tolist()
    parts = []
    for b, (n, N) in enumerate(zip(counts, sc_counts)):
        # block[J, beta, i, alpha] = d^2 E / d r_J,beta d r_i,alpha: the first 3 n columns are the home atoms'
        phi = blocks[ptr[b]:ptr[b] + 9 * N * N].view(N, 3, N, 3)[:, :, :n, :].permute(2, 3, 0, 1).contiguous()
        parts.append((acoustic_sum_rule(phi) if asr else phi).reshape(-1))
    fc_t = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32, device=dev)
    return fc_t, sc_counts


def _checked_crystals(model, z, pos, cell, batch, supercell, check_bound):
    """The checks phonons() makes before any device work, shared with newtonnet_amd/elastic.py: (cells fp64 numpy [B,3,3],
    supercells int [B,3], atoms per primitive cell).  check_bound(counts) (may be None) sits where phonons() refuses a primitive
    cell above max_dim()."""
    _validate_model(model)
    n_atoms, B = pos.shape[0], cell.shape[0]
    if tuple(pos.shape) != (n_atoms, 3) or tuple(cell.shape) != (B, 3, 3) or batch.numel() != n_atoms or z.numel() != n_atoms:
        raise ValueError('z [N], pos [N,3], cell [B,3,3] and batch [N] expected')
    cells = _cells(cell)
    for b in range(B):
        if np.abs(cells[b] - cells[b].T).max() > 1e-5 * np.abs(cells[b]).max():
            raise ValueError(f'crystal {b}: the cell is not a symmetric matrix.  The model shifts a pair to its minimum image by '
                             f'cell @ round(frac), as the reference writes it, which is a lattice vector only when cell = cell^T; with '
                             f'another cell the supercell is not periodic in the primitive lattice and has no dispersion.  Rotate '
                             f'the crystal first: phonons.symmetric_cell(pos, cell)')
    S = _supercells(supercell, B)
    counts = _counts(batch, B, n_atoms)
    if check_bound is not None:
        check_bound(counts)
    cutoff = float(model.embedding_layers.edge_embedding.cutoff)
    for b in range(B):
        w = perpendicular_widths(cells[b]) * S[b]
        if (w < 2.0 * cutoff).any():
            raise ValueError(f'crystal {b}: the supercell {S[b].tolist()} has perpendicular widths '
                             f'{", ".join(f"{x:.3f}" for x in w)} A, below 2 x cutoff = {2.0 * cutoff:.3f} A (the neighbour list takes '
                             f'a single minimum image): enlarge the supercell')
    return cells, S, counts


def _supercell_batch(z, pos, cells, S, counts, dev):
    """(z, pos, cell, batch, atoms per supercell): the supercells as one batch on `dev` (host, fp64, rounded once to fp32)"""
    pos_h, z_h = pos.detach().double().cpu().numpy(), z.detach().reshape(-1).cpu().numpy()
    off = np.concatenate([[0], np.cumsum(counts)])
    zs, ps, cs, bs = [], [], [], []
    for b in range(len(counts)):
        zb, pb, cb = build_supercell(z_h[off[b]:off[b + 1]], pos_h[off[b]:off[b + 1]], cells[b], S[b])
        zs.append(zb)
        ps.append(pb)
        cs.append(cb)
        bs.append(np.full(len(zb), b))
    sc_counts = [len(x) for x in zs]
    z_sc = torch.tensor(np.concatenate(zs), dtype=torch.long, device=dev)
    pos_sc = torch.tensor(np.concatenate(ps), dtype=torch.float32, device=dev)
    cell_sc = torch.tensor(np.stack(cs), dtype=torch.float32, device=dev)
    batch_sc = torch.tensor(np.concatenate(bs), dtype=torch.long, device=dev)
    return z_sc, pos_sc, cell_sc, batch_sc, sc_counts
