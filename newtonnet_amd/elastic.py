"""Analytic second-order elastic constants of crystals on the HIP path.

Definition.  C_IJ = (1 / V) d^2 E / d e_I d e_J at the geometry given, under the homogeneous deformation x -> (1 + eps) x of the
positions and the cell, eps = [[e1, e6/2, e5/2], [e6/2, e2, e4/2], [e5/2, e4/2, e3]] (Voigt order xx, yy, zz, yz, xz, xy with
engineering shears), in eV / A^3.  Away from zero stress this second derivative of the energy differs from the stress-strain
(Birch) coefficients by terms in the stress; at zero stress they agree.

Clamped-ion (Born) part.  One tangent-over-reverse pass of the Hessian kernels seeded with a strain (hessian.strain_vector_product,
nnhip_strain_vp, csrc/elastic.hip) gives, for the strain of unit Voigt component J, the column d^2E/de_I de_J and the internal-
strain coupling Lambda[(i a), J] = d^2 E / d r_ia d e_J.  The six strains ride on R = min(6, REPLICA_ATOM_BUDGET // N) replicas of
the batch (the replica scheme of hessian._Pass: every replica carries its own strain), so 6 N <= the budget means ONE pass.

Relaxed-ion part.  With the atoms free to follow the strain, and ZERO FORCES at the geometry given,
    C = C_born - (1 / V) Lambda^T pinv(Phi0) Lambda,
Phi0 = the force constants at Gamma (nnhip_elastic_fold over the Phonons' force constants), its pseudo-inverse over the modes the
device eigensolver (vibrations.eig_blocks: unit masses, no projection) puts above the zero threshold: nnhip_elastic_relax.  The
three acoustic modes are the null space; a negative mode is reported (status bit 1) and enters the sum as the formula says.

Supercells.  The model's neighbour list takes a single minimum image, so -- exactly as phonons.phonons -- the strain pass runs on a
supercell whose perpendicular widths are at least twice the cutoff, a cell that is not orthogonal must be a symmetric matrix, and
the sums are divided by the supercell's volume.  Lambda is read at the home atoms.

Size.  The relaxed term serves primitive cells of up to max_dim() = 96 coordinates by default (solver='lds': the bound of the
one-workgroup phonon kernel) and, with solver='auto' / 'blocked', of up to max_dim_large() = 768 (256 atoms): the keyword is
handed to vibrations.eig_blocks and to the Phonons the call computes; nnhip_elastic_fold and nnhip_elastic_relax have no limit.

Left out: finite-strain and third-order constants, Birch coefficients, piezoelectric terms, symmetry reduction of the six
strains.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from newtonnet_amd import hessian as _hessian
from newtonnet_amd import hip
from newtonnet_amd import phonons as _ph
from newtonnet_amd import vibrations as _v

GPA_PER_EV_A3 = 160.21766          # 1 eV / A^3 in GPa
STATUS_ZERO = hip.abi.CONSTANTS['NNHIP_ELASTIC_STATUS_ZERO']           # not exactly three modes under the zero threshold
STATUS_NEGATIVE = hip.abi.CONSTANTS['NNHIP_ELASTIC_STATUS_NEGATIVE']   # a negative mode: the geometry is no minimum
STATUS_SOLVER = 4                                                      # the eigensolver flagged Phi0 (its own status is non-zero)
VOIGT_PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def max_dim() -> int:
    """Largest 3 n_b of a primitive cell the relaxed-ion term serves (that of the Phonons whose force constants it folds)."""
    return _ph.max_dim()


def max_dim_large() -> int:
    """Largest 3 n_b the relaxed-ion term serves with solver='auto' / 'blocked': the smaller of the bounds of the two blocked
    solvers (phonons.max_dim_large(), vibrations.max_dim_large())."""
    return min(_ph.max_dim_large(), _v.max_dim_large())


def voigt_matrices(e) -> np.ndarray:
    """fp64 [..., 3, 3]: eps of Voigt components e [..., 6] (engineering shears)."""
    e = np.asarray(e, dtype=np.float64)
    out = np.zeros(e.shape[:-1] + (3, 3))
    for k, (a, b) in enumerate(VOIGT_PAIRS):
        out[..., a, b] = out[..., b, a] = e[..., k] if a == b else 0.5 * e[..., k]
    return out


def _check_bound(counts, solver: str = 'lds'):
    if solver != 'lds':
        bound = max_dim_large()
        for b, n in enumerate(counts):
            if 3 * n > bound:
                raise NotImplementedError(f'crystal {b} has 3 x {n} = {3 * n} coordinates per primitive cell, above the {bound} of '
                                          f'elastic.max_dim_large() that the relaxed-ion term serves: relaxed=False has no size limit')
        return
    bound = max_dim()
    for b, n in enumerate(counts):
        if 3 * n > bound:
            raise NotImplementedError(f'crystal {b} has 3 x {n} = {3 * n} coordinates per primitive cell, above the {bound} of '
                                      f'elastic.max_dim() that the relaxed-ion term serves: relaxed=False has no size limit')


class ElasticConstants:
    """Elastic constants of B crystals (all tensors on the device unless said otherwise, eV / A^3).

    born             fp32 [B,6,6]  clamped-ion constants, symmetrised
    relaxation       fp32 [B,6,6]  Lambda^T pinv(Phi0) Lambda / V (zeros with relaxed=False)
    C                fp32 [B,6,6]  born - relaxation (exactly symmetric)
    asymmetry        fp32 [B]      max |C_IJ - C_JI| before the symmetrisation
    internal_strain  fp32 [3 n, 6] Lambda[(i a), J] = d^2 E / d r_ia d e_J of the home atoms (eV / A), packed crystal by crystal
    volume           fp64 [B] (CPU) volume of the primitive cell, A^3
    status           int32 [B]     bit 0: not exactly three zero modes; bit 1: a negative mode (the geometry is not a minimum: the
                                   relaxed constants are the formula's value, not a physical modulus); bit 2: the eigensolver
                                   flagged Phi0.  Zero with relaxed=False
    n_zero, n_negative  int32 [B]
    counts           atoms per primitive cell (list)
    """

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def _c64(self) -> torch.Tensor:
        return self.C.detach().double().cpu()

    def gpa(self) -> torch.Tensor:
        """C in GPa (fp64, CPU)."""
        return self._c64() * GPA_PER_EV_A3

    def compliance(self) -> torch.Tensor:
        """S = C^-1 per crystal (fp64, CPU), A^3 / eV."""
        return torch.linalg.inv(self._c64())

    def bulk_modulus(self):
        """(Voigt, Reuss, Hill) bulk moduli, fp64 [B] each, eV / A^3."""
        c, s = self._c64(), self.compliance()
        kv = (c[:, 0, 0] + c[:, 1, 1] + c[:, 2, 2] + 2.0 * (c[:, 0, 1] + c[:, 0, 2] + c[:, 1, 2])) / 9.0
        kr = 1.0 / (s[:, 0, 0] + s[:, 1, 1] + s[:, 2, 2] + 2.0 * (s[:, 0, 1] + s[:, 0, 2] + s[:, 1, 2]))
        return kv, kr, 0.5 * (kv + kr)

    def shear_modulus(self):
        """(Voigt, Reuss, Hill) shear moduli, fp64 [B] each, eV / A^3."""
        c, s = self._c64(), self.compliance()
        gv = (c[:, 0, 0] + c[:, 1, 1] + c[:, 2, 2] - (c[:, 0, 1] + c[:, 0, 2] + c[:, 1, 2])
              + 3.0 * (c[:, 3, 3] + c[:, 4, 4] + c[:, 5, 5])) / 15.0
        gr = 15.0 / (4.0 * (s[:, 0, 0] + s[:, 1, 1] + s[:, 2, 2]) - 4.0 * (s[:, 0, 1] + s[:, 0, 2] + s[:, 1, 2])
                     + 3.0 * (s[:, 3, 3] + s[:, 4, 4] + s[:, 5, 5]))
        return gv, gr, 0.5 * (gv + gr)

    def youngs_modulus(self) -> torch.Tensor:
        """E = 9 K G / (3 K + G) of the Hill averages, fp64 [B], eV / A^3."""
        k, g = self.bulk_modulus()[2], self.shear_modulus()[2]
        return 9.0 * k * g / (3.0 * k + g)

    def poisson_ratio(self) -> torch.Tensor:
        """nu = (3 K - 2 G) / (2 (3 K + G)) of the Hill averages, fp64 [B]."""
        k, g = self.bulk_modulus()[2], self.shear_modulus()[2]
        return (3.0 * k - 2.0 * g) / (2.0 * (3.0 * k + g))

    def stability(self) -> torch.Tensor:
        """Smallest eigenvalue of C per crystal (fp64 [B], eV / A^3): positive = mechanically stable (Born criterion)."""
        return torch.linalg.eigvalsh(self._c64())[:, 0]


def born_pass(model, z, pos, cell, batch, replicas: Optional[int] = None):
    """The six unit Voigt strains on one batch: (d2 fp32 [B,6,6] with d2[b, I, J] = d^2 E_b / de_I de_J as the pass for strain J
    returns it (not symmetrised, not divided by a volume), dgrad fp32 [N,3,6] = d^2 E / d pos d e_J).  replicas: R strains per
    pass (None: min(6, REPLICA_ATOM_BUDGET // N))."""
    n, B, dev = pos.shape[0], cell.shape[0], pos.device
    R = _hessian.replicas_for(n, 6) if replicas is None else max(1, min(int(replicas), 6))
    d2 = torch.zeros(B, 6, 6, dtype=torch.float32, device=dev)
    dgrad = torch.zeros(n, 3, 6, dtype=torch.float32, device=dev)
    if n == 0 or B == 0:
        return d2, dgrad
    p = _hessian._Pass(model, z, pos, cell, batch, R, None)
    out_g = torch.empty(R * n, 3, dtype=torch.float32, device=dev)
    out_2 = torch.empty(R * B, 6, dtype=torch.float32, device=dev)
    for k in range(-(-6 // R)):
        eta = torch.zeros(R, B, 6, dtype=torch.float32)
        live = [r for r in range(R) if k * R + r < 6]
        for r in live:
            eta[r, :, k * R + r] = 1.0
        _hessian._strain_pass(p, eta.reshape(R * B, 6).to(dev), out_g, out_2)
        for r in live:
            d2[:, :, k * R + r] = out_2[r * B:(r + 1) * B]
            dgrad[:, :, k * R + r] = out_g[r * n:(r + 1) * n]
    return d2, dgrad


def fold_force_constants(ph) -> torch.Tensor:
    """Phi0 of every crystal of a Phonons, packed [n_b,3,n_b,3] at ph.out_ptr[b] (nnhip_elastic_fold)."""
    if not ph.fc.is_cuda:
        raise RuntimeError('newtonnet_amd elastic constants run on an MI355X (ROCm) device only: build the Phonons on "cuda"')
    for b, (n, N) in enumerate(zip(ph.counts, ph.sc_counts)):
        if n and N % n:
            raise ValueError(f'crystal {b}: {N} supercell atoms are no multiple of its {n} atoms')
    phi0 = torch.zeros(sum(9 * n * n for n in ph.counts), dtype=torch.float32, device=ph.fc.device)
    # The library wants a status array (NNHIP_ELASTIC_STATUS_SIZE per crystal whose sc_atoms is no multiple of its atoms).  It is
    # not read back: ph.sc_atoms and ph.cry_ptr are the device copies of the very counts the loop above has just checked, so the
    # bit cannot be set here, and reading it would cost a device-to-host wait per call.  The bit is a C caller's; the stage test
    # (tests/test_hip_crystal_stages.py) produces it through the library directly.
    status = torch.zeros(len(ph.counts), dtype=torch.int32, device=ph.fc.device)
    hip._check(hip.lib().nnhip_elastic_fold(hip._ptr(ph.fc), hip._ptr(ph.fc_ptr), hip._ptr(ph.cry_ptr), hip._ptr(ph.sc_atoms),
                                            hip._ptr(ph.out_ptr), len(ph.counts), hip._ptr(phi0), hip._ptr(status),
                                            hip._stream(phi0.device)), 'nnhip_elastic_fold')
    return phi0


def relaxation_term(phi0: torch.Tensor, blk_ptr: torch.Tensor, counts, lam: torch.Tensor, tol_zero: Optional[float] = None,
                    solver: str = 'lds'):
    """(R fp32 [B,6,6], n_zero, n_negative, status int32 [B]) with R = Lambda^T pinv(Phi0) Lambda: phi0 packed [n_b,3,n_b,3] blocks at
    blk_ptr (int64 [B]), counts the atoms per crystal (list), lam fp32 [3 n, 6].  The eigenpairs come from vibrations.eig_blocks
    (unit masses, no projection); a mode counts as zero when |lambda| <= vibrations.zero_threshold (tol_zero overrides its
    relative tolerance).  solver: 'lds' (default: up to max_dim() coordinates), 'auto' or 'blocked' (up to max_dim_large()), handed
    to vibrations.eig_blocks."""
    _ph._check_solver(solver)
    dev, B, n = phi0.device, len(counts), sum(counts)
    if tuple(lam.shape) != (3 * n, 6) or lam.dtype != torch.float32:
        raise ValueError(f'Lambda: float32 [{3 * n}, 6] expected (got {tuple(lam.shape)})')
    bound = max_dim() if solver == 'lds' else max_dim_large()
    for b, k in enumerate(counts):
        if 3 * k > bound:
            raise NotImplementedError(f'crystal {b} has 3 x {k} = {3 * k} coordinates, above the {bound} of elastic.'
                                      f'{"max_dim()" if solver == "lds" else "max_dim_large()"}')
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(counts, dtype=torch.long)).to(dev)
    nm = _v.eig_blocks(phi0, blk_ptr, batch, torch.zeros(n, 3, device=dev), torch.zeros(B, 3, 3, device=dev), None, project=False,
                       modes=True, tol_zero=tol_zero, counts=torch.tensor(counts, dtype=torch.long), solver=solver)
    cry = torch.zeros(B + 1, dtype=torch.int32)
    cry[1:] = torch.cumsum(torch.tensor(counts, dtype=torch.int32), 0)
    cry = cry.to(dev)
    out = torch.zeros(B, 6, 6, dtype=torch.float32, device=dev)
    n_zero, n_neg, status = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    lam_c = lam.contiguous()
    thr = nm.threshold.float().contiguous()
    hip._check(hip.lib().nnhip_elastic_relax(hip._ptr(nm.eigenvalues), hip._ptr(nm.modes), hip._ptr(blk_ptr), hip._ptr(cry),
                                             hip._ptr(lam_c), hip._ptr(thr), B, hip._ptr(out), hip._ptr(n_zero), hip._ptr(n_neg),
                                             hip._ptr(status), hip._stream(dev)), 'nnhip_elastic_relax')
    status = status | (nm.status != 0).to(torch.int32) * STATUS_SOLVER
    return out, n_zero, n_neg, status


def elastic_constants(model, z, pos, cell, batch, supercell=(1, 1, 1), relaxed: bool = True, phonons=None,
                      tol_zero: Optional[float] = None, replicas: Optional[int] = None, solver: str = 'lds') -> ElasticConstants:
    """Elastic constants of every crystal of the batch (z, pos, cell, batch: the primitive cells) at the current parameters; see
    the module text.  supercell: three integers or an integer [B,3], checked as phonons.phonons checks it.  relaxed=True adds
    the relaxed-ion term from `phonons` (a Phonons of the same crystals on the same supercell) or, when None, from
    model.phonons(..., asr=True); it needs zero forces to mean anything and serves primitive cells of up to max_dim()
    coordinates (NotImplementedError above).  relaxed=False: the clamped-ion constants, no size limit.  tol_zero: relative zero
    threshold of the modes of Phi0 (None: vibrations.zero_threshold's).  replicas: strains per pass (None: as many of the six as
    REPLICA_ATOM_BUDGET allows).  solver: 'lds' (default), 'auto' or 'blocked': with the latter two the relaxed term serves
    primitive cells of up to max_dim_large() coordinates (see the module text)."""
    _ph._check_solver(solver)
    cells, S, counts = _ph._checked_crystals(model, z, pos, cell, batch, supercell,
                                             (lambda c: _check_bound(c, solver)) if relaxed else None)
    B = len(counts)
    if phonons is not None and relaxed:
        if list(phonons.counts) != list(counts) or not np.array_equal(np.asarray(phonons.supercell), S):
            raise ValueError('phonons: built for other crystals or another supercell than this call')
    if not pos.is_cuda:
        raise RuntimeError('newtonnet_amd elastic constants run on an MI355X (ROCm) device only: move the model and the inputs to '
                           '"cuda"')
    dev = pos.device
    z_sc, pos_sc, cell_sc, batch_sc, sc_counts = _ph._supercell_batch(z, pos, cells, S, counts, dev)
    with torch.no_grad():
        d2, dgrad = born_pass(model, z_sc, pos_sc, cell_sc, batch_sc, replicas)
    vol = np.abs(np.linalg.det(cells))
    vol_sc = torch.tensor(vol * np.prod(S, axis=1), dtype=torch.float64, device=dev)
    raw = (d2.double() / vol_sc[:, None, None]).float()
    born = 0.5 * (raw + raw.transpose(1, 2))
    asym = (raw - raw.transpose(1, 2)).abs().amax(dim=(1, 2))
    sc_off = np.concatenate([[0], np.cumsum(sc_counts)])
    home = torch.tensor(np.concatenate([np.arange(sc_off[b], sc_off[b] + n) for b, n in enumerate(counts)]), dtype=torch.long, device=dev)
    lam = dgrad[home].reshape(-1, 6).contiguous()
    relaxation = torch.zeros_like(born)
    n_zero, n_neg, status = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    if relaxed:
        ph = phonons if phonons is not None else model.phonons(z, pos, cell, batch, supercell, asr=True, solver=solver)
        r, n_zero, n_neg, status = relaxation_term(fold_force_constants(ph), ph.out_ptr, counts, lam, tol_zero, solver)
        relaxation = (r.double() / torch.tensor(vol, dtype=torch.float64, device=dev)[:, None, None]).float()
    return ElasticConstants(born=born, relaxation=relaxation, C=born - relaxation, asymmetry=asym, internal_strain=lam,
                            volume=torch.tensor(vol, dtype=torch.float64), status=status, n_zero=n_zero, n_negative=n_neg,
                            counts=list(counts), supercell=S)
