"""Batched normal-mode analysis on the HIP path: harmonic frequencies, normal modes, imaginary-mode counts and zero-point
energies of a whole batch from its analytic Hessian blocks, without a host round trip per molecule.

The reference stops at the Hessian (HessianOutput, newtonnet/models/output.py:134-152); its users then call LAPACK per molecule
on the host.  Here the packed blocks of newtonnet_amd.hessian.hessian_blocks stay on the device and ONE launch of
nnhip_eig_blocks (csrc/eig.hip: one workgroup per molecule; symmetrise, mass-weight, project translations / rotations, cyclic
Jacobi in LDS, sort) returns every spectrum.  The derived quantities below are elementwise torch ops on the packed device arrays
plus one deterministic segmented sum (hip.segment_sum); nothing is copied to the host beyond the per-molecule atom counts that
hessian_blocks already brings there.

Units: positions in Angstrom, energies in eV, masses in amu, so eigenvalues are in eV / (A^2 amu).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from newtonnet_amd import hessian as _hessian
from newtonnet_amd import hip

# CODATA 2018 (the SI of 2019 fixes e, h and c exactly; the atomic mass constant is measured)
_E_CHARGE = 1.602176634e-19        # J per eV
_AMU = 1.66053906660e-27           # kg
_C_LIGHT = 2.99792458e10           # cm / s
_PLANCK = 6.62607015e-34           # J s
# omega = sqrt(lambda) with lambda in eV / (A^2 amu) = (e / (1e-20 amu)) s^-2; wavenumber = omega / (2 pi c):
#   sqrt(1.602176634e-19 / (1e-20 x 1.66053906660e-27)) = 9.822694e13 rad/s;  / (2 pi x 2.99792458e10 cm/s) = 521.4709 cm^-1
WAVENUMBER_PER_SQRT_EIGENVALUE = math.sqrt(_E_CHARGE / (1e-20 * _AMU)) / (2.0 * math.pi * _C_LIGHT)
# 0.5 hbar omega = 0.5 h c nu~:  h c = 1.239841984e-4 eV cm
EV_PER_WAVENUMBER = _PLANCK * _C_LIGHT / _E_CHARGE

EPS32 = 2.0 ** -24

# Standard atomic weights (IUPAC abridged values, amu).  Only elements whose value is beyond doubt; pass masses= for the rest.
STANDARD_ATOMIC_WEIGHTS = {
    1: 1.008, 2: 4.0026, 3: 6.94, 4: 9.0122, 5: 10.81, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998, 10: 20.180,
    11: 22.990, 12: 24.305, 13: 26.982, 14: 28.085, 15: 30.974, 16: 32.06, 17: 35.45, 35: 79.904, 53: 126.90,
}


def atomic_mass(z: int) -> float:
    """Standard atomic weight of element z (amu); ValueError outside the built-in table."""
    try:
        return STANDARD_ATOMIC_WEIGHTS[int(z)]
    except KeyError:
        raise ValueError(f'no built-in atomic weight for Z = {int(z)}: pass masses= (amu per atom)') from None


def table_masses(z: torch.Tensor) -> torch.Tensor:
    """masses [N] fp32 for atomic numbers z (any device).  ValueError for an element outside the table -- the one scalar the
    check brings to the host."""
    zmax = max(STANDARD_ATOMIC_WEIGHTS)
    table = torch.zeros(zmax + 1, dtype=torch.float32)
    for k, m in STANDARD_ATOMIC_WEIGHTS.items():
        table[k] = m
    table = table.to(z.device)
    zl = z.long().reshape(-1)
    m = table[zl.clamp(0, zmax)]
    bad = (zl < 1) | (zl > zmax) | (m == 0)
    if bool(bad.any()):
        atomic_mass(int(zl[bad][0]))
    return m


def max_dim() -> int:
    """Largest 3 n_b the solver serves (nnhip_eig_max_dim)."""
    return int(hip.lib().nnhip_eig_max_dim())


class NormalModes:
    """Spectra of a batch, packed per molecule (molecule b owns eigenvalues[ptr[b]:ptr[b+1]] and the [3 n_b, n_b, 3] rows of
    modes at blk_ptr[b]).

    eigenvalues        fp32 [3N]  eV / (A^2 amu), ascending per molecule
    frequencies        fp32 [3N]  cm^-1 = sign(lambda) sqrt(|lambda|) x 521.4709; negative = imaginary
    modes              fp32 [sum 9 n_b^2] or None: ROW k = mode k in mass-weighted coordinates, unit norm, largest component positive
    ptr, blk_ptr       int64 [B+1], [B]
    n_projected        int32 [B]  translation / rotation vectors projected out (6, 5, 3 or 0)
    sweeps, status     int32 [B]  Jacobi sweeps used; status bit 0 = the sweep cap was hit (always for a block
                                  that holds a NaN or an Inf), bit 2 = a mass of the molecule is not
                                  positive and finite (the molecule is not computed: its outputs are zero)
    n_imaginary        int64 [B]  eigenvalues below -tol_zero max_k |lambda_k|
    zero_point_energy  fp32 [B]   eV: sum of hbar omega / 2 over the modes with lambda > tol_zero max_k |lambda_k|
    masses             fp32 [N] or None (unit masses)
    """

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def molecule(self, b: int):
        """(frequencies [3 n_b], modes [3 n_b, n_b, 3] or None) of molecule b: views, no copy."""
        n = self._counts[b]
        o = 3 * self._offsets[b]
        f = self.frequencies[o:o + 3 * n]
        if self.modes is None:
            return f, None
        q = self._blk_offsets[b]
        return f, self.modes[q:q + 9 * n * n].view(3 * n, n, 3)

    def cartesian(self, b: int):
        """Modes of molecule b as Cartesian displacements [3 n_b, n_b, 3]: mode / sqrt(m) per atom (not renormalised)."""
        _, m = self.molecule(b)
        if m is None:
            raise ValueError('this result holds no modes (modes=False)')
        if self.masses is None:
            return m.clone()
        o, n = self._offsets[b], self._counts[b]
        return m / self.masses[o:o + n].sqrt()[None, :, None]


def eig_blocks(blocks: torch.Tensor, blk_ptr: torch.Tensor, batch: torch.Tensor, pos: torch.Tensor, cell: torch.Tensor,
               masses: Optional[torch.Tensor] = None, project: bool = True, modes: bool = True,
               tol_zero: Optional[float] = None, counts: Optional[torch.Tensor] = None) -> NormalModes:
    """The solver alone on packed blocks the caller already has (layout of hessian_blocks; atoms of a molecule contiguous and
    molecules ascending in `batch`: not checked, a check would cost a copy to the host).  masses: fp32 [N] in amu, None = unit
    masses (plain eigenvalues of the symmetrised block); a molecule with a mass that is not positive and finite is not computed
    and says so in `status` (bit 2), checked on the device.
    counts: atoms per molecule as a CPU tensor if the caller has them (else one bincount is copied to the host).
    modes=False skips the eigenvectors; the eigenvalues are bitwise the same either way (the rotations of the matrix do not depend
    on the accumulated vectors)."""
    dev = blocks.device
    if not blocks.is_cuda:
        raise RuntimeError('newtonnet_amd normal modes run on an MI355X (ROCm) device only: move the inputs to "cuda"')
    n_mol = cell.shape[0]
    n_atoms = pos.shape[0]
    if blocks.dtype != torch.float32 or not blocks.is_contiguous() or blocks.dim() != 1:
        raise ValueError('blocks: contiguous 1-d float32 expected')
    if blk_ptr.dtype != torch.int64 or blk_ptr.shape != (n_mol,) or not blk_ptr.is_contiguous():
        raise ValueError('blk_ptr: contiguous int64 [B] expected')
    if tuple(pos.shape) != (n_atoms, 3) or tuple(cell.shape) != (n_mol, 3, 3) or batch.numel() != n_atoms:
        raise ValueError('pos [N,3], cell [B,3,3] and batch [N] expected')
    for name, t in (('blk_ptr', blk_ptr), ('batch', batch), ('pos', pos), ('cell', cell), ('masses', masses)):
        if t is not None and t.device != dev:
            raise ValueError(f'{name} is on {t.device}, blocks on {dev}')
    pos_c, cell_c = hip._f32c(pos.detach(), 'pos'), hip._f32c(cell.detach(), 'cell')
    m_c = None
    if masses is not None:
        if masses.numel() != n_atoms:
            raise ValueError(f'masses: {masses.numel()} values for {n_atoms} atoms')
        m_c = hip._f32c(masses.detach().reshape(-1), 'masses')
    if counts is None:
        counts = torch.bincount(batch.long().reshape(-1), minlength=n_mol).cpu() if n_atoms else torch.zeros(n_mol, dtype=torch.long)
    counts = counts.long().cpu()
    cl = counts.tolist()
    if len(cl) != n_mol or sum(cl) != n_atoms or blocks.numel() != sum(9 * n * n for n in cl):
        raise ValueError('blocks / batch / cell disagree about the molecules')
    bound = max_dim()
    for b, n in enumerate(cl):
        if 3 * n > bound:
            raise NotImplementedError(f'molecule {b} has 3 x {n} = {3 * n} coordinates, above the {bound} the batched eigensolver '
                                      f'serves (nnhip_eig_max_dim)')
    mol_host = torch.zeros(n_mol + 1, dtype=torch.int32)
    mol_host[1:] = torch.cumsum(counts, 0).to(torch.int32)
    mol_dev = mol_host.to(dev)
    ptr = 3 * mol_dev.long()
    blk_off = [0] * n_mol
    for b in range(1, n_mol):
        blk_off[b] = blk_off[b - 1] + 9 * cl[b - 1] * cl[b - 1]
    evals = torch.zeros(3 * n_atoms, dtype=torch.float32, device=dev)
    vecs = torch.zeros(blocks.numel(), dtype=torch.float32, device=dev) if modes else None
    n_proj, sweeps, status = (torch.zeros(n_mol, dtype=torch.int32, device=dev) for _ in range(3))
    if n_mol and n_atoms:
        rc = hip.lib().nnhip_eig_blocks(hip._ptr(blocks), hip._ptr(blk_ptr), hip._ptr(mol_dev), mol_host.data_ptr(), n_mol,
                                        hip._ptr(pos_c), hip._ptr(cell_c), hip._ptr(m_c), 1 if project else 0, hip._ptr(evals),
                                        hip._ptr(vecs), hip._ptr(n_proj), hip._ptr(sweeps), hip._ptr(status), hip._stream(dev))
        if rc == 2:
            raise NotImplementedError(hip.lib().nnhip_last_error().decode())
        hip._check(rc, 'nnhip_eig_blocks')
    # ---- derived quantities: elementwise on the packed arrays + one segmented sum ----
    counts_dev = (mol_dev[1:] - mol_dev[:-1]).long()
    freq = torch.sign(evals) * evals.abs().sqrt() * WAVENUMBER_PER_SQRT_EIGENVALUE
    if n_atoms:
        last = 3 * n_atoms - 1
        lo, hi = ptr[:-1].clamp(max=last), (ptr[1:] - 1).clamp(min=0)
        scale = torch.maximum(evals[lo].abs(), evals[hi].abs()) * (counts_dev > 0)   # sorted: the extremes are at the ends
        tol = (8.0 * EPS32) * (3 * counts_dev).float() if tol_zero is None else torch.full_like(scale, float(tol_zero))
        thr = (tol * scale)[batch.long().reshape(-1)].repeat_interleave(3)
        imag, real = evals < -thr, evals > thr
        x = torch.stack([imag.float(), (0.5 * EV_PER_WAVENUMBER) * freq * real], dim=1).contiguous()
        s = hip.segment_sum(x, ptr.to(torch.int32), n_mol)
        n_imag, zpe = s[:, 0].round().long(), s[:, 1].contiguous()
    else:
        n_imag = torch.zeros(n_mol, dtype=torch.long, device=dev)
        zpe = torch.zeros(n_mol, dtype=torch.float32, device=dev)
    return NormalModes(eigenvalues=evals, frequencies=freq, modes=vecs, ptr=ptr, blk_ptr=blk_ptr, n_projected=n_proj, sweeps=sweeps,
                       status=status, n_imaginary=n_imag, zero_point_energy=zpe, masses=m_c, _counts=cl,
                       _offsets=mol_host[:-1].tolist(), _blk_offsets=blk_off)


def normal_modes(model, z, pos, cell, batch, masses: Optional[torch.Tensor] = None, project: bool = True, modes: bool = True,
                 tol_zero: Optional[float] = None) -> NormalModes:
    """Harmonic analysis of every molecule of the batch at the current parameters: Hessian blocks (hessian.hessian_blocks) and
    the batched solver, on the caller's current stream.  masses=None: standard atomic weights of z (ValueError for an element
    outside the built-in table).  project: remove translations and rotations (translations only for periodic molecules).
    tol_zero: relative threshold below which an eigenvalue counts as zero (default 8 x 3 n_b x 2^-24, the solver's error bound,
    so projected modes are never counted as imaginary or real)."""
    _hessian._validate(model, pos)
    m = table_masses(z) if masses is None else masses
    blocks, blk_ptr, counts = _hessian.hessian_blocks_counts(model, z, pos, cell, batch)
    return eig_blocks(blocks, blk_ptr, batch, pos, cell, m, project=project, modes=modes, tol_zero=tol_zero, counts=counts)
