"""Batched normal-mode analysis on the HIP path: harmonic frequencies, normal modes, imaginary-mode counts and zero-point
energies of a whole batch from its analytic Hessian blocks, without a host round trip per molecule.

The reference stops at the Hessian (HessianOutput, newtonnet/models/output.py:134-152); its users then call LAPACK per molecule
on the host.  Here the packed blocks of newtonnet_amd.hessian.hessian_blocks stay on the device and ONE launch of
nnhip_eig_blocks (csrc/eig.hip: one workgroup per molecule; symmetrise, mass-weight, project translations / rotations, cyclic
Jacobi in LDS, sort) returns every spectrum of up to 126 coordinates; solver='auto' sends larger molecules (up to 1536) through
the blocked solver nnhip_eig_blocks_large (csrc/eig_large.hip), which keeps the matrix in a workspace in HBM.  The derived quantities below are elementwise torch ops on the packed device arrays
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
# Boltzmann constant in eV / K: 1.380649e-23 J/K / 1.602176634e-19 J/eV = 8.617333262e-5 (both exact in the SI of 2019)
K_BOLTZMANN = 8.617333262e-5
# hbar omega (eV) of a mode with eigenvalue 1 eV / (A^2 amu): eps = EV_PER_SQRT_EIGENVALUE sqrt(lambda) = 0.064654 eV
EV_PER_SQRT_EIGENVALUE = EV_PER_WAVENUMBER * WAVENUMBER_PER_SQRT_EIGENVALUE

EPS32 = 2.0 ** -24
EIG_PROJECT = hip.abi.CONSTANTS['NNHIP_EIG_PROJECT']      # flag of nnhip_eig_blocks / nnhip_eig_blocks_large

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


def lowest_mode_direction(model, z, pos, cell, batch, masses: torch.Tensor, solver: str):
    """(u fp64 [N,3], n_imaginary [B]): every molecule's lowest normal mode as a Cartesian direction -- its mass-weighted
    eigenvector divided by sqrt(m), not normalised -- and the molecule's count of imaginary modes.  The start direction of a
    SaddleSearch or a ReactionPath that was given none."""
    from newtonnet_amd.dynamics import _mol_ptr          # (dynamics imports this module)
    B, dev = cell.shape[0], pos.device
    nm = model.normal_modes(z, pos.detach(), cell, batch, masses=masses, solver=solver)
    ptr = _mol_ptr(batch, B).long()
    local = torch.arange(pos.shape[0], device=dev) - ptr[batch.long()]
    q = nm.modes[(nm.blk_ptr[batch.long()] + 3 * local)[:, None] + torch.arange(3, device=dev)]
    return q.double() / masses.double().sqrt()[:, None], nm.n_imaginary


def max_dim() -> int:
    """Largest 3 n_b the one-workgroup solver serves (nnhip_eig_max_dim): the bound of solver='lds' and of
    NormalModes.sample(kernel='lds')."""
    return int(hip.lib().nnhip_eig_max_dim())


def max_dim_large() -> int:
    """Largest 3 n_b the blocked solver serves (nnhip_eig_large_max_dim; solver='auto' / 'blocked').  Bounded by the range its
    accuracy has been verified in and by the one-workgroup-per-molecule kernels around its sweeps (csrc/eig_large.hip)."""
    return int(hip.lib().nnhip_eig_large_max_dim())


def max_dim_sample_large() -> int:
    """Largest 3 n_b the tiled sampling kernel serves (nnhip_mode_sample_large_max_dim; NormalModes.sample with kernel='auto' /
    'tiled'): the bound of the blocked solver, max_dim_large()."""
    return int(hip.lib().nnhip_mode_sample_large_max_dim())


SOLVERS = ('lds', 'auto', 'blocked')
SAMPLE_KERNELS = ('lds', 'auto', 'tiled')
KERNEL_OF_SOLVER = {'lds': 'lds', 'auto': 'auto', 'blocked': 'tiled'}   # the sampling kernel that serves what the solver produced


def _check_solver(solver) -> str:
    if solver not in SOLVERS:
        raise ValueError(f"solver: one of 'lds', 'auto', 'blocked' expected (got {solver!r})")
    return solver


def _check_kernel(kernel) -> str:
    if kernel not in SAMPLE_KERNELS:
        raise ValueError(f"kernel: one of 'lds', 'auto', 'tiled' expected (got {kernel!r})")
    return kernel


_STORED = object()   # sample(): "the value stored on the NormalModes"


def _temperature(temperature) -> float:
    T = float(temperature)
    if not (T >= 0.0 and math.isfinite(T)):
        raise ValueError(f'temperature: a finite value >= 0 K expected (got {temperature!r})')
    return T


def zero_threshold(evals: torch.Tensor, ptr: torch.Tensor, counts_dev: torch.Tensor, tol_zero: Optional[float]) -> torch.Tensor:
    """threshold [B] below which an eigenvalue counts as zero: tol_zero max_k |lambda_k| per molecule (default tol_zero: 8 x 3 n_b x
    2^-24, the solver's error bound).  The one rule behind n_imaginary, zero_point_energy, sample and thermochemistry."""
    last = evals.numel() - 1
    lo, hi = ptr[:-1].clamp(max=last), (ptr[1:] - 1).clamp(min=0)
    scale = torch.maximum(evals[lo].abs(), evals[hi].abs()) * (counts_dev > 0)   # sorted: the extremes are at the ends
    tol = (8.0 * EPS32) * (3 * counts_dev).float() if tol_zero is None else torch.full_like(scale, float(tol_zero))
    return tol * scale


class ModeSamples:
    """Displaced geometries of NormalModes.sample, ready for model(z, pos, cell, batch): molecule b S + s is sample s of molecule b.

    z                    int64 [S N] or None (the NormalModes held no z)
    pos                  fp32 [S N, 3]
    cell                 fp32 [B S, 3, 3]
    batch                int64 [S N]
    harmonic_energy      fp32 [B S]    eV: 1/2 sum_k lambda_k q_k^2 over the live modes
    n_skipped_imaginary  int64 [B]     imaginary modes (lambda < -threshold) left undisplaced
    amplitudes           fp32 [3 S N]  q_k per sample in mass-weighted coordinates (A sqrt(amu)), packed like the draws xi
    """

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Thermochemistry:
    """U, F (eV) and S, Cv (eV / K) of NormalModes.thermochemistry: fp32 [B] each, at `temperature` (K)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class NormalModes:
    """Spectra of a batch, packed per molecule (molecule b owns eigenvalues[ptr[b]:ptr[b+1]] and the [3 n_b, n_b, 3] rows of
    modes at blk_ptr[b]).

    eigenvalues        fp32 [3N]  eV / (A^2 amu), ascending per molecule
    frequencies        fp32 [3N]  cm^-1 = sign(lambda) sqrt(|lambda|) x 521.4709; negative = imaginary
    modes              fp32 [sum 9 n_b^2] or None: ROW k = mode k in mass-weighted coordinates, unit norm, largest component positive
    ptr, blk_ptr       int64 [B+1], [B]
    n_projected        int32 [B]  translation / rotation vectors projected out (6, 5, 3 or 0)
    sweeps, status     int32 [B]  Jacobi sweeps used (a molecule solved by the blocked solver -- solver='auto' above max_dim(),
                                  solver='blocked' -- counts its OUTER sweeps over the block pairs); status bit 0 = the
                                  sweep cap was hit (always for a block that holds a NaN or an Inf), bit 2 = a mass of
                                  the molecule is not positive and finite (the molecule is not computed: its outputs are zero)
    n_imaginary        int64 [B]  eigenvalues below -tol_zero max_k |lambda_k|
    zero_point_energy  fp32 [B]   eV: sum of hbar omega / 2 over the modes with lambda > tol_zero max_k |lambda_k|
    masses             fp32 [N] or None (unit masses)
    threshold          fp32 [B]   tol_zero max_k |lambda_k|: a mode is LIVE iff lambda > threshold, imaginary iff lambda < -threshold
    pos, cell, z       the geometry the spectra belong to (z: None when eig_blocks was not given one): what sample() displaces
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

    def _live(self):
        """(live [3N] bool, imaginary [3N] bool): the one rule n_imaginary, zero_point_energy, sample and thermochemistry share"""
        thr = self.threshold.repeat_interleave(self.ptr[1:] - self.ptr[:-1], output_size=self.eigenvalues.numel())
        return self.eigenvalues > thr, self.eigenvalues < -thr

    def sample(self, n_samples: int, temperature: float, quantum: bool = False, generator: Optional[torch.Generator] = None,
               xi: Optional[torch.Tensor] = None, pos=_STORED, z=_STORED, cell=_STORED, kernel: str = 'lds') -> 'ModeSamples':
        """n_samples displaced geometries per molecule drawn from its harmonic distribution at `temperature` (K), in one launch
        (nnhip_mode_sample, csrc/sample.hip).  quantum=False: classical normal-mode sampling, amplitude variance k_B T / lambda per
        live mode; quantum=True: Wigner sampling, (eps / 2 lambda) coth(eps / 2 k_B T) with eps = hbar omega (T = 0: the ground
        state).  Modes that are not live (projected, zero, imaginary: lambda <= threshold) are not displaced; the imaginary ones
        skipped are counted in n_skipped_imaginary.
        xi: the standard-normal draws, fp32 on the device, S x [3 n_b] values per molecule packed at 3 S x (atom offset),
        sample-major; None draws them with torch.randn and `generator` (a generator of the device).  pos / z / cell: other values
        than the stored ones (same shapes).  The result is ready for model(z, pos, cell, batch): the samples of molecule b are the
        molecules b S .. b S + S - 1, each with that molecule's cell.
        kernel: 'lds' (default) -- nnhip_mode_sample stages a molecule's mode matrix in LDS: a result that holds a molecule above
        max_dim() (126 coordinates; solver='auto' / 'blocked' produce them) raises NotImplementedError; 'tiled' -- every molecule
        goes through nnhip_mode_sample_large (csrc/sample_large.hip: two launches, the mode matrix streamed from HBM),
        NotImplementedError above max_dim_sample_large() (1536 coordinates); 'auto' -- the molecules within max_dim() go through
        nnhip_mode_sample, bitwise as with 'lds', the others through the tiled kernel.  The kernels sum in the same order, so
        'tiled' and 'lds' agree bitwise where both serve."""
        _check_kernel(kernel)
        S = int(n_samples)
        if S < 1 or S != n_samples:
            raise ValueError(f'n_samples: a positive integer expected (got {n_samples!r})')
        T = _temperature(temperature)
        if self.modes is None:
            raise ValueError('this result holds no modes (modes=False)')
        pos = self.pos if pos is _STORED else pos
        z = self.z if z is _STORED else z
        cell = self.cell if cell is _STORED else cell
        n_atoms, n_mol = self.eigenvalues.numel() // 3, len(self._counts)
        dev = self.eigenvalues.device
        if pos is None or tuple(pos.shape) != (n_atoms, 3) or cell is None or tuple(cell.shape) != (n_mol, 3, 3):
            raise ValueError(f'pos [{n_atoms},3] and cell [{n_mol},3,3] expected')
        if z is not None and z.numel() != n_atoms:
            raise ValueError(f'z: {z.numel()} values for {n_atoms} atoms')
        if xi is not None:
            if xi.numel() != 3 * n_atoms * S or xi.dim() != 1:
                raise ValueError(f'xi: 1-d with n_samples x 3 N = {3 * n_atoms * S} values expected (got {tuple(xi.shape)})')
            if xi.device != dev:
                raise ValueError(f'xi is on {xi.device}, the modes on {dev}')
            if xi.dtype != torch.float32:
                raise ValueError(f'xi: float32 expected (got {xi.dtype})')
        for name, t in (('pos', pos), ('cell', cell), ('z', z)):
            if t is not None and t.device != dev:
                raise ValueError(f'{name} is on {t.device}, the modes on {dev}')
        if generator is not None and xi is None and torch.device(generator.device).type != dev.type:
            raise ValueError(f'generator is on {generator.device}, the modes on {dev}')
        if not self.eigenvalues.is_cuda:
            raise RuntimeError('newtonnet_amd normal modes run on an MI355X (ROCm) device only: move the inputs to "cuda"')
        if xi is None:
            xi = torch.randn(3 * n_atoms * S, generator=generator, device=dev, dtype=torch.float32)
        xi = xi.contiguous()
        pos_c = hip._f32c(pos.detach(), 'pos')
        mol_host = torch.tensor(self._offsets + [n_atoms], dtype=torch.int32)
        mol_dev = (self.ptr // 3).to(torch.int32)
        new_pos = torch.empty(n_atoms * S, 3, dtype=torch.float32, device=dev)
        amp = torch.empty(3 * n_atoms * S, dtype=torch.float32, device=dev)
        energy = torch.zeros(n_mol * S, dtype=torch.float32, device=dev)
        skipped = torch.zeros(n_mol, dtype=torch.int32, device=dev)
        bound = max_dim()
        large = [False] * n_mol if kernel == 'lds' else [n > 0 and (kernel == 'tiled' or 3 * n > bound) for n in self._counts]
        if any(large):
            bound_large = max_dim_sample_large()
            for b, n in enumerate(self._counts):
                if large[b] and 3 * n > bound_large:
                    raise NotImplementedError(f'molecule {b} has 3 x {n} = {3 * n} coordinates, above the {bound_large} the tiled '
                                              f'sampling kernel serves (nnhip_mode_sample_large_max_dim)')
        L, stream = hip.lib(), hip._stream(dev)

        def call(fn, first, count, *tail):
            """fn on the molecules first .. first + count - 1: the per-molecule pointers moved up by `first` (`energy`, which the
            kernels index by b S, by first x S); everything else is addressed through the absolute offsets they hold"""
            return fn(hip._ptr(self.modes), hip._ptr(self.eigenvalues), self.blk_ptr.data_ptr() + 8 * first,
                      mol_dev.data_ptr() + 4 * first, mol_host.data_ptr() + 4 * first, count, hip._ptr(self.masses), hip._ptr(pos_c),
                      self.threshold.data_ptr() + 4 * first, T, 1 if quantum else 0, S, hip._ptr(xi), hip._ptr(new_pos),
                      energy.data_ptr() + 4 * first * S, hip._ptr(amp), skipped.data_ptr() + 4 * first, *tail, stream)
        if n_mol and not any(large):
            rc = call(L.nnhip_mode_sample, 0, n_mol)
            if rc == 2:
                raise NotImplementedError(L.nnhip_last_error().decode())
            hip._check(rc, 'nnhip_mode_sample')
        elif n_mol:
            # nnhip_mode_sample on every run of consecutive molecules it serves, as _solve_mixed does for the eigensolver, and one
            # nnhip_mode_sample_large call on the others: it picks them by their size on the device and touches nothing of the
            # rest, so both write the same packed outputs
            b = 0
            while b < n_mol:
                if large[b]:
                    b += 1
                    continue
                e = b
                while e < n_mol and not large[e]:
                    e += 1
                if sum(self._counts[b:e]):
                    hip._check(call(L.nnhip_mode_sample, b, e - b), 'nnhip_mode_sample')
                b = e
            rc = call(L.nnhip_mode_sample_large, 0, n_mol, 0 if kernel == 'tiled' else bound + 1)
            if rc == 2:
                raise NotImplementedError(L.nnhip_last_error().decode())
            hip._check(rc, 'nnhip_mode_sample_large')
        # the sample batch: molecule b S + s is sample s of molecule b
        counts = (mol_dev[1:] - mol_dev[:-1]).long()
        mol_of = torch.arange(n_mol, device=dev).repeat_interleave(S)
        batch = torch.arange(n_mol * S, device=dev).repeat_interleave(counts[mol_of], output_size=n_atoms * S)
        new_z = None
        if z is not None:
            first_new = S * mol_dev[:-1].long()[mol_of] + (torch.arange(n_mol * S, device=dev) % S) * counts[mol_of]
            src = mol_dev[:-1].long()[mol_of][batch] + torch.arange(n_atoms * S, device=dev) - first_new[batch]
            new_z = z.reshape(-1)[src]
        return ModeSamples(z=new_z, pos=new_pos, cell=cell.repeat_interleave(S, dim=0), batch=batch, harmonic_energy=energy,
                           n_skipped_imaginary=skipped.long(), amplitudes=amp, n_samples=S, temperature=T, quantum=bool(quantum))

    def thermochemistry(self, temperature: float) -> 'Thermochemistry':
        """Harmonic vibrational thermochemistry per molecule at `temperature` (K) over the live modes, with x = eps / k_B T and
        eps = hbar omega per mode:
            U_vib = sum eps / 2 + eps / (e^x - 1)                       eV  (the first sum is zero_point_energy)
            S_vib = k_B sum x / (e^x - 1) - ln(1 - e^-x)                eV / K
            F_vib = U - T S = sum eps / 2 + k_B T ln(1 - e^-x)          eV  (summed in this per-mode form)
            C_v   = k_B sum x^2 e^-x / (1 - e^-x)^2                     eV / K
        fp32 [B] each.  The per-mode terms are elementwise torch ops in fp64 on the packed device arrays (e^-x is as
        ill-conditioned as x is large), rounded to fp32 and summed per molecule by the deterministic hip.segment_sum; x is capped at
        100, where every thermal term is below the smallest fp32 number relative to eps.  T = 0 returns U = F = the zero-point
        energy and S = C_v = 0."""
        T = _temperature(temperature)
        n_mol = len(self._counts)
        zpe = self.zero_point_energy
        if T == 0.0 or self.eigenvalues.numel() == 0:
            zero = torch.zeros_like(zpe)
            return Thermochemistry(U=zpe.clone(), S=zero, F=zpe.clone(), Cv=zero.clone(), temperature=T)
        kT = K_BOLTZMANN * T
        live, _ = self._live()
        eps = EV_PER_SQRT_EIGENVALUE * torch.where(live, self.eigenvalues, torch.ones_like(self.eigenvalues)).double().sqrt()
        x = (eps / kT).clamp(max=100.0)
        em = torch.exp(-x)
        om = -torch.expm1(-x)                     # 1 - e^-x
        occ = em / om                             # 1 / (e^x - 1)
        ln = torch.log(om)
        terms = torch.stack([eps * occ, K_BOLTZMANN * (x * occ - ln), kT * ln, K_BOLTZMANN * x * x * em / (om * om)], dim=1)
        terms = torch.where(live[:, None], terms, torch.zeros_like(terms)).float().contiguous()
        s = hip.segment_sum(terms, self.ptr.to(torch.int32), n_mol)
        return Thermochemistry(U=zpe + s[:, 0], S=s[:, 1].contiguous(), F=zpe + s[:, 2], Cv=s[:, 3].contiguous(), temperature=T)


def derived_quantities(evals: torch.Tensor, ptr: torch.Tensor, batch: torch.Tensor, n_mol: int, tol_zero: Optional[float] = None):
    """(frequencies [3N], threshold [B], n_imaginary [B], zero_point_energy [B]) of packed eigenvalues that ascend per molecule:
    elementwise on the packed arrays + one segmented sum."""
    dev = evals.device
    n_atoms = evals.numel() // 3
    counts_dev = ((ptr[1:] - ptr[:-1]) // 3).long()
    freq = torch.sign(evals) * evals.abs().sqrt() * WAVENUMBER_PER_SQRT_EIGENVALUE
    if n_atoms:
        thr_mol = zero_threshold(evals, ptr, counts_dev, tol_zero)
        thr = thr_mol[batch.long().reshape(-1)].repeat_interleave(3)
        imag, real = evals < -thr, evals > thr
        x = torch.stack([imag.float(), (0.5 * EV_PER_WAVENUMBER) * freq * real], dim=1).contiguous()
        s = hip.segment_sum(x, ptr.to(torch.int32), n_mol)
        n_imag, zpe = s[:, 0].round().long(), s[:, 1].contiguous()
    else:
        thr_mol = torch.zeros(n_mol, dtype=torch.float32, device=dev)
        n_imag = torch.zeros(n_mol, dtype=torch.long, device=dev)
        zpe = torch.zeros(n_mol, dtype=torch.float32, device=dev)
    return freq, thr_mol, n_imag, zpe


def eig_blocks(blocks: torch.Tensor, blk_ptr: torch.Tensor, batch: torch.Tensor, pos: torch.Tensor, cell: torch.Tensor,
               masses: Optional[torch.Tensor] = None, project: bool = True, modes: bool = True,
               tol_zero: Optional[float] = None, counts: Optional[torch.Tensor] = None,
               z: Optional[torch.Tensor] = None, solver: str = 'lds') -> NormalModes:
    """The solver alone on packed blocks the caller already has (layout of hessian_blocks; atoms of a molecule contiguous and
    molecules ascending in `batch`: not checked, a check would cost a copy to the host).  masses: fp32 [N] in amu, None = unit
    masses (plain eigenvalues of the symmetrised block); a molecule with a mass that is not positive and finite is not computed
    and says so in `status` (bit 2), checked on the device.
    counts: atoms per molecule as a CPU tensor if the caller has them (else one bincount is copied to the host).
    modes=False skips the eigenvectors; the eigenvalues are bitwise the same either way (the rotations of the matrix do not depend
    on the accumulated vectors).  z: atomic numbers, kept on the result for sample() (not used by the solver).
    solver: 'lds' (default) -- nnhip_eig_blocks, one workgroup per molecule, NotImplementedError above max_dim() = 126 coordinates;
    'auto' -- the molecules within max_dim() go through nnhip_eig_blocks, bitwise as with 'lds', the others through the blocked
    solver (nnhip_eig_blocks_large, csrc/eig_large.hip: block Jacobi over many workgroups, the matrix in a torch-owned workspace,
    one small read-back per sweep), NotImplementedError above max_dim_large(); 'blocked' -- every molecule through the blocked
    solver.  All land in one packed NormalModes."""
    _check_solver(solver)
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
    large = [False] * n_mol if solver == 'lds' else [n > 0 and (solver == 'blocked' or 3 * n > bound) for n in cl]
    if solver == 'lds':
        for b, n in enumerate(cl):
            if 3 * n > bound:
                raise NotImplementedError(f'molecule {b} has 3 x {n} = {3 * n} coordinates, above the {bound} the batched eigensolver '
                                          f'serves (nnhip_eig_max_dim)')
    elif any(large):
        bound_large = max_dim_large()
        for b, n in enumerate(cl):
            if large[b] and 3 * n > bound_large:
                raise NotImplementedError(f'molecule {b} has 3 x {n} = {3 * n} coordinates, above the {bound_large} the blocked '
                                          f'eigensolver serves (nnhip_eig_large_max_dim)')
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
    if n_mol and n_atoms and not any(large):
        rc = hip.lib().nnhip_eig_blocks(hip._ptr(blocks), hip._ptr(blk_ptr), hip._ptr(mol_dev), mol_host.data_ptr(), n_mol,
                                        hip._ptr(pos_c), hip._ptr(cell_c), hip._ptr(m_c), EIG_PROJECT if project else 0, hip._ptr(evals),
                                        hip._ptr(vecs), hip._ptr(n_proj), hip._ptr(sweeps), hip._ptr(status), hip._stream(dev))
        if rc == 2:
            raise NotImplementedError(hip.lib().nnhip_last_error().decode())
        hip._check(rc, 'nnhip_eig_blocks')
    elif n_mol and n_atoms:
        _solve_mixed(blocks, blk_ptr, mol_dev, mol_host, cl, large, pos_c, cell_c, m_c, project, evals, vecs, n_proj, sweeps, status)
    freq, thr_mol, n_imag, zpe = derived_quantities(evals, ptr, batch, n_mol, tol_zero)
    return NormalModes(eigenvalues=evals, frequencies=freq, modes=vecs, ptr=ptr, blk_ptr=blk_ptr, n_projected=n_proj, sweeps=sweeps,
                       status=status, n_imaginary=n_imag, zero_point_energy=zpe, masses=m_c, _counts=cl,
                       _offsets=mol_host[:-1].tolist(), _blk_offsets=blk_off, threshold=thr_mol, pos=pos_c, cell=cell_c,
                       z=None if z is None else z.detach())


def _solve_mixed(blocks, blk_ptr, mol_dev, mol_host, cl, large, pos_c, cell_c, m_c, project, evals, vecs, n_proj, sweeps, status):
    """solver='auto' / 'blocked': nnhip_eig_blocks on every run of consecutive molecules the one-workgroup solver serves (it takes a
    batch as offsets into the packed arrays, so a run is the same call with the per-molecule pointers moved up), one
    nnhip_eig_blocks_large call on the others; both write the same packed outputs."""
    L, dev, n_mol, flags = hip.lib(), blocks.device, len(cl), EIG_PROJECT if project else 0
    b = 0
    while b < n_mol:
        if large[b]:
            b += 1
            continue
        e = b
        while e < n_mol and not large[e]:
            e += 1
        if sum(cl[b:e]):
            rc = L.nnhip_eig_blocks(hip._ptr(blocks), blk_ptr.data_ptr() + 8 * b, mol_dev.data_ptr() + 4 * b,
                                    mol_host.data_ptr() + 4 * b, e - b, hip._ptr(pos_c), cell_c.data_ptr() + 36 * b, hip._ptr(m_c),
                                    flags, hip._ptr(evals), hip._ptr(vecs), n_proj.data_ptr() + 4 * b, sweeps.data_ptr() + 4 * b,
                                    status.data_ptr() + 4 * b, hip._stream(dev))
            hip._check(rc, 'nnhip_eig_blocks')
        b = e
    select = torch.tensor(large, dtype=torch.uint8)
    sel_host = torch.zeros(sum(large) + 1, dtype=torch.int32)          # the workspace is sized by the selected molecules alone
    sel_host[1:] = torch.cumsum(torch.tensor([n for n, big in zip(cl, large) if big], dtype=torch.int32), 0)
    ws_bytes = int(L.nnhip_eig_large_ws_bytes(sel_host.data_ptr(), sel_host.numel() - 1, 0 if vecs is None else 1))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rc = L.nnhip_eig_blocks_large(hip._ptr(blocks), hip._ptr(blk_ptr), hip._ptr(mol_dev), mol_host.data_ptr(), n_mol, hip._ptr(pos_c),
                                  hip._ptr(cell_c), hip._ptr(m_c), flags, hip._ptr(evals), hip._ptr(vecs), hip._ptr(n_proj),
                                  hip._ptr(sweeps), hip._ptr(status), select.data_ptr(), hip._ptr(ws), ws_bytes, hip._stream(dev))
    if rc == 2:
        raise NotImplementedError(L.nnhip_last_error().decode())
    hip._check(rc, 'nnhip_eig_blocks_large')


def normal_modes(model, z, pos, cell, batch, masses: Optional[torch.Tensor] = None, project: bool = True, modes: bool = True,
                 tol_zero: Optional[float] = None, solver: str = 'lds') -> NormalModes:
    """Harmonic analysis of every molecule of the batch at the current parameters: Hessian blocks (hessian.hessian_blocks) and
    the batched solver, on the caller's current stream.  masses=None: standard atomic weights of z (ValueError for an element
    outside the built-in table).  project: remove translations and rotations (translations only for periodic molecules).
    tol_zero: relative threshold below which an eigenvalue counts as zero (default 8 x 3 n_b x 2^-24, the solver's error bound,
    so projected modes are never counted as imaginary or real).  solver: 'lds' (molecules up to max_dim() = 126 coordinates),
    'auto' (larger ones go through the blocked solver, up to max_dim_large()) or 'blocked': see eig_blocks."""
    _check_solver(solver)
    _hessian._validate(model, pos)
    m = table_masses(z) if masses is None else masses
    blocks, blk_ptr, counts = _hessian.hessian_blocks_counts(model, z, pos, cell, batch)
    return eig_blocks(blocks, blk_ptr, batch, pos, cell, m, project=project, modes=modes, tol_zero=tol_zero, counts=counts, z=z,
                      solver=solver)
