"""Batched variable-cell geometry relaxation on the HIP path: the atoms AND the cell of every periodic system of a batch are
relaxed on the device to zero stress (or to stress equal to a target pressure), one model() call and one optimiser launch
(nnhip_cell_lbfgs_step, csrc/cellrelax.hip) per step, with no host round trip of positions, cells, forces or virials.

The method is ASE's UnitCellFilter (ase.filters) under ASE's L-BFGS as `Relaxation` has it (relax.py: fixed H0 = 1 / alpha, the
longest row of a step capped at maxstep, a curvature pair kept only when y.s > 0 and cos(y, s) > 1e-4).  Per system, with h the
cell (rows are lattice vectors), h0 the cell at construction, x the Cartesian positions, f the forces, W the virial (out.virial,
or -out.displacement_grad with a 'stress' head, as npt.py selects it), V = det h, p the target pressure and c = cell_factor:

    state                      the deformation gradient F and reference-frame positions q:   h = h0 F^T,   x = q F^T
    generalised coordinates    X = [q ; c F]                      n + 3 rows of 3
    generalised forces         G = [f F ; Wc / c]                 Wc = (W - p V I) F^-T

G is minus the gradient of the enthalpy H = E + p V with respect to X.  Applied to Wc, in this order: hydrostatic=True replaces
it by (tr Wc / 3) I; `mask` (six 0/1 flags in Voigt order xx, yy, zz, yz, xz, xy) multiplies it elementwise by the symmetric 3x3
mask; constant_volume=True subtracts tr Wc / 3 from its diagonal.  A system has converged when the largest |G_row| over atom rows
and cell rows alike is below fmax (compared as squares in fp32) -- ASE's criterion under a filter.  A fixed atom has its row of G
exactly 0: its reference-frame position q is frozen, so it RIDES WITH THE CELL (its Cartesian position changes when F does).

`form` chooses the launch as for `Relaxation` (relax.py): 'wave' (the default) gives one wave64 to a system, 'workgroup' one
workgroup of hip.LBFGS_WG_THREADS threads (nnhip_cell_lbfgs_step_wg; for one large box), 'auto' the workgroup form to the systems
of at least wg_min_atoms ATOMS (the chain walks n + 3 rows) and the wave form to the others, decided on the device.

Left out on purpose: Frechet / exponential cell filters; cell relaxation of bands, dimers and reaction paths.

Units: positions in Angstrom, forces and fmax in eV / Angstrom, alpha in eV / Angstrom^2, pressure and stress in bar."""
from __future__ import annotations

import math

import numpy as np
import torch

from newtonnet_amd import hip
from newtonnet_amd.dynamics import _mol_ptr
from newtonnet_amd.npt import BAR, _per_system
from newtonnet_amd.relax import check_arguments, check_form, check_inputs
from newtonnet_amd.stepper import Stepper

_F32 = torch.float32
_TRAJ = (('pos', ('n_atoms', 3), _F32), ('cell', ('n_mol', 3, 3), _F32), ('force', ('n_atoms', 3), _F32),
         ('virial', ('n_mol', 3, 3), _F32), ('energy', ('n_mol',), _F32), ('n_pairs', ('n_mol',), torch.int64))


class CellRelaxResult:
    """What CellRelaxation.run returns, as device tensors:

    pos        fp32 [N,3]     positions after the last step;   cell fp32 [B,3,3]: the cells after the last step
    volume     fp32 [B]       det(cell), Angstrom^3
    energy     fp32 [B]       the model's energy at (pos, cell);   enthalpy fp32 [B]: energy + p V
    stress     fp32 [B,3,3]   -virial / V in bar (the sign convention of the model's 'stress' head; at convergence -p on the
                              free diagonal components)
    fmax       fp32 [B]       the largest generalised force norm, over atom rows and cell rows, at (pos, cell)
    converged  bool [B]       fmax < the threshold, now or at an earlier step (sticky);   failed bool [B]: fmax is NaN (the launch
                              skipped the system: det F <= 0 or a non-finite cell);   n_steps int64 [B]: steps taken
    traj_*     only with record_every > 0, over the R recorded steps: traj_step int64 [R], traj_pos and traj_force fp32 [R,N,3],
               traj_cell and traj_virial fp32 [R,B,3,3], traj_energy fp32 [R,B], traj_n_pairs int64 [R,B] (force, virial and
               energy are the model's at the recorded pos and cell)
    """

    def __init__(self, pos, cell, volume, energy, enthalpy, stress, fmax, converged, failed, n_steps):
        self.pos, self.cell, self.volume, self.energy, self.enthalpy = pos, cell, volume, energy, enthalpy
        self.stress, self.fmax, self.converged, self.failed, self.n_steps = stress, fmax, converged, failed, n_steps
        self.traj_step = None
        for name, _, _ in _TRAJ:
            setattr(self, 'traj_' + name, None)


def check_model(model, who):
    """eval mode and a virial or stress head, refused without touching the device; returns the model's output properties"""
    if getattr(model, 'training', False):
        raise ValueError(f'{who} needs the model in eval mode: call model.eval()')
    props = list(getattr(model, 'output_properties', []))
    if 'virial' not in props and 'stress' not in props:
        raise ValueError(f"{who} needs a model with a 'virial' or 'stress' head (it has {props})")
    return props


def check_cell_arguments(n_mol, pressure, mask, hydrostatic, constant_volume, cell_factor):
    """the cell filter's arguments, refused without touching the device; returns (pressure fp64 [B] in bar, strain_mask bits,
    flags, cell_factor float or None)"""
    P = _per_system(pressure, n_mol, 'pressure')
    if not bool(torch.isfinite(P).all()):
        raise ValueError('pressure: finite values expected')
    bits = hip.CELL_LBFGS_MASK_ALL
    if mask is not None:
        m = np.asarray(mask.detach().cpu() if isinstance(mask, torch.Tensor) else mask)
        if m.shape != (6,) or not np.isin(m, (0, 1)).all():
            raise ValueError(f'mask: six 0/1 flags in Voigt order xx, yy, zz, yz, xz, xy expected (got shape {m.shape})')
        bits = sum(1 << k for k in range(6) if m[k])
    for name, v in (('hydrostatic', hydrostatic), ('constant_volume', constant_volume)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f'{name}: True or False expected (got {v!r})')
    flags = (hip.CELL_LBFGS_HYDROSTATIC if hydrostatic else 0) | (hip.CELL_LBFGS_CONSTANT_VOLUME if constant_volume else 0)
    if cell_factor is not None:
        cell_factor = float(cell_factor)
        if not (cell_factor > 0.0 and math.isfinite(cell_factor)):
            raise ValueError(f'cell_factor: a finite value > 0 expected (got {cell_factor!r})')
    return P, bits, flags, cell_factor


class CellRelaxation(Stepper):
    """B periodic systems relaxed together on the device, atoms and cells.

    model: a NewtonNet in eval mode with the 'energy' and 'gradient_force' heads and a 'virial' or 'stress' head.  z, pos, cell,
    batch: as for model(...), on the device; none of them is modified.  fmax, memory, maxstep, alpha: as for Relaxation, with
    fmax and maxstep taken over the n + 3 generalised rows of a system.  pressure: bar, a number or [B].  mask, hydrostatic,
    constant_volume: the module docstring.  cell_factor: c; None = the system's atom count (ASE's default; 1 for an empty system).
    fixed: bool [N]; a fixed atom keeps its reference-frame position, so it rides with the cell.  Every system needs
    det(cell) > 0 (checked once, at construction, with one host read).  Positions stay unwrapped.  form, wg_min_atoms: as for
    Relaxation ('wave', 'workgroup' or 'auto'; the threshold of 'auto' counts atoms)."""
    NOUN, CHECK_ONLY, TRAJ = 'relaxations', hip.CELL_LBFGS_CHECK_ONLY, _TRAJ

    def __init__(self, model, z, pos, cell, batch, fmax=0.01, memory=16, maxstep=0.2, alpha=70.0, pressure=0.0, mask=None,
                 hydrostatic=False, constant_volume=False, cell_factor=None, fixed=None, form='wave', wg_min_atoms=None):
        # ---- everything that can be refused without touching the device
        N, B = check_inputs(model, 'CellRelaxation', z, pos, cell, batch, fixed)
        props = check_model(model, 'CellRelaxation')
        fmax, memory, maxstep, alpha = check_arguments(fmax, memory, maxstep, alpha)
        P, bits, flags, cell_factor = check_cell_arguments(B, pressure, mask, hydrostatic, constant_volume, cell_factor)
        self.form, self._wg_min_atoms = form, check_form(form, wg_min_atoms)
        dev = self._check_device(pos, z=z, cell=cell, batch=batch, fixed=fixed)
        if B and not bool((torch.linalg.det(cell.detach().double()) > 0).all().cpu()):       # (the one host read)
            raise ValueError('CellRelaxation needs periodic systems with det(cell) > 0 (a right-handed cell of positive volume)')
        # ---- state
        self.model, self.z, self.batch = model, z, batch
        self.n_atoms, self.n_mol = N, B
        self.fmax, self.memory = fmax, memory
        self._virial_of = (lambda out: out.virial) if 'virial' in props else (lambda out: -out.displacement_grad)
        self._tol2 = float(np.float32(fmax * fmax))
        self._maxstep, self._alpha = float(np.float32(maxstep)), float(np.float32(alpha))
        self._bits, self._flags = bits, flags
        R = N + 3 * B
        with torch.no_grad():
            f32 = dict(dtype=torch.float32, device=dev)
            self._free = None if fixed is None else (~fixed).contiguous()
            self._mol_ptr = _mol_ptr(batch, B)
            counts = (self._mol_ptr[1:] - self._mol_ptr[:-1]).to(torch.float32)
            self._c = torch.full((B,), cell_factor, **f32) if cell_factor is not None else counts.clamp(min=1.0)
            self._p = (P.to(dev) * BAR).to(torch.float32).contiguous()
            self._h0 = cell.detach().clone().contiguous()
            # two buffers each of X, pos and cell: a step reads one set and writes the other (Stepper._init_buffers)
            self._init_buffers(pos.detach().clone().contiguous())
            self._cells = [self._h0.clone(), torch.empty(B, 3, 3, **f32)]
            # X = [q ; c F] per system with F = I: system b's rows are [mol_ptr[b] + 3 b, mol_ptr[b+1] + 3 b + 3)
            shift = 3 * batch.long()
            self._atom_rows = torch.arange(N, device=dev) + shift
            cell_rows = (self._mol_ptr[1:].long() + 3 * torch.arange(B, device=dev))[:, None] + torch.arange(3, device=dev)
            x0 = torch.empty(R, 3, **f32)
            x0[self._atom_rows] = self._pos[0]
            x0[cell_rows.reshape(-1)] = (self._c[:, None, None] * torch.eye(3, **f32)).reshape(-1, 3)
            self._x = [x0, torch.empty(R, 3, **f32)]

            def ints():
                return torch.zeros(B, dtype=torch.int32, device=dev)
            self._converged, self._n_steps, self._n_pairs, self._head = ints(), ints(), ints(), ints()
            self._active = self._converged
            self._S = torch.zeros(memory, R, 3, **f32)
            self._Y = torch.zeros(memory, R, 3, **f32)
            self._rho = torch.zeros(B, memory, **f32)
            self._g_prev = torch.zeros(R, 3, **f32)
            self._G = torch.zeros(R, 3, **f32)
            self._work = torch.empty(R, 3, **f32) if R > 64 else None
            self._fmax = torch.zeros(B, **f32)
            self._virial = None

    # ------------------------------------------------------------------------------------------
    def _evaluate(self):
        """forces, energies and the virial at the current positions and cell.  Touching them settles the deferred record of the
        call -- a repeat, if one is needed, happens HERE, from the buffers the call was queued with and before any kernel writes a
        buffer"""
        out = self.model(self.z, self._pos[self._cur], self._cells[self._cur], self.batch)
        self._force = out.gradient_force
        self._energy = out.energy
        self._virial = self._virial_of(out)

    def _launch(self, flags=0):
        """one launch: reads the current buffers, forces and virial, writes the other buffers, and the buffers swap"""
        cur, other = self._cur, 1 - self._cur
        hip.cell_lbfgs_step(self._x[cur], self._pos[cur], self._force, self._virial, self._cells[cur], self._h0, self._free,
                            self._mol_ptr, self._p, self._c, self.memory, self._tol2, self._alpha, self._maxstep, self._bits,
                            self._flags | flags, self._converged, self._n_steps, self._n_pairs, self._head, self._S, self._Y,
                            self._rho, self._g_prev, self._work, self._G, self._x[other], self._pos[other], self._cells[other],
                            self._fmax, wg_min_atoms=self._wg_min_atoms)
        self._cur = other

    @property
    def cell(self):
        return self._cells[self._cur].detach().clone()

    @property
    def virial(self):
        self._ensure_state()
        return self._virial

    @property
    def n_pairs(self):
        return self._n_pairs.long()

    # ------------------------------------------------------------------------------------------
    # run (Stepper.run): variable-cell L-BFGS steps of every system that has not converged; the check-only launch measures fmax
    # at the state reached and marks what has converged there (it copies X, positions and cells into the other buffers)
    def _frame(self):
        return (self._pos[self._cur].clone(), self._cells[self._cur].clone(), self._force.clone(), self._virial.clone(),
                self._energy.clone(), self._n_pairs.long())

    def _result(self):
        cell = self._cells[self._cur].clone()
        volume = torch.linalg.det(cell.double()).float() if self.n_mol else torch.zeros(0, dtype=torch.float32, device=cell.device)
        energy = self._energy.clone()
        stress = -self._virial / volume[:, None, None] * (1.0 / BAR)
        return CellRelaxResult(self._pos[self._cur].clone(), cell, volume, energy, energy + self._p * volume, stress,
                               self._fmax.clone(), self._converged != 0, torch.isnan(self._fmax), self._n_steps.long())
