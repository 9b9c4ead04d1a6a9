"""Batched geometry relaxation on the HIP path: every molecule of a batch is relaxed to a minimum on the device, one force
evaluation and one optimiser launch (nnhip_lbfgs_step, csrc/relax.hip) per step, with no host round trip of positions or forces.

The reference leaves optimisation to an outside driver that calls its calculator once per step for one structure.
Here `Relaxation` owns the positions and the L-BFGS histories of B molecules as device tensors and steps them together.  The
method is L-BFGS without line search in ASE's convention (ase.optimize.LBFGS: fixed H0 = 1 / alpha, the longest atomic displacement
of a step capped at maxstep), every molecule with its own history and its own sticky `converged` flag.  One deviation from ASE,
stated in include/newtonnet_hip.h: a curvature pair enters the history only when y.s > 0 and cos(y, s) > 1e-4.

A molecule that has converged is frozen -- later launches leave every bit of it alone -- but model() keeps evaluating it with the
rest of the batch: compacting the batch is not done here.  Minima only (saddles: newtonnet_amd.dimer, which takes its translation
from the same device code, csrc/lbfgs_chain.h) at a fixed cell (the cell is relaxed by newtonnet_amd.cellrelax, again on that
device code): no Hessian-based steps, no constraint other than fixed atoms.

Two forms of the launch, chosen with `form`: 'wave' (the default) gives one wave64 to a molecule, whatever its size -- it is meant
for batches of molecules, and one large system pays about 2 memory ceil(n / 64) dependent sweeps of a single wave per step;
'workgroup' gives every molecule one workgroup of hip.LBFGS_WG_THREADS threads (nnhip_lbfgs_step_wg), for large systems; 'auto'
sends the molecules of at least wg_min_atoms atoms to the workgroup form and the others to the wave form, decided per molecule on
the device.  Both forms satisfy the same contract; their bits differ from each other because their reductions are ordered
differently (above 64 atoms; up to 64 they agree).  WG_AUTO_MIN_ATOMS, the default threshold of 'auto', is measured: the smallest
size of the sweep of tools/bench_relax_large.py from which on the workgroup launch is no slower at 1 and at 64 systems.

Units: positions in Angstrom, forces and fmax in eV / Angstrom, alpha in eV / Angstrom^2."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from newtonnet_amd import hip
from newtonnet_amd.dynamics import _mol_ptr
from newtonnet_amd.stepper import Stepper, check_run_arguments          # noqa: F401 (check_run_arguments: callers import it from here)


FORMS = ('wave', 'workgroup', 'auto')
WG_AUTO_MIN_ATOMS = 128          # default wg_min_atoms of form='auto': measured (tools/bench_relax_large.py, profiles/relax_large.json)


def check_form(form, wg_min_atoms):
    """form and wg_min_atoms of a driver, refused without touching the device; returns the wg_min_atoms argument of
    hip.lbfgs_step / hip.cell_lbfgs_step: None ('wave': the wave entry point), 0 ('workgroup': every system) or the threshold
    ('auto')"""
    if not isinstance(form, str) or form not in FORMS:
        raise ValueError(f"form: one of {', '.join(repr(f) for f in FORMS)} expected (got {form!r})")
    if wg_min_atoms is None:
        wg_min_atoms = WG_AUTO_MIN_ATOMS
    elif (isinstance(wg_min_atoms, (bool, np.bool_)) or not isinstance(wg_min_atoms, (int, np.integer)) or
          not 1 <= wg_min_atoms < 2 ** 31):
        raise ValueError(f'wg_min_atoms: None or a positive int expected (got {wg_min_atoms!r})')
    return {'wave': None, 'workgroup': 0, 'auto': int(wg_min_atoms)}[form]


class RelaxResult:
    """What Relaxation.run returns, as device tensors:

    pos        fp32 [N,3]   positions after the last step
    energy     fp32 [B]     the model's energy at pos;  fmax fp32 [B]: the largest force norm on a free atom at pos
    converged  bool [B]     fmax < the threshold, now or at an earlier step (the flag is sticky);  n_steps int64 [B]: steps taken
    traj_*     only with record_every > 0, over the R recorded steps: traj_step int64 [R] (steps since the Relaxation was made),
               traj_pos and traj_force fp32 [R,N,3] (the forces are the ones the next launch consumed at those positions),
               traj_energy fp32 [R,B], traj_n_pairs int64 [R,B] (pairs in each molecule's history after that step)
    """

    def __init__(self, pos, energy, fmax, converged, n_steps, traj=None):
        self.pos, self.energy, self.fmax, self.converged, self.n_steps = pos, energy, fmax, converged, n_steps
        self.traj_step = self.traj_pos = self.traj_force = self.traj_energy = self.traj_n_pairs = None
        if traj is not None:
            self.traj_step, self.traj_pos, self.traj_force, self.traj_energy, self.traj_n_pairs = traj


def check_arguments(fmax, memory, maxstep, alpha):
    """the optimiser's numbers, refused without touching the device; returns them as (float, int, float, float)"""
    if int(memory) != memory or not 1 <= memory <= hip.LBFGS_MAX_MEMORY:
        raise ValueError(f'memory: an integer in 1 .. {hip.LBFGS_MAX_MEMORY} expected (got {memory!r})')
    fmax, maxstep, alpha = float(fmax), float(maxstep), float(alpha)
    if not (fmax > 0.0 and math.isfinite(fmax)):
        raise ValueError(f'fmax: a finite value > 0 eV/Angstrom expected (got {fmax!r})')
    if not (maxstep > 0.0 and math.isfinite(maxstep)):
        raise ValueError(f'maxstep: a finite value > 0 Angstrom expected (got {maxstep!r})')
    if not (alpha > 0.0 and math.isfinite(alpha)):
        raise ValueError(f'alpha: a finite value > 0 eV/Angstrom^2 expected (got {alpha!r})')
    return fmax, int(memory), maxstep, alpha


def check_inputs(model, who, z, pos, cell, batch, fixed):
    """the model and the tensors of a driver named `who` (Relaxation, SaddleSearch), refused without touching the device; returns
    (N, B)"""
    if getattr(model, 'training', False):
        raise ValueError(f'{who} needs the model in eval mode: call model.eval()')
    props = list(getattr(model, 'output_properties', []))
    if 'energy' not in props or 'gradient_force' not in props:
        raise ValueError(f"{who} needs a model with the 'energy' and 'gradient_force' heads (it has {props})")
    for name, t in (('z', z), ('pos', pos), ('cell', cell), ('batch', batch)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'{name}: a tensor expected (got {type(t).__name__})')
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f'pos: [N,3] expected (got {tuple(pos.shape)})')
    N = pos.shape[0]
    if cell.dim() != 3 or tuple(cell.shape[1:]) != (3, 3):
        raise ValueError(f'cell: [B,3,3] expected (got {tuple(cell.shape)})')
    B = cell.shape[0]
    if tuple(z.shape) != (N,) or tuple(batch.shape) != (N,):
        raise ValueError(f'z and batch: [{N}] expected (got {tuple(z.shape)}, {tuple(batch.shape)})')
    if pos.dtype != torch.float32 or cell.dtype != torch.float32:
        raise ValueError(f'pos and cell: float32 expected (got {pos.dtype}, {cell.dtype})')
    if fixed is not None and (not isinstance(fixed, torch.Tensor) or fixed.dtype != torch.bool or tuple(fixed.shape) != (N,)):
        raise ValueError(f'fixed: a bool tensor [{N}] expected')
    return N, B


class Relaxation(Stepper):
    """B molecules relaxed together on the device.

    model: a NewtonNet in eval mode with the 'energy' and 'gradient_force' heads.  z, pos, cell, batch: as for model(...), on the
    device; none of them is modified (the positions are copied).  fmax: a molecule has converged when the largest force norm on one
    of its free atoms is below it (compared as squares in fp32: |f|^2 < fl32(fmax^2)).  memory: pairs kept per molecule.  maxstep:
    cap on the longest atomic displacement of a step.  alpha: the initial inverse Hessian is 1 / alpha.  fixed: bool [N], atoms
    that never move.  form: 'wave' (one wave64 per molecule, the default), 'workgroup' (one workgroup per molecule, for large
    systems) or 'auto' (per molecule on the device: the workgroup form from wg_min_atoms atoms on; None = WG_AUTO_MIN_ATOMS);
    wg_min_atoms means something with 'auto' only.

    Periodic molecules: the cell is fixed and positions stay unwrapped; the model's neighbor list takes the minimum image itself."""
    NOUN, CHECK_ONLY = 'relaxations', hip.LBFGS_CHECK_ONLY
    TRAJ = (('pos', ('n_atoms', 3), torch.float32), ('force', ('n_atoms', 3), torch.float32), ('energy', ('n_mol',), torch.float32),
            ('n_pairs', ('n_mol',), torch.int64))

    def __init__(self, model, z, pos, cell, batch, fmax=0.01, memory=16, maxstep=0.2, alpha=70.0, fixed=None, form='wave',
                 wg_min_atoms=None):
        # ---- everything that can be refused without touching the device
        N, B = check_inputs(model, 'Relaxation', z, pos, cell, batch, fixed)
        fmax, memory, maxstep, alpha = check_arguments(fmax, memory, maxstep, alpha)
        self.form, self._wg_min_atoms = form, check_form(form, wg_min_atoms)
        dev = self._check_device(pos, z=z, cell=cell, batch=batch, fixed=fixed)
        # ---- state
        self.model, self.z, self.cell, self.batch = model, z, cell, batch
        self.n_atoms, self.n_mol = N, B
        self.fmax, self.memory = fmax, memory
        # the numbers the kernel gets, as the Python floats of their fp32 values
        self._tol2 = float(np.float32(fmax * fmax))
        self._maxstep, self._alpha = float(np.float32(maxstep)), float(np.float32(alpha))
        with torch.no_grad():
            self._free = None if fixed is None else (~fixed).contiguous()
            self._init_buffers(pos.detach().clone().contiguous())
            self._mol_ptr = _mol_ptr(batch, B)

            def ints():
                return torch.zeros(B, dtype=torch.int32, device=dev)
            self._converged, self._n_steps, self._n_pairs, self._head = ints(), ints(), ints(), ints()
            self._active = self._converged
            self._S = torch.zeros(memory, N, 3, dtype=torch.float32, device=dev)
            self._Y = torch.zeros(memory, N, 3, dtype=torch.float32, device=dev)
            self._rho = torch.zeros(B, memory, dtype=torch.float32, device=dev)
            self._f_prev = torch.zeros(N, 3, dtype=torch.float32, device=dev)
            self._work = torch.empty(N, 3, dtype=torch.float32, device=dev) if N > 64 else None
            self._fmax = torch.zeros(B, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------------------------------
    def _launch(self, flags=0):
        """one launch: reads the current buffer and the current forces, writes the other buffer, and the buffers swap"""
        other = 1 - self._cur
        hip.lbfgs_step(self._pos[self._cur], self._force, self._free, self._mol_ptr, self.memory, self._tol2, self._alpha,
                       self._maxstep, flags, self._converged, self._n_steps, self._n_pairs, self._head, self._S, self._Y, self._rho,
                       self._f_prev, self._work, self._pos[other], self._fmax, wg_min_atoms=self._wg_min_atoms)
        self._cur = other

    @property
    def n_pairs(self):
        return self._n_pairs.long()

    # ------------------------------------------------------------------------------------------
    # run (Stepper.run): L-BFGS steps of every molecule that has not converged; the check-only launch measures fmax at the
    # positions reached and marks what has converged there
    def _frame(self):
        return self._pos[self._cur].clone(), self._force.clone(), self._energy.clone(), self._n_pairs.long()

    def _result(self):
        return RelaxResult(self._pos[self._cur].clone(), self._energy.clone(), self._fmax.clone(), self._converged != 0,
                           self._n_steps.long())
