"""Batched dimer-method saddle search on the HIP path: the dimer of every molecule of a batch climbs to a first-order saddle on the
device, one force evaluation and one launch (nnhip_dimer_step, csrc/dimer.hip) per step, with no host round trip of positions or
forces.  It needs gradients only -- no Hessian, no second endpoint -- and serves two uses: refining the climbing image of a band
that stopped at its usual threshold (newtonnet_amd.neb) to a saddle good enough for normal modes and a reaction path, and a
single-ended search from a guessed transition geometry and a direction.

The method is min-mode following after Henkelman & Jonsson (J. Chem. Phys. 111, 7010 (1999)) with the one-evaluation rotations of
Heyden, Bell & Keil (J. Chem. Phys. 123, 224101 (2005)) and Kaestner & Sherwood (J. Chem. Phys. 128, 014106 (2008)): a dimer is a
centre x and a unit direction N; a ROTATION turns N towards the lowest curvature mode in the plane of N and a conjugate-gradient
direction, by the angle a two-term Fourier fit of the curvature gives from ONE trial evaluation, the rotated endpoint's force being
interpolated; a TRANSLATION moves the centre by an L-BFGS step (nnhip_lbfgs_step's recursion) on the force with its component along N
inverted -- while the curvature along N is not negative, by the plain step along -(F.N) N, and the history keeps pairs of steps
made with a negative curvature only.  Every evaluation of the batch is one model() call: each molecule is its own state machine, and what it has evaluated is
its centre, its endpoint or a trial endpoint (`phase` 0, 1, 2).  A molecule has converged (sticky) when, after at least one
translation, the largest force on a free atom of its centre is below fmax and the curvature along N is negative.  A converged molecule
is frozen bit for bit, but model() keeps evaluating it with the rest of the batch.  include/newtonnet_hip.h holds the contract of a
launch; DESIGN.md section 20 says what was left out.

Units: positions and dimer_length in Angstrom, forces and fmax in eV / Angstrom, curvature and alpha in eV / Angstrom^2,
rotation_tolerance in degrees."""
from __future__ import annotations

import math

import numpy as np
import torch

from newtonnet_amd import hip, stepper
from newtonnet_amd.dynamics import _mol_ptr, _molecule_sums
from newtonnet_amd.relax import check_arguments as check_lbfgs_arguments
from newtonnet_amd.relax import check_inputs
from newtonnet_amd.vibrations import _check_solver, lowest_mode_direction, table_masses

CENTER, ENDPOINT, TRIAL = 0, 1, 2          # what a molecule's probe is (the `phase` of the kernel's contract)


class SaddleResult:
    """What SaddleSearch.run returns, as device tensors:

    pos         fp32 [N,3]   the dimer centres;   mode fp32 [N,3]: the dimers' directions (unit per molecule, zero on fixed atoms)
    energy      fp32 [B]     the model's energy at pos;  fmax fp32 [B]: the largest force norm on a free atom at pos
    curvature   fp32 [B]     the curvature along mode, by the dimer's finite difference (the last rotation's estimate)
    converged   bool [B]     fmax below the threshold with a negative curvature after >= 1 translation (sticky)
    n_steps, n_evaluations, n_rotations   int64 [B]   translations, force evaluations consumed, rotations
    traj_*      only with record_every > 0, over the R recorded evaluations: traj_step int64 [R] (evaluations since the SaddleSearch
                was made), traj_pos fp32 [R,N,3] (the geometry evaluated: the probe), traj_force fp32 [R,N,3] and traj_energy fp32
                [R,B] (the model's results there, which the next launch consumed), traj_center, traj_mode fp32 [R,N,3],
                traj_phase int64 [R,B] (what each molecule's probe is: 0 centre, 1 endpoint, 2 trial endpoint), traj_curvature
                fp32 [R,B]
    """

    def __init__(self, pos, mode, energy, fmax, curvature, converged, n_steps, n_evaluations, n_rotations):
        self.pos, self.mode, self.energy, self.fmax, self.curvature = pos, mode, energy, fmax, curvature
        self.converged, self.n_steps, self.n_evaluations, self.n_rotations = converged, n_steps, n_evaluations, n_rotations
        self.traj_step = self.traj_pos = self.traj_force = self.traj_energy = self.traj_center = self.traj_mode = None
        self.traj_phase = self.traj_curvature = None


def check_arguments(fmax, dimer_length, rotation_tolerance, max_rotations, memory, maxstep, alpha):
    """the method's numbers, refused without touching the device; returns them as (float, float, float, int, int, float, float)"""
    fmax, memory, maxstep, alpha = check_lbfgs_arguments(fmax, memory, maxstep, alpha)
    dimer_length, rotation_tolerance = float(dimer_length), float(rotation_tolerance)
    if not (dimer_length > 0.0 and math.isfinite(dimer_length)):
        raise ValueError(f'dimer_length: a finite value > 0 Angstrom expected (got {dimer_length!r})')
    if not 0.0 < rotation_tolerance < 45.0:
        raise ValueError(f'rotation_tolerance: a value in (0, 45) degrees expected (got {rotation_tolerance!r})')
    if int(max_rotations) != max_rotations or max_rotations < 0:
        raise ValueError(f'max_rotations: an integer >= 0 expected (got {max_rotations!r})')
    return fmax, dimer_length, rotation_tolerance, int(max_rotations), memory, maxstep, alpha


def check_run_arguments(max_evaluations, check_every, record_every):
    return stepper.check_run_arguments(max_evaluations, check_every, record_every, 'max_evaluations')


class SaddleSearch(stepper.Stepper):
    """The dimers of B molecules, searching together on the device.

    model: a NewtonNet in eval mode with the 'energy' and 'gradient_force' heads.  z, pos, cell, batch: as for model(...), on the
    device, pos being the start geometries; none of them is modified.  direction: fp32 [N,3], the start direction of every
    molecule's dimer; it is zeroed on fixed atoms and normalised per molecule, and a molecule whose direction vanishes is refused.
    After a band the natural argument is BandResult.tangent at the rows of saddle_image, with pos the positions of that image.
    None: model.normal_modes(..., solver=solver) is called and every molecule's lowest mode taken, un-mass-weighted (standard atomic
    weights); the mode need not be imaginary.  fmax: the convergence threshold on the largest force norm of a free atom at the
    centre (compared as squares in fp32).  dimer_length: the distance delta from the centre to the endpoint.  rotation_tolerance: a
    rotation cycle ends when the predicted rotation angle falls below it, or after max_rotations rotations.  memory, maxstep,
    alpha: the translation's L-BFGS, as for Relaxation.  fixed: bool [N], atoms that never move.

    Not done: rigid translations and rotations are not projected out of the direction, so a search started in a convex region of a
    free molecule can lock onto a near-zero rigid mode (a refinement from a band image cannot); at an exact minimum the modified
    force vanishes -- displace the geometry first.

    Periodic molecules: the cell is fixed and positions stay unwrapped; the model's neighbor list takes the minimum image itself,
    the dimer's endpoints are plain Cartesian displacements."""
    NOUN, CHECK_ONLY = 'saddle searches', hip.DIMER_CHECK_ONLY
    TRAJ = (('pos', ('n_atoms', 3), torch.float32), ('force', ('n_atoms', 3), torch.float32), ('energy', ('n_mol',), torch.float32),
            ('center', ('n_atoms', 3), torch.float32), ('mode', ('n_atoms', 3), torch.float32), ('phase', ('n_mol',), torch.int64),
            ('curvature', ('n_mol',), torch.float32))

    def __init__(self, model, z, pos, cell, batch, direction=None, fmax=0.001, dimer_length=0.01, rotation_tolerance=5.0,
                 max_rotations=8, memory=16, maxstep=0.2, alpha=70.0, fixed=None, solver='lds'):
        # ---- everything that can be refused without touching the device
        N, B = check_inputs(model, 'SaddleSearch', z, pos, cell, batch, fixed)
        if direction is not None and (not isinstance(direction, torch.Tensor) or direction.dtype != torch.float32
                                      or tuple(direction.shape) != (N, 3)):
            raise ValueError(f'direction: a float32 tensor [{N},3] expected')
        fmax, dimer_length, rotation_tolerance, max_rotations, memory, maxstep, alpha = check_arguments(
            fmax, dimer_length, rotation_tolerance, max_rotations, memory, maxstep, alpha)
        solver = _check_solver(solver)
        dev = self._check_device(pos, z=z, cell=cell, batch=batch, fixed=fixed, direction=direction)
        # ---- state
        f32 = np.float32
        self.model, self.z, self.cell, self.batch = model, z, cell, batch
        self.n_atoms, self.n_mol = N, B
        self.fmax, self.memory, self.max_rotations = fmax, memory, max_rotations
        # the numbers the kernel gets, as the Python floats of their fp32 values
        self._tol2 = float(f32(fmax * fmax))
        self._delta = float(f32(dimer_length))
        self._rot_tol = float(f32(math.tan(2.0 * math.radians(rotation_tolerance))))
        self._maxstep, self._alpha = float(f32(maxstep)), float(f32(alpha))
        with torch.no_grad():
            free = torch.ones(N, dtype=torch.bool, device=dev) if fixed is None else ~fixed
            if direction is None:
                u, _ = lowest_mode_direction(model, z, pos, cell, batch, table_masses(z), solver)
            else:
                u = direction.detach().double()
            u = u * free[:, None]
            n2 = (u * u).sum(1).float()
            norm2 = _molecule_sums(torch.stack([n2, torch.zeros_like(n2)], 1), batch, B)[:, 0].double()     # (an even width)
            counts = torch.bincount(batch.long(), minlength=B)
            # the one host read of the construction: what only the device knows and must be refused
            if not bool((((norm2 > 0) & torch.isfinite(norm2)) | (counts == 0)).all()):
                raise ValueError('direction: a molecule has a direction that vanishes on its free atoms (or is not finite)')
            mode = (u / norm2.clamp_min(1e-300).sqrt()[batch.long()][:, None]).float()
            self._free = None if fixed is None else free.contiguous()
            self._init_buffers(pos.detach().clone().contiguous())     # (the probes; step_count counts evaluations consumed)
            self._mol_ptr = _mol_ptr(batch, B)
            self._istate = torch.zeros(hip.DIMER_N_INT, B, dtype=torch.int32, device=dev)
            self._active = self._istate[hip.DIMER_I['status']]
            self._fstate = torch.zeros(hip.DIMER_N_FLOAT, B, dtype=torch.float32, device=dev)
            self._vstate = torch.zeros(hip.DIMER_N_VEC, N, 3, dtype=torch.float32, device=dev)
            self._vstate[hip.DIMER_V['center']] = self._pos[0]
            self._vstate[hip.DIMER_V['mode']] = mode
            self._S = torch.zeros(memory, N, 3, dtype=torch.float32, device=dev)
            self._Y = torch.zeros(memory, N, 3, dtype=torch.float32, device=dev)
            self._rho = torch.zeros(B, memory, dtype=torch.float32, device=dev)
            self._work = torch.empty(N, 3, dtype=torch.float32, device=dev) if N > 64 else None
            self._fmax = torch.zeros(B, dtype=torch.float32, device=dev)
            self._e_center = torch.zeros(B, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------------------------------
    def _launch(self, flags=0):
        """one launch: reads the current probes and their forces, writes the next probes into the other buffer, the buffers swap"""
        other = 1 - self._cur
        hip.dimer_step(self._pos[self._cur], self._force, self._energy.reshape(-1), self._free, self._mol_ptr, self.memory,
                       self._delta, self._rot_tol, self.max_rotations, self._tol2, self._alpha, self._maxstep, flags, self._istate,
                       self._fstate, self._vstate, self._S, self._Y, self._rho, self._work, self._pos[other], self._fmax,
                       self._e_center)
        self._cur = other

    def _int(self, name):
        return self._istate[hip.DIMER_I[name]].long()

    @property
    def positions(self):
        """the dimer centres"""
        return self._vstate[hip.DIMER_V['center']].clone()

    @property
    def mode(self):
        return self._vstate[hip.DIMER_V['mode']].clone()

    @property
    def curvature(self):
        return self._fstate[hip.DIMER_F['curvature']].clone()

    @property
    def n_steps(self):
        return self._int('steps')

    @property
    def n_evaluations(self):
        return self._int('evals')

    @property
    def n_rotations(self):
        return self._int('rot_total')

    # ------------------------------------------------------------------------------------------
    def run(self, max_evaluations: int, check_every: int = 10, record_every: int = 0) -> SaddleResult:
        """Stepper.run with a step being one force evaluation (launch): up to max_evaluations of every molecule that has not
        converged, then the result at the centres reached; check_every and record_every count evaluations.  The check-only launch
        measures fmax and the energy of every molecule whose probe is its centre, sets no flag and moves nothing."""
        return self._run(*check_run_arguments(max_evaluations, check_every, record_every))

    def _frame(self):
        return (self._pos[self._cur].clone(), self._force.clone(), self._energy.reshape(-1).clone(), self.positions, self.mode,
                self._int('phase'), self.curvature)

    def _result(self):
        return SaddleResult(self.positions, self.mode, self._e_center.clone(), self._fmax.clone(), self.curvature,
                            self._active != 0, self.n_steps, self.n_evaluations, self.n_rotations)
