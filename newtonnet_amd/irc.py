"""Batched intrinsic-reaction-coordinate (IRC) following on the HIP path: from the saddle of every molecule of a batch the steepest-
descent path in mass-weighted coordinates is followed down both sides on the device, one force evaluation and one launch
(nnhip_irc_step, csrc/irc.hip) per step, with no host round trip of positions or forces.

The method is damped velocity Verlet (after Hratchian & Schlegel, J. Phys. Chem. A 106, 165 (2002)): a trajectory whose speed is
reset to the constant `speed` after every step, so that it moves along M^-1 F; the time step of every path follows an error
estimate (`error_target`) that needs no further force evaluation.  A path stops (sticky `status`) when the largest force on a free
atom falls below `fmax` after having been above it (1: minimum reached) or when the force turns against the velocity (2: the last
step passed the minimum along the path).  A stopped path is frozen bit for bit, but model() keeps evaluating it with the rest of the
batch.  include/newtonnet_hip.h holds the contract of a step; DESIGN.md section 19 says what was left out.

Units: positions in Angstrom, time in fs, speed in Angstrom / fs, arc lengths in amu^1/2 Angstrom, forces and fmax in eV / Angstrom."""
from __future__ import annotations

import math

import numpy as np
import torch

from newtonnet_amd import hip
from newtonnet_amd.dynamics import _mol_ptr, _molecule_sums
from newtonnet_amd.relax import check_inputs
from newtonnet_amd.stepper import Stepper, check_run_arguments
from newtonnet_amd.vibrations import lowest_mode_direction, table_masses

RUNNING, MINIMUM, TURNED = 0, 1, 2


class PathResult:
    """What ReactionPath.run returns, as device tensors (P paths: 2 per molecule with both=True, path 2b forward, 2b + 1 backward):

    pos         fp32 [N',3]  positions after the last step;   energy fp32 [P]: the model's energy there
    fmax        fp32 [P]     the largest force norm on a free atom at pos
    status      int64 [P]    0 running, 1 minimum reached, 2 turned;   n_steps int64 [P]: steps taken
    arc_length  fp32 [P]     mass-weighted length of the path from the saddle (it starts at initial_displacement)
    traj_*      only with record_every > 0, over the R recorded steps: traj_step int64 [R] (steps since the ReactionPath was made),
                traj_pos, traj_force, traj_vel fp32 [R,N',3] (the forces are the ones the next launch consumed at those positions,
                the velocities the damped ones that brought the path there), traj_energy, traj_arc, traj_dt fp32 [R,P] (traj_dt:
                the time step the NEXT step takes), traj_status int64 [R,P]
    """

    def __init__(self, pos, energy, fmax, status, n_steps, arc_length, both, mol_ptr, saddle, first):
        self.pos, self.energy, self.fmax, self.status, self.n_steps, self.arc_length = pos, energy, fmax, status, n_steps, arc_length
        self.traj_step = self.traj_pos = self.traj_force = self.traj_vel = self.traj_energy = self.traj_arc = self.traj_dt = None
        self.traj_status = None
        self._both, self._mol_ptr, self._saddle, self._first = both, mol_ptr, saddle, first

    def _branch(self, p):
        """(arc [K], energy [K], pos [K,n,3]) of path p in path order: the start of the run when it was the path's start, the
        recorded frames in which the path moved, and the end point"""
        a0, a1 = self._mol_ptr[p], self._mol_ptr[p + 1]
        arc, energy, pos = [], [], []
        if self._first is not None:
            arc.append(self._first[2][p:p + 1]), energy.append(self._first[1][p:p + 1]), pos.append(self._first[0][a0:a1][None])
        if self.traj_step is not None and self.traj_step.numel():
            arc.append(self.traj_arc[:, p]), energy.append(self.traj_energy[:, p]), pos.append(self.traj_pos[:, a0:a1])
        arc.append(self.arc_length[p:p + 1]), energy.append(self.energy[p:p + 1]), pos.append(self.pos[a0:a1][None])
        arc, energy, pos = torch.cat(arc), torch.cat(energy), torch.cat(pos)
        keep = torch.ones_like(arc, dtype=torch.bool)
        keep[1:] = arc[1:] != arc[:-1]                    # a frame without progress repeats the one before (a stopped path)
        return arc[keep], energy[keep], pos[keep]

    def profile(self, b: int):
        """The energy profile through saddle b: (arc, energy, pos) with the backward branch reversed (arc counted negative), then
        the saddle (arc 0), then the forward branch -- arc fp32 [K] from -s_back to +s_fwd, energy fp32 [K], pos fp32 [K,n,3].
        Holds the end points alone unless the run recorded frames.  It covers THIS run: the frames it recorded, its end points and,
        when the run was the first of its ReactionPath, the start points; a later run() knows neither the start nor the frames of
        the runs before it.  A frame whose arc length equals the one before it is left out: that drops the repeats of a stopped
        path, and also a running path's step of zero length (the |v| = 0 case).  Needs both=True."""
        if not self._both:
            raise ValueError('profile needs a ReactionPath made with both=True')
        s_pos, s_energy = self._saddle
        fa, fe, fp = self._branch(2 * b)
        ba, be, bp = self._branch(2 * b + 1)
        a0, a1 = self._mol_ptr[2 * b] // 2, self._mol_ptr[2 * b + 1] - self._mol_ptr[2 * b] + self._mol_ptr[2 * b] // 2
        zero = torch.zeros(1, dtype=fa.dtype, device=fa.device)
        return (torch.cat([-ba.flip(0), zero, fa]), torch.cat([be.flip(0), s_energy[b:b + 1], fe]),
                torch.cat([bp.flip(0), s_pos[a0:a1][None], fp]))


def check_arguments(speed, error_target, timestep, timestep_min, timestep_max, initial_displacement, fmax):
    """the method's numbers, refused without touching the device; returns them as floats"""
    vals = []
    for name, v, unit in (('speed', speed, 'Angstrom/fs'), ('error_target', error_target, 'Angstrom'), ('timestep', timestep, 'fs'),
                          ('timestep_min', timestep_min, 'fs'), ('timestep_max', timestep_max, 'fs'),
                          ('initial_displacement', initial_displacement, 'amu^1/2 Angstrom'), ('fmax', fmax, 'eV/Angstrom')):
        v = float(v)
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError(f'{name}: a finite value > 0 {unit} expected (got {v!r})')
        vals.append(v)
    if not vals[3] <= vals[2] <= vals[4]:
        raise ValueError(f'timestep_min <= timestep <= timestep_max expected (got {vals[3]!r}, {vals[2]!r}, {vals[4]!r})')
    return tuple(vals)


class ReactionPath(Stepper):
    """The IRC paths from the saddles of B molecules, followed together on the device.

    model: a NewtonNet in eval mode with the 'energy' and 'gradient_force' heads.  z, pos, cell, batch: as for model(...), on the
    device, pos being the saddle geometries; none of them is modified.  direction: fp32 [N,3], the Cartesian direction to leave
    each saddle along, or None: model.normal_modes is called and every molecule's lowest mode taken (ValueError for a molecule
    without an imaginary mode).  The direction is zeroed on fixed atoms and its sign fixed so that its component of largest
    magnitude (the lowest index at a tie) is positive: "forward" is reproducible.  both=True doubles the batch: path 2b runs
    forward and 2b + 1 backward; both=False follows the forward branch alone.  A path starts at x_saddle +- initial_displacement u /
    |M^1/2 u| with the velocity +- speed u / |u| and the arc length initial_displacement.  speed, error_target: the method's
    constant speed and the target of its per-step error estimate (Hratchian & Schlegel's 0.04 bohr / fs and 0.003 bohr);
    timestep: the first time step, kept inside [timestep_min, timestep_max].  fmax: a path has reached a minimum when the largest
    force norm on a free atom is below it (compared as squares in fp32) after having been above it.  fixed: bool [N], atoms that
    never move.  masses: fp32 [N] amu (None: standard atomic weights of z).

    Periodic molecules: the cell is fixed and positions stay unwrapped; the model's neighbor list takes the minimum image itself."""
    NOUN, CHECK_ONLY = 'reaction paths', hip.IRC_CHECK_ONLY
    TRAJ = (('pos', ('n_atoms', 3), torch.float32), ('force', ('n_atoms', 3), torch.float32), ('vel', ('n_atoms', 3), torch.float32),
            ('energy', ('n_mol',), torch.float32), ('arc', ('n_mol',), torch.float32), ('dt', ('n_mol',), torch.float32),
            ('status', ('n_mol',), torch.int64))

    def __init__(self, model, z, pos, cell, batch, direction=None, masses=None, both=True, speed=0.02, error_target=1.5e-3,
                 timestep=0.25, timestep_min=0.01, timestep_max=2.0, initial_displacement=0.1, fmax=0.01, fixed=None):
        # ---- everything that can be refused without touching the device
        N, B = check_inputs(model, 'ReactionPath', z, pos, cell, batch, fixed)
        if direction is not None and (not isinstance(direction, torch.Tensor) or direction.dtype != torch.float32
                                      or tuple(direction.shape) != (N, 3)):
            raise ValueError(f'direction: a float32 tensor [{N},3] expected')
        if masses is not None and (not isinstance(masses, torch.Tensor) or masses.numel() != N):
            raise ValueError(f'masses: a tensor of {N} values expected')
        speed, error_target, timestep, timestep_min, timestep_max, initial_displacement, fmax = check_arguments(
            speed, error_target, timestep, timestep_min, timestep_max, initial_displacement, fmax)
        dev = self._check_device(pos, z=z, cell=cell, batch=batch, fixed=fixed, direction=direction, masses=masses)
        # ---- state
        f32 = np.float32
        self.model, self.both, self.fmax = model, bool(both), fmax
        self.initial_displacement = initial_displacement
        # the numbers the kernel gets, as the Python floats of their fp32 values
        self._v0, self._delta0 = float(f32(speed)), float(f32(error_target))
        self._dt_min, self._dt_max = float(f32(timestep_min)), float(f32(timestep_max))
        self._tol2 = float(f32(fmax * fmax))
        with torch.no_grad():
            m = table_masses(z) if masses is None else masses.detach().float().reshape(-1).clone()
            free = torch.ones(N, dtype=torch.bool, device=dev) if fixed is None else ~fixed
            imaginary = torch.ones(B, dtype=torch.bool, device=dev)
            if direction is None:
                u, n_imaginary = lowest_mode_direction(model, z, pos, cell, batch, m, 'auto')
                imaginary = n_imaginary > 0
            else:
                u = direction.detach().double()
            u = u * free[:, None]
            # the sign: the component of largest magnitude of every molecule, the lowest index at a tie, is positive
            flat, owner = u.reshape(-1), batch.long().repeat_interleave(3)
            big = torch.zeros(B, dtype=torch.float64, device=dev).scatter_reduce(0, owner, flat.abs(), 'amax', include_self=True)
            index = torch.arange(3 * N, device=dev)
            first = torch.full((B,), 3 * N, dtype=torch.int64, device=dev).scatter_reduce(
                0, owner, torch.where(flat.abs() == big[owner], index, 3 * N), 'amin', include_self=True)
            sign = torch.where(flat[first.clamp(max=max(3 * N - 1, 0))] < 0, -1.0, 1.0) if N else torch.ones(B, device=dev)
            u = u * sign.double()[batch.long()][:, None]
            sums = _molecule_sums(torch.stack([(m.double()[:, None] * u * u).sum(1), (u * u).sum(1)], 1).float(), batch, B).double()
            norms_ok = (sums > 0).all(1) & torch.isfinite(sums).all(1)
            counts = torch.bincount(batch.long(), minlength=B)
            # the one host read of the construction: what only the device knows and must be refused
            word = torch.stack([imaginary.all(), (norms_ok | (counts == 0)).all(),
                                (torch.isfinite(m) & (m > 0) | ~free).all()]).tolist()
            if not word[2]:
                raise ValueError('masses: positive finite values expected')
            if not word[0]:
                bad = (~imaginary).nonzero().reshape(-1).tolist()
                raise ValueError(f'direction=None: molecules {bad} have no imaginary mode (not a saddle); pass a direction')
            if not word[1]:
                raise ValueError('direction: a molecule has a direction that vanishes on its free atoms (or is not finite)')
            mw, eu = sums[:, 0].sqrt()[batch.long()][:, None], sums[:, 1].sqrt()[batch.long()][:, None]
            step0, vel0 = initial_displacement * u / mw, speed * u / eu
            self._saddle_inputs = (z, pos.detach().clone(), cell, batch)
            self._saddle_energy = None
            if self.both:
                P = 2 * B
                new_counts = counts.repeat_interleave(2, output_size=P)
                new_ptr = torch.zeros(P + 1, dtype=torch.int64, device=dev)
                new_ptr[1:] = torch.cumsum(new_counts, 0)
                new_batch = torch.arange(P, device=dev).repeat_interleave(new_counts, output_size=2 * N)
                old_ptr = _mol_ptr(batch, B).long()
                src = old_ptr[new_batch // 2] + torch.arange(2 * N, device=dev) - new_ptr[new_batch]
                way = torch.where(new_batch % 2 == 0, 1.0, -1.0).double()[:, None]
                self.z, self.cell, self.batch = z[src].contiguous(), cell.repeat_interleave(2, dim=0, output_size=P).contiguous(), \
                    new_batch.to(batch.dtype)
                start = pos.detach().double()[src] + way * step0[src]
                vel = way * vel0[src]
                m, free = m[src], free[src]
            else:
                P = B
                self.z, self.cell, self.batch = z, cell, batch
                start, vel = pos.detach().double() + step0, vel0
            Np = start.shape[0]
            self.n_atoms, self.n_mol = Np, P
            self.masses = m.contiguous()
            self._free = None if fixed is None else free.contiguous()
            self._init_buffers(start.float().contiguous())
            self._mol_ptr = _mol_ptr(self.batch, P)
            self._mol_ptr_host = None

            def ints():
                return torch.zeros(P, dtype=torch.int32, device=dev)
            self._status, self._armed, self._n_steps = ints(), ints(), ints()
            self._active = self._status
            self._dt = torch.full((P,), float(f32(timestep)), dtype=torch.float32, device=dev)
            self._dt_prev = torch.zeros(P, dtype=torch.float32, device=dev)
            self._arc = torch.full((P,), float(f32(initial_displacement)), dtype=torch.float32, device=dev)
            self._vel = vel.float().contiguous()
            self._x_prev, self._v_prev, self._a_prev = (torch.zeros(Np, 3, dtype=torch.float32, device=dev) for _ in range(3))
            self._fmax = torch.zeros(P, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------------------------------
    def _launch(self, flags=0):
        """one launch: reads the current buffer and the current forces, writes the other buffer, and the buffers swap"""
        other = 1 - self._cur
        hip.irc_step(self._pos[self._cur], self._force, self._free, self.masses, self._mol_ptr, self._v0, self._delta0, self._dt_min,
                     self._dt_max, self._tol2, flags, self._status, self._armed, self._n_steps, self._dt, self._dt_prev, self._arc,
                     self._vel, self._x_prev, self._v_prev, self._a_prev, self._pos[other], self._fmax)
        self._cur = other

    def _ensure_state(self):
        if self._saddle_energy is None:
            with torch.no_grad():
                z, pos, cell, batch = self._saddle_inputs
                out = self.model(z, pos, cell, batch)
                out.gradient_force                        # (settles the deferred record of the call, as _evaluate says)
                self._saddle_energy = out.energy.clone()
        super()._ensure_state()

    @property
    def velocities(self):
        return self._vel.clone()

    @property
    def status(self):
        return self._status.long()

    @property
    def arc_length(self):
        return self._arc.clone()

    @property
    def timestep(self):
        return self._dt.clone()

    # ------------------------------------------------------------------------------------------
    def run(self, max_steps: int, check_every: int = 10, record_every: int = 1) -> PathResult:
        """Stepper.run, recording every step unless told otherwise: steps of every path that has not stopped, then the result at
        the positions reached.  The check-only launch measures fmax there and moves nothing."""
        return self._run(*check_run_arguments(max_steps, check_every, record_every))

    def _begin(self):
        self._first = None
        if self.step_count == 0:
            self._first = (self._pos[self._cur].clone(), self._energy.clone(), self._arc.clone())

    def _frame(self):
        return (self._pos[self._cur].clone(), self._force.clone(), self._vel.clone(), self._energy.clone(), self._arc.clone(),
                self._dt.clone(), self._status.long())

    def _result(self):
        if self._mol_ptr_host is None:
            self._mol_ptr_host = self._mol_ptr.tolist()
        return PathResult(self._pos[self._cur].clone(), self._energy.clone(), self._fmax.clone(), self._status.long(),
                          self._n_steps.long(), self._arc.clone(), self.both, self._mol_ptr_host,
                          (self._saddle_inputs[1].detach(), self._saddle_energy), self._first)
