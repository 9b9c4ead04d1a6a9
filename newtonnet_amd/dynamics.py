"""Batched molecular dynamics on the HIP path: every molecule of a batch is integrated on the device, one force evaluation and one
integrator launch (nnhip_md_step, csrc/md.hip) per step, with no host round trip of positions or forces.

The reference leaves dynamics to an outside driver that calls its calculator once per step for one structure.
Here `Dynamics` owns positions, velocities and forces of B molecules as device tensors and advances them together: microcanonical
(velocity Verlet) with friction = 0, Langevin in the BAOAB splitting (Leimkuhler & Matthews 2013, the O step exact) otherwise.

Units: positions in Angstrom, energies in eV, masses in amu, hence time in Angstrom sqrt(amu / eV) = 10.18 fs; `timestep` is given in
fs and `friction` in 1 / fs (FS converts), temperatures in K, velocities in Angstrom per internal time unit.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from newtonnet_amd import hip
from newtonnet_amd.vibrations import K_BOLTZMANN, _AMU, _E_CHARGE, table_masses

# one femtosecond in the internal time unit Angstrom sqrt(amu / eV): 1e-15 s x sqrt(e / (1e-20 amu)) s^-1 = 0.0982269
FS = 1e-15 * math.sqrt(_E_CHARGE / (1e-20 * _AMU))


def _per_atom_temperature(temperature, batch: torch.Tensor, n_mol: Optional[int] = None) -> torch.Tensor:
    """fp64 [N]: the temperature of every atom's molecule; `temperature` is a number or a [B] tensor (a ladder)"""
    if isinstance(temperature, torch.Tensor) and temperature.dim() > 0:
        T = temperature.detach().to(device=batch.device, dtype=torch.float64).reshape(-1)
        if n_mol is not None and T.numel() != n_mol:
            raise ValueError(f'temperature: a number or one value per molecule ({n_mol}) expected (got {T.numel()})')
        return T[batch.long()]
    return torch.full((batch.numel(),), float(temperature), dtype=torch.float64, device=batch.device)


def _check_temperature(temperature, n_mol: int):
    if temperature is None:
        return
    if isinstance(temperature, torch.Tensor) and temperature.dim() > 0:
        if temperature.numel() != n_mol:
            raise ValueError(f'temperature: a number or one value per molecule ({n_mol}) expected (got {temperature.numel()})')
        return        # (its values live on the device: a negative one gives NaN velocities, not an exception)
    T = float(temperature)
    if not (T >= 0.0 and math.isfinite(T)):
        raise ValueError(f'temperature: a finite value >= 0 K expected (got {temperature!r})')


def langevin_coefficients(timestep_fs: float, friction_per_fs: float, temperature, masses: torch.Tensor, batch: torch.Tensor):
    """(c1, sigma [N] fp32) of the exact Ornstein-Uhlenbeck step v <- c1 v + sigma xi over one time step:
    c1 = exp(-gamma dt), sigma_i = sqrt((1 - c1^2) k_B T_{batch[i]} / m_i).  Computed in fp64 and rounded once to fp32 (c1 comes back
    as the Python float of its fp32 value).  temperature: a number, or a [B] tensor -- one temperature per molecule."""
    gdt = float(friction_per_fs) * float(timestep_fs)
    if not (gdt >= 0.0 and math.isfinite(gdt)):
        raise ValueError(f'friction x timestep: a finite value >= 0 expected (got {gdt!r})')
    c1 = math.exp(-gdt)
    one_minus_c1sq = -math.expm1(-2.0 * gdt)
    T = _per_atom_temperature(temperature, batch)
    sigma = torch.sqrt(one_minus_c1sq * K_BOLTZMANN * T / masses.detach().double().reshape(-1))
    return float(np.float32(c1)), sigma.float()


def _mol_ptr(batch: torch.Tensor, n_mol: int) -> torch.Tensor:
    """int32 [B+1] atom offsets of a sorted batch vector"""
    ptr = torch.zeros(n_mol + 1, dtype=torch.int32, device=batch.device)
    if batch.numel():
        ptr[1:] = torch.cumsum(torch.bincount(batch.long(), minlength=n_mol), 0).to(torch.int32)
    return ptr


def _molecule_sums(x: torch.Tensor, batch: torch.Tensor, n_mol: int) -> torch.Tensor:
    """[B, W] sums of the rows x [N, W] (W even) per molecule: the library's deterministic segment sum on the device"""
    if x.is_cuda:
        return hip.segment_sum(x.contiguous(), _mol_ptr(batch, n_mol), n_mol)
    return torch.zeros(n_mol, x.shape[1], dtype=x.dtype).index_add_(0, batch.long(), x)


def maxwell_boltzmann(masses: torch.Tensor, batch: torch.Tensor, temperature, generator: Optional[torch.Generator] = None,
                      n_mol: Optional[int] = None) -> torch.Tensor:
    """Velocities fp32 [N,3] drawn from the Maxwell-Boltzmann distribution at `temperature` (a number or a [B] ladder) with exactly
    one torch.randn((N, 3)) call on the device of `masses`, then each molecule's centre-of-mass momentum removed."""
    m = masses.detach().float().reshape(-1)
    n_mol = int(batch.max()) + 1 if n_mol is None else int(n_mol)
    xi = torch.randn((m.numel(), 3), generator=generator, device=m.device, dtype=torch.float32)
    T = _per_atom_temperature(temperature, batch, n_mol)
    v = xi * torch.sqrt(K_BOLTZMANN * T / m.double()).float()[:, None]
    s = _molecule_sums(torch.cat([m[:, None] * v, m[:, None]], dim=1), batch, n_mol)       # [B, 4]: momentum, mass
    return v - (s[:, :3] / s[:, 3:].clamp(min=1e-30))[batch.long()]


class Trajectory:
    """What Dynamics.run recorded, as device tensors:

    step              int64 [R]      step numbers since the Dynamics was made
    pos, vel          fp32 [R,N,3]   positions (unwrapped) and full-step velocities
    potential_energy  fp32 [R,B]     the model's energy at pos
    kinetic_energy    fp32 [R,B]     sum of m v^2 / 2 per molecule
    total_energy      fp32 [R,B]     their sum;  temperature fp32 [R,B] = 2 KE / (3 n_b k_B)
                                     (a run with C_b constrained bond lengths in molecule b: 2 KE / ((3 n_b - C_b) k_B))
    """

    _dof = None          # fp32 [B] degrees of freedom 3 n_b - C_b of a constrained run (Dynamics sets it); None: 3 n_b

    def __init__(self, step, pos, vel, potential_energy, kinetic_energy, counts):
        self.step, self.pos, self.vel = step, pos, vel
        self.potential_energy, self.kinetic_energy, self._counts = potential_energy, kinetic_energy, counts

    @property
    def total_energy(self):
        return self.potential_energy + self.kinetic_energy

    @property
    def temperature(self):
        if self._dof is not None:
            return 2.0 * self.kinetic_energy / (K_BOLTZMANN * self._dof.clamp(min=1).float())
        return 2.0 * self.kinetic_energy / (3.0 * K_BOLTZMANN * self._counts.clamp(min=1).float())

    # ---- observables (newtonnet_amd/observables.py): the frames stay on the device
    _system = None       # (z, batch, cell, masses, timestep) of the run: Dynamics attaches it

    def _observed(self):
        if self._system is None:
            raise AttributeError('this trajectory does not know its system: use newtonnet_amd.observables with z and batch')
        return self._system

    def _frame_cells(self):
        """the cells of the frames: [B,3,3] here (they do not change); NPTTrajectory holds one set per frame"""
        return self._observed()[2]

    def _frame_spacing(self) -> float:
        """fs between two recorded frames; ValueError unless the records are evenly spaced (one host read of `step`)"""
        step = self.step.cpu()
        d = step[1:] - step[:-1]
        if d.numel() and not bool((d == d[0]).all()):
            raise ValueError(f'the recorded steps {step.tolist()[:4]} ... {step.tolist()[-2:]} are not evenly spaced (the last record '
                             f'is the final step): choose n_steps a multiple of record_every')
        return self._observed()[4] * (int(d[0]) if d.numel() else 1)

    def radial_distribution(self, r_max, n_bins, species=None):
        """observables.RadialDistribution of every recorded frame (under the cell of its own frame), counted on the device"""
        from newtonnet_amd import observables
        z, batch = self._observed()[:2]
        return observables.RadialDistribution(z, batch, r_max, n_bins, species=species).add(self.pos, self._frame_cells())

    def mean_squared_displacement(self, max_lag, origin_every=1, species=None):
        """observables.MSD of the recorded (unwrapped) positions; the records must be evenly spaced"""
        from newtonnet_amd import observables
        z, batch, cell = self._observed()[:3]
        return observables.mean_squared_displacement(self.pos, z, batch, self._frame_spacing(), max_lag, origin_every=origin_every,
                                                     species=species, n_mol=cell.shape[0])

    def velocity_autocorrelation(self, max_lag, mass_weighted=False, origin_every=1, species=None):
        """observables.VACF of the recorded velocities (mass_weighted: with the run's masses); the records must be evenly spaced"""
        from newtonnet_amd import observables
        z, batch, cell, masses = self._observed()[:4]
        return observables.velocity_autocorrelation(self.vel, z, batch, self._frame_spacing(), max_lag,
                                                    masses=masses if mass_weighted else None, origin_every=origin_every,
                                                    species=species, n_mol=cell.shape[0])


def _check_system(model, z, pos, cell, batch, masses, velocities, fixed, timestep, friction):
    """the model, the batch and the integrator's numbers, refused without touching the device; returns (N, B, timestep, friction)"""
    if getattr(model, 'training', False):
        raise ValueError('Dynamics needs the model in eval mode: call model.eval()')
    props = list(getattr(model, 'output_properties', []))
    if 'energy' not in props or 'gradient_force' not in props:
        raise ValueError(f"Dynamics needs a model with the 'energy' and 'gradient_force' heads (it has {props})")
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
    if masses is not None and (not isinstance(masses, torch.Tensor) or masses.numel() != N):
        raise ValueError(f'masses: a tensor of {N} values expected')
    if velocities is not None and (not isinstance(velocities, torch.Tensor) or tuple(velocities.shape) != (N, 3)):
        raise ValueError(f'velocities: a tensor [{N},3] expected')
    if fixed is not None and (not isinstance(fixed, torch.Tensor) or fixed.dtype != torch.bool or tuple(fixed.shape) != (N,)):
        raise ValueError(f'fixed: a bool tensor [{N}] expected')
    timestep, friction = float(timestep), float(friction)
    if not (timestep > 0.0 and math.isfinite(timestep)):
        raise ValueError(f'timestep: a finite value > 0 fs expected (got {timestep!r})')
    if not (friction >= 0.0 and math.isfinite(friction)):
        raise ValueError(f'friction: a finite value >= 0 per fs expected (got {friction!r})')
    return N, B, timestep, friction


def _check_devices(pos, generator, **tensors):
    """everything lives on the device of pos, which is a ROCm device; returns it"""
    if not pos.is_cuda:
        raise RuntimeError('newtonnet_amd dynamics run on an MI355X (ROCm) device only: move the model and the inputs to "cuda"')
    dev = pos.device
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.dim() > 0 and t.device != dev:
            raise ValueError(f'{name} is on {t.device}, pos on {dev}')
    if generator is not None and torch.device(generator.device).type != dev.type:
        raise ValueError(f'generator is on {generator.device}, pos on {dev}')
    return dev


def _check_constraint_arguments(constraints, tolerance, max_iter, dev):
    """the form of the `constraints` argument (the pairs themselves are checked by constraints.prepare)"""
    if constraints is None:
        return
    if not (float(tolerance) > 0.0 and math.isfinite(float(tolerance))):
        raise ValueError(f'constraint_tolerance: a finite value > 0 expected (got {tolerance!r})')
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f'constraint_max_iter: an integer >= 1 expected (got {max_iter!r})')
    if isinstance(constraints, str):
        if constraints != 'h-bonds':
            raise ValueError(f"constraints: (pairs, lengths), 'h-bonds' or None expected (got {constraints!r})")
        return
    if not isinstance(constraints, (tuple, list)) or len(constraints) != 2:
        raise ValueError(f"constraints: (pairs, lengths), 'h-bonds' or None expected (got {type(constraints).__name__})")
    pairs, lengths = constraints
    if not isinstance(pairs, torch.Tensor) or pairs.dtype != torch.int64 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError('constraints: pairs, an int64 tensor [C,2] of atom indices, expected')
    if lengths is not None and (not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.float32
                                or tuple(lengths.shape) != (pairs.shape[0],)):
        raise ValueError(f'constraints: lengths, a float32 tensor [{pairs.shape[0]}] or None, expected')
    for name, t in (('pairs', pairs), ('lengths', lengths)):
        if t is not None and t.device.type != 'cpu' and t.device != dev:
            raise ValueError(f'constraints: {name} is on {t.device}, pos on {dev}')


class Dynamics:
    """B molecules advanced together on the device.

    model: a NewtonNet in eval mode with the 'energy' and 'gradient_force' heads.  z, pos, cell, batch: as for model(...), on the
    device; none of them is modified (the positions are copied).  masses: fp32 [N] amu (None: standard atomic weights of z).
    timestep in fs, friction in 1 / fs: 0 = microcanonical (velocity Verlet; no random numbers are drawn), > 0 = Langevin at
    `temperature` (K; a number or a [B] tensor, one temperature per molecule).  velocities: fp32 [N,3] in Angstrom per internal time
    unit (None: Maxwell-Boltzmann at `temperature` when one is given, else zero).  fixed: bool [N], atoms that never move.
    generator: a generator of the device for the initial velocities and the noise (None: torch's global one).

    constraints: None, or bond lengths kept by SHAKE / RATTLE inside the step's one launch (nnhip_md_step_constrained,
    csrc/rattle.hip; constrained BAOAB): (pairs int64 [C,2] of global atom indices, lengths fp32 [C] in
    Angstrom or None = the present distances), on the host or on the device of pos, or the string 'h-bonds' (hydrogen_constraints).
    Construction imposes the lengths on the initial positions and makes the initial velocities tangent (for a Maxwell-Boltzmann
    draw that gives the constrained distribution), and raises ValueError when that fails.  constraint_tolerance: relative, on
    d^2 (| |r|^2 - d^2 | <= tol d^2 in the solver's molecule-relative fp32 coordinates); constraint_max_iter: sweeps per solve.
    A molecule with constraints has at most hip.MDC_MAX_ATOMS atoms.  Distances are taken on the positions as stored (no minimum
    image): a constrained bond must not straddle a periodic boundary in the input.

    Periodic molecules: positions stay unwrapped; the model's neighbor list takes the minimum image of every pair itself."""

    _con = _dof = None       # no constraints (a subclass that builds its own state never sets them)

    def __init__(self, model, z, pos, cell, batch, masses=None, velocities=None, temperature=None, friction=0.0, timestep=0.5,
                 fixed=None, generator=None, constraints=None, constraint_tolerance=1e-5, constraint_max_iter=150):
        # ---- everything that can be refused without touching the device
        N, B, timestep, friction = _check_system(model, z, pos, cell, batch, masses, velocities, fixed, timestep, friction)
        _check_temperature(temperature, B)
        if friction > 0.0 and temperature is None:
            raise ValueError('friction > 0 (Langevin dynamics) needs a temperature')
        dev = _check_devices(pos, generator, z=z, cell=cell, batch=batch, masses=masses, velocities=velocities, fixed=fixed,
                             temperature=temperature)
        _check_constraint_arguments(constraints, constraint_tolerance, constraint_max_iter, dev)
        # ---- state
        self.model, self.z, self.cell, self.batch = model, z, cell, batch
        self.n_atoms, self.n_mol = N, B
        self.timestep, self.friction, self.temperature, self.generator = timestep, friction, temperature, generator
        self.step_count = 0
        with torch.no_grad():
            m = table_masses(z) if masses is None else masses.detach().float().reshape(-1).clone()
            if N and not bool(((m > 0) & torch.isfinite(m)).all()):
                raise ValueError('masses: positive finite values expected')
            self.masses = m.contiguous()
            dt = timestep * FS
            self._dth = float(np.float32(0.5 * dt))
            free = None if fixed is None else ~fixed
            hk = (0.5 * dt) / m.double()
            self._hk = (hk if free is None else hk * free).float().contiguous()
            self._c1, self._sigma = 1.0, None
            if friction > 0.0:
                self._c1, sigma = langevin_coefficients(timestep, friction, temperature, m, batch)
                self._sigma = (sigma if free is None else sigma * free).contiguous()
            if velocities is not None:
                vel = velocities.detach().float().clone()
            elif temperature is not None:
                vel = maxwell_boltzmann(m, batch, temperature, generator, n_mol=B)
            else:
                vel = torch.zeros(N, 3, dtype=torch.float32, device=dev)
            self._vel = (vel if free is None else vel * free[:, None]).contiguous()
            # two position buffers: a step reads one and writes the other, so the forward call queued on the one it read can still
            # be repeated from it (NewtonNet._forward_deferred)
            self._pos = [pos.detach().clone().contiguous(), torch.empty(N, 3, dtype=torch.float32, device=dev)]
            self._cur = 0
            self._mol_ptr = _mol_ptr(batch, B)
            self._counts = (self._mol_ptr[1:] - self._mol_ptr[:-1]).long()
            self._ke_atom = torch.zeros(N, dtype=torch.float32, device=dev)
            self._ke = torch.zeros(B, dtype=torch.float32, device=dev)
            self._force = self._energy = None
            self._con = self._dof = None
            if constraints is not None:
                self._init_constraints(constraints, float(constraint_tolerance), int(constraint_max_iter), free)

    def _init_constraints(self, constraints, tol, max_iter, free):
        """check, colour and upload the constraints, then impose them on the initial state with one NNHIP_MDC_PROJECT launch"""
        from newtonnet_amd import constraints as _c
        dev, N, B = self._vel.device, self.n_atoms, self.n_mol
        pos0 = self._pos[0]
        if isinstance(constraints, str):
            pairs, lengths = _c.hydrogen_constraints(self.z, pos0, self.batch)[0], None       # (the present distances, in fp64)
        else:
            pairs, lengths = constraints
        prep = _c.prepare(pairs.detach().cpu().numpy(), None if lengths is None else lengths.detach().cpu().numpy(),
                          self.batch.detach().cpu().numpy(), B, None if free is None else (~free).cpu().numpy(),
                          max_atoms=hip.MDC_MAX_ATOMS)
        if lengths is None:
            x = pos0.cpu().double().numpy()
            d2 = ((x[prep.pairs[:, 0]] - x[prep.pairs[:, 1]]) ** 2).sum(1)
        else:
            d2 = lengths.detach().cpu().double().numpy()[prep.order] ** 2
        self._con = _c.device_tables(prep, d2.astype(np.float32), self._mol_ptr)
        self._con_tol, self._con_max_iter = tol, max_iter
        self.constraint_pairs = torch.from_numpy(prep.pairs).to(dev)                  # (sorted by molecule and colour)
        self.constraint_lengths = torch.from_numpy(np.sqrt(d2).astype(np.float32)).to(dev)
        w = 1.0 / self.masses.double()
        self._inv_mass = (w if free is None else w * free).float().contiguous()
        self._inv_dth = float(np.float32(1.0 / self._dth))
        self._dof = (3 * self._counts - torch.from_numpy(prep.per_mol).to(dev)).float()
        self._n_failed = torch.zeros(B, dtype=torch.int32, device=dev)
        self._n_sweeps = torch.zeros(B, dtype=torch.int32, device=dev)
        self._constrained_step(hip.MDC_PROJECT, pos_out=self._pos[1])
        self._cur = 1
        failed = self._n_failed.cpu()
        if bool(failed.any()):
            raise ValueError(f'constraints: the initial positions could not be brought onto the constraints within {max_iter} sweeps '
                             f'(molecules {torch.nonzero(failed).reshape(-1).tolist()[:8]}): are the lengths far from the geometry?')

    def _constrained_step(self, flags, pos_out=None, force=None, noise=None, ke_out=None):
        hip.md_step_constrained(self._pos[self._cur], self._vel, force, self._hk, self._inv_mass, self._dth, self._inv_dth, self._c1,
                                flags, self._con, self._con_tol, self._con_max_iter, self._n_failed, self._n_sweeps,
                                pos_out=pos_out, mass=self.masses, sigma=None if noise is None else self._sigma, noise=noise,
                                ke_out=ke_out)

    @property
    def constraint_failures(self):
        """int32 [B]: the launches in which a constraint solve of the molecule did not converge or met the breakdown guard"""
        if self._con is None:
            raise AttributeError('this Dynamics has no constraints')
        return self._n_failed.clone()

    @property
    def constraint_sweeps(self):
        """int32 [B]: the largest sweep count among the solves of the last launch"""
        if self._con is None:
            raise AttributeError('this Dynamics has no constraints')
        return self._n_sweeps.clone()

    # ------------------------------------------------------------------------------------------
    def _evaluate(self):
        """forces and energies at the current positions.  Touching gradient_force settles the deferred record of the call -- a
        repeat, if one is needed, happens HERE, from the buffer the call was queued with and before any kernel writes a buffer"""
        out = self.model(self.z, self._pos[self._cur], self.cell, self.batch)
        self._force = out.gradient_force
        self._energy = out.energy

    def _finish(self):
        """the second half kick with the current forces, and the kinetic energies of the full-step velocities"""
        if self._con is not None:
            self._constrained_step(hip.MD_FINISH, force=self._force, ke_out=self._ke_atom)
        else:
            hip.md_step(None, self._vel, self._force, self._hk, self._dth, self._c1, hip.MD_FINISH, mass=self.masses,
                        ke_out=self._ke_atom)
        hip.md_kinetic(self._ke_atom, self._mol_ptr, out=self._ke)

    def _ensure_state(self):
        if self._force is None:
            with torch.no_grad():
                self._evaluate()
                # (kinetic energies of the initial velocities from the kernel that computes every later one: a kick with zero forces)
                if self._con is not None:
                    self._constrained_step(hip.MD_FINISH, force=torch.zeros_like(self._force), ke_out=self._ke_atom)
                else:
                    hip.md_step(None, self._vel, torch.zeros_like(self._force), self._hk, self._dth, self._c1, hip.MD_FINISH,
                                mass=self.masses, ke_out=self._ke_atom)
                hip.md_kinetic(self._ke_atom, self._mol_ptr, out=self._ke)

    @property
    def positions(self):
        return self._pos[self._cur].detach().clone()

    @property
    def velocities(self):
        return self._vel.clone()

    @property
    def forces(self):
        self._ensure_state()
        return self._force

    @property
    def potential_energy(self):
        self._ensure_state()
        return self._energy

    @property
    def kinetic_energy(self):
        self._ensure_state()
        return self._ke.clone()

    # ------------------------------------------------------------------------------------------
    def run(self, n_steps: int, record_every: int = 0) -> Trajectory:
        """Advance every molecule by n_steps and return what was recorded: the steps record_every, 2 record_every, ... of this call
        and its final step (record_every = 0: the final step only; n_steps = 0: the current state).  May be called again: the state
        between calls is (positions, velocities, forces, energies) at a full step, and run(a); run(b) leaves the same bits as
        run(a + b).  Langevin dynamics draws exactly one torch.randn((N, 3)) per step from the generator, in step order."""
        n_steps, recorded = self._recorded_steps(n_steps, record_every)
        with torch.no_grad():
            self._ensure_state()
            traj = self._new_trajectory(Trajectory, recorded)
            r = 0
            pending = False          # the second half kick of the previous step has not been launched yet
            for k in range(1, n_steps + 1):
                self._advance(pending)
                pending = True
                if k == recorded[r]:
                    self._finish()
                    pending = False
                    self._store(traj, r)
                    r += 1
            if n_steps == 0:
                self._store(traj, 0)
            self.step_count += n_steps
        return traj

    # ---- the pieces of run (newtonnet_amd/remd.py puts its exchange attempts between them)
    @staticmethod
    def _recorded_steps(n_steps, record_every):
        """(n_steps, the steps of a call that are recorded) of run's two arguments, refused without touching the device"""
        if int(n_steps) != n_steps or n_steps < 0:
            raise ValueError(f'n_steps: an integer >= 0 expected (got {n_steps!r})')
        if int(record_every) != record_every or record_every < 0:
            raise ValueError(f'record_every: an integer >= 0 expected (got {record_every!r})')
        n_steps, every = int(n_steps), int(record_every)
        recorded = list(range(every, n_steps + 1, every)) if every else []
        if not recorded or recorded[-1] != n_steps:
            recorded.append(n_steps)
        return n_steps, recorded

    def _new_trajectory(self, cls, recorded):
        R, N, B, dev = len(recorded), self.n_atoms, self.n_mol, self._vel.device
        traj = cls(torch.tensor([self.step_count + k for k in recorded], dtype=torch.int64, device=dev),
                   torch.empty(R, N, 3, dtype=torch.float32, device=dev), torch.empty(R, N, 3, dtype=torch.float32, device=dev),
                   torch.empty(R, B, dtype=torch.float32, device=dev), torch.empty(R, B, dtype=torch.float32, device=dev),
                   self._counts)
        if self._dof is not None:
            traj._dof = self._dof
        traj._system = (self.z, self.batch, self.cell, self.masses, self.timestep)
        return traj

    def _advance(self, pending: bool):
        """the noise of a step, the first half of it (with the second half kick of the step before, if that is still pending) and
        the forces at the new positions"""
        noise = None
        if self._sigma is not None:
            noise = torch.randn((self.n_atoms, 3), generator=self.generator, device=self._vel.device, dtype=torch.float32)
        other = 1 - self._cur
        flags = (hip.MD_FINISH | hip.MD_BEGIN) if pending else hip.MD_BEGIN
        if self._con is not None:
            self._constrained_step(flags, pos_out=self._pos[other], force=self._force, noise=noise)
        else:
            hip.md_step(self._pos[self._cur], self._vel, self._force, self._hk, self._dth, self._c1, flags,
                        pos_out=self._pos[other], sigma=self._sigma, noise=noise)
        self._cur = other
        self._evaluate()

    def _store(self, traj, r: int):
        traj.pos[r].copy_(self._pos[self._cur])
        traj.vel[r].copy_(self._vel)
        traj.potential_energy[r].copy_(self._energy)
        traj.kinetic_energy[r].copy_(self._ke)
