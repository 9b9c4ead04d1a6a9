"""Constant-pressure (NPT) batched molecular dynamics on the HIP path: `Dynamics` with a cell that breathes.

Isotropic stochastic cell rescaling (Bernetti & Bussi, J. Chem. Phys. 153, 114107 (2020)) as a first-order (Euler) step S for
eps = ln V inside the BAOAB step of newtonnet_amd/dynamics.py:

    B(F_k) [full-step v, KE] B(F_k) S A O A,   then the model at the new positions with the new cell

    S, per system b:   P_int = (2 K + tr W) / (3 V)        K: kinetic energy of the full-step velocities, W: the model's virial
                       d eps = -a_b (P0_b - P_int) + s_b xi_b,   a = beta_T dt / tau_p,  s = sqrt(2 k_B T_b beta_T dt / (tau_p V))
                       mu = exp(d eps / 3);   x <- mu x,  cell <- mu cell,  v <- v / mu

Both half kicks of a step use the forces of the geometry they belong to: S comes after them and before the first half drift, so no
kick ever sees a force from before a rescale.  Two launches per step (nnhip_npt_barostat, nnhip_npt_step: csrc/npt.hip) beside the
model's, no host read in the loop.  DESIGN.md section 18 has the derivation, the rounding chain and the measurements.

Left out on purpose: anisotropic or fully flexible cells; a coupling interval above one step; constant pressure under
ReplicaExchange, PathIntegral or Metadynamics; a time-reversible splitting of the barostat; `fixed` atoms and `constraints` (a
rescale moves fixed atoms and changes bond lengths).

Units: as in dynamics.py (Angstrom, eV, amu, fs for the arguments), pressures and the compressibility in bar and 1 / bar.
"""
from __future__ import annotations

import math

import torch

from newtonnet_amd import hip
from newtonnet_amd.dynamics import K_BOLTZMANN, Dynamics, Trajectory, _check_devices, _check_system, _check_temperature

BAR = 1e5 * 1e-30 / 1.602176634e-19         # one bar in eV / Angstrom^3: 6.241509e-7
AMU_PER_A3_IN_G_PER_CM3 = 1.66053906660     # one amu / Angstrom^3 in g / cm^3


def _per_system(value, n_mol: int, name: str) -> torch.Tensor:
    """fp64 [B] on the host (a number) or where `value` lives (a [B] tensor)"""
    if isinstance(value, torch.Tensor) and value.dim() > 0:
        if value.numel() != n_mol:
            raise ValueError(f'{name}: a number or one value per system ({n_mol}) expected (got {value.numel()})')
        return value.detach().to(torch.float64).reshape(-1)
    v = float(value)
    if not math.isfinite(v):
        raise ValueError(f'{name}: a finite value expected (got {value!r})')
    return torch.full((n_mol,), v, dtype=torch.float64)


def barostat_coefficients(timestep_fs: float, barostat_time_fs: float, compressibility_per_bar: float, pressure_bar, temperature,
                          n_mol: int):
    """(a, p0, s2), fp32 [B] each, of the barostat step  d eps = -a (p0 - P) + sqrt(s2 / V) xi  in the internal units (eV,
    Angstrom):  a = beta_T dt / tau_p  with beta_T in Angstrom^3 / eV,  p0 = the target pressure in eV / Angstrom^3,
    s2 = 2 k_B T a  in Angstrom^3.  Formed in fp64 and rounded once.  pressure, temperature: a number or a [B] tensor."""
    dt, tau, beta = float(timestep_fs), float(barostat_time_fs), float(compressibility_per_bar)
    if not (dt > 0.0 and math.isfinite(dt)):
        raise ValueError(f'timestep: a finite value > 0 fs expected (got {timestep_fs!r})')
    if not (tau > 0.0 and math.isfinite(tau)):
        raise ValueError(f'barostat_time: a finite value > 0 fs expected (got {barostat_time_fs!r})')
    if not (beta >= 0.0 and math.isfinite(beta)):
        raise ValueError(f'compressibility: a finite value >= 0 per bar expected (got {compressibility_per_bar!r})')
    P, T = _per_system(pressure_bar, n_mol, 'pressure'), _per_system(temperature, n_mol, 'temperature')
    dev = next((t.device for t in (P, T) if t.device.type != 'cpu'), P.device)        # (numbers follow a tensor to its device)
    P, T = P.to(dev), T.to(dev)
    a = torch.full_like(P, (beta / BAR) * (dt / tau))
    return a.float(), (P * BAR).float(), (2.0 * K_BOLTZMANN * T * a).float()


class NPTTrajectory(Trajectory):
    """What ConstantPressure.run recorded: Trajectory's fields (positions unwrapped, in the cell of their step) and

    cell      fp32 [R,B,3,3]   the cell of every system at the recorded step
    volume    fp32 [R,B]       det(cell), Angstrom^3
    pressure  fp32 [R,B]       the internal pressure (2 K + tr W) / (3 V) of the recorded state in bar, as the barostat kernel formed it
    density   fp32 [R,B]       total mass / volume in g / cm^3
    """
    cell = volume = pressure = _mass = None

    @property
    def density(self):
        return self._mass[None, :] / self.volume * AMU_PER_A3_IN_G_PER_CM3

    def _frame_cells(self):
        return self.cell


class ConstantPressure(Dynamics):
    """B periodic systems advanced together on the device at constant pressure and temperature.

    model: a NewtonNet in eval mode with the 'energy' and 'gradient_force' heads and a 'virial' or 'stress' head.  z, pos, cell,
    batch, masses, velocities, timestep, friction, generator: as for Dynamics (friction = 0: no thermostat, the barostat alone
    exchanges heat).  pressure: bar, a number or [B].  temperature: K, a number or [B]; required (the barostat's noise has it).
    compressibility: the isothermal compressibility estimate beta_T, 1 / bar (4.5e-5: water); 0 switches the coupling off, and
    the run is then Dynamics' bit for bit.  barostat_time: tau_p, fs.  Every system needs det(cell) > 0 (checked once, at
    construction, with one host read).  `fixed` and `constraints` are not offered.

    Random numbers, per step and in this order: one torch.randn((B,)) for the barostat (only when compressibility > 0), then one
    torch.randn((N, 3)) for the thermostat (only when friction > 0).  Positions stay unwrapped and scale with the cell."""

    _cells = None

    def __init__(self, model, z, pos, cell, batch, pressure, temperature, compressibility=4.5e-5, barostat_time=1000.0,
                 friction=0.0, timestep=0.5, masses=None, velocities=None, generator=None, fixed=None, constraints=None):
        # ---- everything that can be refused without touching the device
        if fixed is not None or constraints is not None:
            raise ValueError('ConstantPressure offers neither fixed atoms nor constraints: a cell rescale moves every atom and '
                             'changes every bond length')
        N, B, timestep, friction = _check_system(model, z, pos, cell, batch, masses, velocities, None, timestep, friction)
        props = list(getattr(model, 'output_properties', []))
        if 'virial' not in props and 'stress' not in props:
            raise ValueError(f"ConstantPressure needs a model with a 'virial' or 'stress' head (it has {props})")
        if temperature is None:
            raise ValueError('ConstantPressure needs a temperature')
        _check_temperature(temperature, B)
        for name, value in (('compressibility', compressibility), ('barostat_time', barostat_time)):
            if not (float(value) >= 0.0 and math.isfinite(float(value))):
                raise ValueError(f'{name}: a finite value >= 0 expected (got {value!r})')
        a, p0, s2 = barostat_coefficients(timestep, barostat_time, compressibility, pressure, temperature, B)
        dev = _check_devices(pos, generator, z=z, cell=cell, batch=batch, masses=masses, velocities=velocities,
                             temperature=temperature, pressure=pressure)
        if B and not bool((torch.linalg.det(cell.detach().double()) > 0).all().cpu()):       # (the one host read)
            raise ValueError('ConstantPressure needs periodic systems with det(cell) > 0 (a right-handed cell of positive volume)')
        # ---- state: Dynamics', two cell buffers beside its two position buffers, the barostat's coefficients and records
        super().__init__(model, z, pos, cell, batch, masses=masses, velocities=velocities, temperature=temperature,
                         friction=friction, timestep=timestep, generator=generator)
        self._virial_of = (lambda out: out.virial) if 'virial' in props else (lambda out: -out.displacement_grad)
        self.pressure, self.compressibility, self.barostat_time = pressure, float(compressibility), float(barostat_time)
        with torch.no_grad():
            self._cells = [cell.detach().clone().contiguous(), torch.empty(B, 3, 3, dtype=torch.float32, device=dev)]
            self._a, self._p0 = a.to(dev).contiguous(), p0.to(dev).contiguous()
            self._s2 = s2.to(dev).contiguous() if self.compressibility > 0.0 else None
            self._mol_of_atom = batch.to(torch.int32).contiguous()
            self._total_mass = torch.zeros(B, dtype=torch.float32, device=dev).index_add_(0, batch.long(), self.masses)
            self._mu, self._inv_mu, self._baro_ke, self._pressure, self._volume, self._deps = (
                torch.zeros(B, dtype=torch.float32, device=dev) for _ in range(6))
            self._virial = None
            self._baro_ready = False        # the barostat launch of the NEXT step has already run (it ran for a record)

    # the cell the model sees: Dynamics stores the caller's tensor; from then on it is the current buffer
    @property
    def cell(self):
        return self._cell0 if self._cells is None else self._cells[self._cur].clone()

    @cell.setter
    def cell(self, value):
        self._cell0 = value

    @property
    def volume(self):
        """fp32 [B]: det(cell) of the current state, as the barostat kernel formed it"""
        self._ensure_state()
        return self._volume.clone()

    @property
    def internal_pressure(self):
        """fp32 [B], bar: (2 K + tr W) / (3 V) of the current state, as the barostat kernel formed it"""
        self._ensure_state()
        return self._pressure * (1.0 / BAR)

    # ------------------------------------------------------------------------------------------
    def _evaluate(self):
        """forces, energies and the virial at the current positions and cell; touching them settles the deferred call before any
        kernel writes a buffer (Dynamics._evaluate)"""
        out = self.model(self.z, self._pos[self._cur], self._cells[self._cur], self.batch)
        self._force = out.gradient_force
        self._energy = out.energy
        self._virial = self._virial_of(out)

    def _barostat(self, force):
        """the barostat launch of the coming step from the current state: its noise, then cell[other], mu and the records"""
        noise = None
        if self._s2 is not None:
            noise = torch.randn((self.n_mol,), generator=self.generator, device=self._vel.device, dtype=torch.float32)
        hip.npt_barostat(self._vel, self.masses, self._mol_ptr, self._cells[self._cur], self._virial, self._a, self._p0,
                         self._cells[1 - self._cur], self._mu, self._inv_mu, self._baro_ke, self._pressure, self._volume, self._deps,
                         force=force, hk=None if force is None else self._hk, s2=self._s2, noise=noise)
        self._baro_ready = True

    def _finish(self):
        """Dynamics' second half kick and kinetic energies, then the barostat of the coming step on the full-step velocities: a
        record holds the pressure and the volume of its own state"""
        super()._finish()
        self._barostat(None)

    def _ensure_state(self):
        if self._force is None:
            super()._ensure_state()
            with torch.no_grad():
                self._barostat(None)

    def _advance(self, pending: bool):
        """the barostat of the step (unless a record has run it already), the noise of the thermostat, the first half of the step
        (with the second half kick of the step before, if that is still pending) and the model at the new positions and cell"""
        if not self._baro_ready:
            self._barostat(self._force if pending else None)
        noise = None
        if self._sigma is not None:
            noise = torch.randn((self.n_atoms, 3), generator=self.generator, device=self._vel.device, dtype=torch.float32)
        other = 1 - self._cur
        flags = (hip.MD_FINISH | hip.MD_BEGIN) if pending else hip.MD_BEGIN
        hip.npt_step(self._pos[self._cur], self._vel, self._force, self._hk, self._dth, self._c1, flags, mu=self._mu,
                     inv_mu=self._inv_mu, mol_of_atom=self._mol_of_atom, pos_out=self._pos[other], sigma=self._sigma, noise=noise)
        self._cur = other
        self._baro_ready = False
        self._evaluate()

    def _new_trajectory(self, cls, recorded):
        traj = super()._new_trajectory(NPTTrajectory, recorded)
        R, B, dev = len(recorded), self.n_mol, self._vel.device
        traj.cell = torch.empty(R, B, 3, 3, dtype=torch.float32, device=dev)
        traj.volume = torch.empty(R, B, dtype=torch.float32, device=dev)
        traj.pressure = torch.empty(R, B, dtype=torch.float32, device=dev)
        traj._mass = self._total_mass
        return traj

    def _store(self, traj, r: int):
        super()._store(traj, r)
        traj.cell[r].copy_(self._cells[self._cur])
        traj.volume[r].copy_(self._volume)
        torch.mul(self._pressure, 1.0 / BAR, out=traj.pressure[r])

    def run(self, n_steps: int, record_every: int = 0) -> NPTTrajectory:
        """Dynamics.run with an NPTTrajectory: run(a); run(b) leaves the bits of run(a + b), record_every changes no bit (a
        recorded step splits into finish, barostat, store, begin: the barostat runs exactly once per step either way, on the
        same full-step velocities)."""
        return super().run(n_steps, record_every)
