"""Path-integral molecular dynamics (ring polymers) on the HIP path: G systems x P beads are the B = G P molecules of ONE model()
call per step, and one launch (nnhip_pimd_step, csrc/pimd.hip) per step couples the beads -- the ring-polymer normal-mode
transform of the forces, the exact propagation of the free ring polymer, the PILE thermostat (Ceriotti, Parrinello, Markland and
Manolopoulos 2010) and the terms of the quantum estimators -- with no host round trip.

The layout is newtonnet_amd/remd.py's: molecule g P + s is bead s of system g.  The STATE is held in normal-mode coordinates, u
(mode positions) and w (mode velocities) in the same layout, slot k holding mode k; the Cartesian bead positions exist only as the
buffer handed to the model, written by the launch's back-transform, and the forces reach the modes by its forward transform.  The
state never makes a Cartesian <-> mode round trip, so no rounding accumulates from one.

Conventions: RPMD's -- the beads are sampled at P T with the physical masses on every mode; omega_P = P k_B T / hbar and the mode
frequencies are omega_k = 2 omega_P sin(k pi / P).  BAOAB with the A step exact for the free ring polymer; the O step has the
friction gamma_0 = centroid_friction on the centroid and gamma_k = 2 mode_friction omega_k on the other modes:
    centroid_friction = 0, mode_friction = 0   RPMD (no random numbers are drawn)
    centroid_friction = 0, mode_friction > 0   thermostatted RPMD (T-RPMD)
    centroid_friction > 0, mode_friction > 0   PILE: canonical sampling
With P = 1 it is `Dynamics`, bit for bit.

Not done here: constant pressure, ring-polymer contraction, centroid MD / adiabatic mass scaling, GLE thermostats, beads x replica
exchange, fixed atoms (a fixed atom with a spread ring would rotate in its springs), systems of unequal bead counts in one object,
an in-kernel Gaussian generator.

Units: as in newtonnet_amd/dynamics.py (Angstrom, eV, amu, fs, K)."""
from __future__ import annotations

import math

import numpy as np
import torch

from newtonnet_amd import hip
from newtonnet_amd.dynamics import FS, Dynamics, Trajectory, _check_devices, _check_system, _mol_ptr, _molecule_sums
from newtonnet_amd.vibrations import K_BOLTZMANN, _E_CHARGE, _PLANCK, table_masses

# hbar in eV x internal time unit (Angstrom sqrt(amu / eV)): J s -> eV s -> eV fs -> eV x internal = 0.0646541513
HBAR = _PLANCK / (2.0 * math.pi) / _E_CHARGE / 1e-15 * FS


def check_beads(n_beads) -> int:
    """n_beads as an int, refused without touching the device: an integer in 1 .. hip.PIMD_MAX_BEADS"""
    ok = not isinstance(n_beads, (bool, np.bool_)) and isinstance(n_beads, (int, np.integer)) and 1 <= int(n_beads) <= hip.PIMD_MAX_BEADS
    if not ok:
        raise ValueError(f'n_beads: an integer in 1 .. {hip.PIMD_MAX_BEADS} expected (got {n_beads!r})')
    return int(n_beads)


def check_temperature(temperature, n_systems: int) -> np.ndarray:
    """the temperatures as fp64 [G]: a number or [G] values, finite and > 0 K.  Host values are refused without touching the
    device; a device tensor is read here (its size is checked first)"""
    if temperature is None:
        raise ValueError('temperature: path-integral dynamics needs one (a number or one value per system)')
    if isinstance(temperature, torch.Tensor):
        if temperature.dim() > 0 and temperature.numel() != n_systems:
            raise ValueError(f'temperature: a number or one value per system ({n_systems}) expected (got {temperature.numel()})')
        temperature = temperature.detach().cpu().numpy()
    try:
        T = np.array(temperature, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f'temperature: a number or one value per system expected (got {temperature!r})') from None
    if T.size == 1 and np.ndim(temperature) == 0:
        T = np.full(n_systems, T[0])
    if T.size != n_systems:
        raise ValueError(f'temperature: a number or one value per system ({n_systems}) expected (got {T.size})')
    if not (np.isfinite(T).all() and (T > 0.0).all()):
        raise ValueError('temperature: finite values > 0 K expected')
    return T


def check_frictions(centroid_friction, mode_friction):
    out = []
    for name, v in (('centroid_friction', centroid_friction), ('mode_friction', mode_friction)):
        try:
            ok = float(v) >= 0.0 and math.isfinite(float(v))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f'{name}: a finite value >= 0 expected (got {v!r})')
        out.append(float(v))
    return tuple(out)


def transform_matrix(n_beads: int) -> np.ndarray:
    """C fp64 [P, P], the orthonormal ring-polymer normal-mode transform: u_k = sum_s C[k][s] x_s, x_s = sum_k C[k][s] u_k"""
    P = int(n_beads)
    s = np.arange(P)
    C = np.empty((P, P))
    for k in range(P):
        angle = 2.0 * math.pi * ((s * k) % P).astype(np.float64) / P         # (the integer product reduced first: a small argument)
        if k == 0:
            C[k] = 1.0 / math.sqrt(P)
        elif 2 * k < P:
            C[k] = math.sqrt(2.0 / P) * np.cos(angle)
        elif 2 * k == P:
            C[k] = np.where(s % 2 == 0, 1.0, -1.0) / math.sqrt(P)
        else:
            C[k] = math.sqrt(2.0 / P) * np.sin(angle)
    return C


def mode_frequencies(n_beads: int, temperature) -> np.ndarray:
    """omega_k fp64 [G, P] in 1 / internal time unit of temperatures [G] (K): 2 omega_P sin(k pi / P), omega_P = P k_B T / hbar"""
    P = int(n_beads)
    omega_P = P * K_BOLTZMANN * np.asarray(temperature, dtype=np.float64).reshape(-1, 1) / HBAR
    return 2.0 * omega_P * np.sin(np.arange(P, dtype=np.float64) * math.pi / P)[None, :]


def mode_tables(n_beads: int, temperature, timestep_fs: float, centroid_friction_per_fs: float, mode_friction: float,
                dtype=np.float32):
    """(mode_tab fp32 [G, P, 5], one_minus_c1sq fp64 [G, P]) of the launch, formed in fp64 and rounded once.  Columns of mode_tab,
    with h = dt / 2:  a = cos(omega_k h),  b = sin(omega_k h) / omega_k (k = 0: the fp32 dt / 2 `Dynamics` forms),
    d = -omega_k sin(omega_k h),  c1 = exp(-gamma_k dt) with gamma_0 = centroid_friction, gamma_k = 2 mode_friction omega_k,
    half_w2 = omega_k^2 / 2.  one_minus_c1sq = 1 - c1^2 as langevin_coefficients forms it.  dtype = np.float64: the unrounded table
    (b = dt / 2 for k = 0), for analysis."""
    P = int(n_beads)
    dt = float(timestep_fs) * FS
    h = 0.5 * dt
    om = mode_frequencies(P, temperature)                                  # [G, P]
    tab = np.empty(om.shape + (5,))
    tab[..., 0] = np.cos(om * h)
    with np.errstate(invalid='ignore', divide='ignore'):
        tab[..., 1] = np.where(om > 0.0, np.sin(om * h) / np.where(om > 0.0, om, 1.0), h)
    tab[:, 0, 1] = float(np.float32(h)) if dtype == np.float32 else h
    tab[..., 2] = -om * np.sin(om * h)
    gdt = 2.0 * float(mode_friction) * om * dt
    gdt[:, 0] = float(centroid_friction_per_fs) * float(timestep_fs)
    tab[..., 3] = np.exp(-gdt)
    tab[..., 4] = 0.5 * om * om
    one_minus = -np.expm1(-2.0 * gdt)
    # (the centroid's pair by the very calls of dynamics.langevin_coefficients, so that P = 1 reproduces its bits)
    tab[:, 0, 3] = math.exp(-float(gdt[0, 0])) if om.shape[0] else 1.0
    one_minus[:, 0] = -math.expm1(-2.0 * float(gdt[0, 0])) if om.shape[0] else 0.0
    return tab.astype(dtype), one_minus


class PathIntegralTrajectory(Trajectory):
    """What PathIntegral.run recorded, as device tensors (N = atoms of all G P beads, n = atoms of all G systems):

    step                 int64 [Rec]      step numbers since the PathIntegral was made
    pos                  fp32 [Rec,N,3]   bead positions, exactly what the model was given
    vel                  fp32 [Rec,N,3]   bead velocities, back-transformed from mode_vel at record time
    mode_pos, mode_vel   fp32 [Rec,N,3]   the state: slot k of a system holds normal mode k
    potential_energy     fp32 [Rec,G P]   the model's energy of every bead
    kinetic_energy       fp32 [Rec,G P]   sum of m w^2 / 2 per mode slot (of the ring polymer at P T)
                                          (Trajectory's total_energy and temperature are NOT offered: they raise AttributeError)
    potential            fp64 [Rec,G]     mean of potential_energy over the beads: the potential-energy estimator
    kinetic_virial       fp64 [Rec,G]     3 n k_B T / 2 - (1 / 2P) sum_{k>0} u_k . f_k: the centroid-virial kinetic-energy estimator
    kinetic_primitive    fp64 [Rec,G]     3 n P k_B T / 2 - (1 / P) sum of the spring energies
    ring_polymer_energy  fp64 [Rec,G]     kinetic + spring + sum_s V_s of the ring polymer: what RPMD conserves
    centroid             fp32 [Rec,n,3]   centroid positions (systems in order)
    radius_of_gyration   fp32 [Rec,n]     sqrt(mean_s |x_s - x_c|^2) per atom
    """

    def __init__(self, *a):
        super().__init__(*a)
        self.mode_pos = self.mode_vel = self.potential = self.kinetic_virial = self.kinetic_primitive = None
        self.ring_polymer_energy = self.centroid = self.radius_of_gyration = None

    # Trajectory's two derived fields pair a slot's potential with a slot's kinetic energy; here a slot holds a BEAD's potential and
    # a MODE's kinetic energy, so neither means anything per slot: not offered
    @property
    def total_energy(self):
        raise AttributeError('a ring-polymer trajectory has no per-slot total energy: see ring_polymer_energy (conserved by RPMD) '
                             'and potential + kinetic_virial (the quantum energy estimator)')

    @property
    def temperature(self):
        raise AttributeError('a ring-polymer trajectory has no per-slot temperature: the modes are thermostatted at P T; see '
                             'kinetic_virial and kinetic_primitive for the quantum kinetic energy')


class PathIntegral(Dynamics):
    """G ring polymers of P beads advanced together on the device.

    model, z, pos, cell, batch, masses, timestep, generator: as for Dynamics, describing the G systems; each is replicated P times,
    system-major (molecule g P + s is bead s of system g), and none of the caller's tensors is modified.  n_beads: 1 ..
    hip.PIMD_MAX_BEADS, one for the whole object.  temperature (K): a number or [G] values, > 0.  centroid_friction (1 / fs) and
    mode_friction (dimensionless, gamma_k = 2 mode_friction omega_k): see the module's text; both 0 draws no random numbers.
    Without bead_positions the beads start coincident at pos; bead_positions and bead_velocities (Cartesian, [G P atoms, 3] in the
    replicated layout) are for restarts and are transformed to modes in fp64.  Without bead_velocities the mode velocities come
    from ONE torch.randn((N, 3)) at P T, the centre-of-mass momentum removed from the centroid; afterwards the generator's stream
    is exactly one randn((N, 3)) per step, the noise, drawn directly in mode space (an orthogonal map of iid Gaussians is iid
    Gaussian)."""

    def __init__(self, model, z, pos, cell, batch, n_beads, temperature, timestep=0.25, centroid_friction=0.0, mode_friction=1.0,
                 masses=None, generator=None, bead_positions=None, bead_velocities=None):
        # ---- everything that can be refused without touching the device
        N0, G, timestep, _ = _check_system(model, z, pos, cell, batch, masses, None, None, timestep, 0.0)
        P = check_beads(n_beads)
        centroid_friction, mode_friction = check_frictions(centroid_friction, mode_friction)
        T = check_temperature(temperature, G)
        for name, t in (('bead_positions', bead_positions), ('bead_velocities', bead_velocities)):
            if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (N0 * P, 3)):
                raise ValueError(f'{name}: a tensor [{N0 * P},3] expected (the atoms of all {P} beads of every system)')
        dev = _check_devices(pos, generator, z=z, cell=cell, batch=batch, masses=masses, temperature=temperature,
                             bead_positions=bead_positions, bead_velocities=bead_velocities)
        # ---- state
        self.model, self.n_systems, self.n_beads = model, G, P
        self.timestep, self.centroid_friction, self.mode_friction = timestep, centroid_friction, mode_friction
        self.friction = centroid_friction
        self.generator, self.step_count = generator, 0
        with torch.no_grad():
            # the replicated batch: the atoms of system g, P times in a row
            counts = torch.bincount(batch.long(), minlength=G)
            ptr = torch.zeros(G + 1, dtype=torch.long, device=dev)
            ptr[1:] = torch.cumsum(counts, 0)
            rep_counts = counts.repeat_interleave(P)
            rep_batch = torch.repeat_interleave(torch.arange(G * P, device=dev), rep_counts)
            rep_ptr = torch.zeros(G * P + 1, dtype=torch.long, device=dev)
            rep_ptr[1:] = torch.cumsum(rep_counts, 0)
            system = torch.div(rep_batch, P, rounding_mode='floor')
            atom = torch.arange(rep_batch.numel(), device=dev) - rep_ptr[rep_batch]           # index within the system
            src = ptr[system] + atom
            N = rep_batch.numel()
            self.z, self.cell, self.batch = z[src], cell.repeat_interleave(P, dim=0), rep_batch.to(batch.dtype)
            self.n_atoms, self.n_mol = N, G * P
            m = table_masses(self.z) if masses is None else masses.detach().float().reshape(-1)[src].clone()
            if N and not bool(((m > 0) & torch.isfinite(m)).all()):
                raise ValueError('masses: positive finite values expected')
            self.masses = m.contiguous()
            self.temperatures = torch.tensor(T, dtype=torch.float64, device=dev)                # [G]: one per SYSTEM
            self._mol_ptr = _mol_ptr(rep_batch, G * P)
            self._mol_ptr_host = self._mol_ptr.cpu()
            self._counts = (self._mol_ptr[1:] - self._mol_ptr[:-1]).long()
            self._slot = (rep_batch - system * P).long()                                        # [N]: the slot of every row
            # [N, P]: the rows of the same atom in every slot of the row's system
            self._rows = (rep_ptr[system * P] + atom)[:, None] + torch.arange(P, device=dev)[None, :] * counts[system][:, None]
            self._centroid_rows = torch.nonzero(self._slot == 0).reshape(-1)
            # ---- tables (fp64 on the host, rounded once)
            C = transform_matrix(P)
            self._ctab = torch.from_numpy(C.astype(np.float32)).to(dev).contiguous()
            tab, one_minus = mode_tables(P, T, timestep, centroid_friction, mode_friction)
            self._mode_tab = torch.from_numpy(tab.reshape(G * P, 5)).to(dev).contiguous()
            dt = timestep * FS
            self._hk = ((0.5 * dt) / m.double()).float().contiguous()
            self._hk_zero = torch.zeros_like(self._hk)
            T_row = (float(P) * self.temperatures)[system]                                      # fp64 [N]: P T of every row
            self._sigma = None
            if centroid_friction > 0.0 or (mode_friction > 0.0 and P > 1):
                om = torch.from_numpy(one_minus.reshape(-1)).to(dev)[rep_batch.long()]
                self._sigma = torch.sqrt(om * K_BOLTZMANN * T_row / m.double()).float().contiguous()
            # ---- the state, in mode coordinates
            Cd = torch.from_numpy(C).to(dev)
            self._C64_rows = Cd[self._slot]                                                     # [N, P]: row k of C for a row of slot k
            self._Ct64_rows = Cd.t().contiguous()[self._slot]                                   # [N, P]: column s of C for a row of slot s
            if bead_positions is not None:
                u = self._to_modes(bead_positions.detach().double())
            else:
                u = (self._slot == 0)[:, None] * (math.sqrt(P) * pos.detach().double()[src])     # coincident beads: u_0 = sqrt(P) x
            self._u = u.float().contiguous()
            if bead_velocities is not None:
                w = self._to_modes(bead_velocities.detach().double()).float()
            else:
                xi = torch.randn((N, 3), generator=generator, device=dev, dtype=torch.float32)
                v = xi * torch.sqrt(K_BOLTZMANN * T_row / m.double()).float()[:, None]
                s = _molecule_sums(torch.cat([m[:, None] * v, m[:, None]], dim=1), rep_batch, G * P)     # [B, 4]: momentum, mass
                w = torch.where((self._slot == 0)[:, None], v - (s[:, :3] / s[:, 3:].clamp(min=1e-30))[rep_batch.long()], v)
            self._w = w.contiguous()
            self._vel = self._w                      # (Dynamics's name for the velocity state: here the mode velocities)
            # two position buffers, for the reason given in dynamics.py; the first is the back-transform of the state
            ct32 = torch.from_numpy(C.astype(np.float32).astype(np.float64).T.copy()).to(dev)[self._slot]
            x0 = (ct32[:, :, None] * self._u.double()[self._rows]).sum(1).float()
            self._pos = [x0.contiguous(), torch.empty(N, 3, dtype=torch.float32, device=dev)]
            self._cur = 0
            self._est = torch.zeros(N, 4, dtype=torch.float32, device=dev)
            self._ke = torch.zeros(G * P, dtype=torch.float32, device=dev)
            self._sums = torch.zeros(G, 4, dtype=torch.float64, device=dev)
            n_g = counts.double()
            self._virial_const = 1.5 * n_g * K_BOLTZMANN * self.temperatures
            self._primitive_const = 1.5 * n_g * P * K_BOLTZMANN * self.temperatures
            self._force = self._energy = None

    # ------------------------------------------------------------------------------------------
    def _to_modes(self, x64):
        """u_k = sum_s C[k][s] x_s in fp64, for rows in the slot layout"""
        return (self._C64_rows[:, :, None] * x64[self._rows]).sum(1)

    def _to_beads(self, u64):
        """x_s = sum_k C[k][s] u_k in fp64"""
        return (self._Ct64_rows[:, :, None] * u64[self._rows]).sum(1)

    def _launch(self, flags, hk=None, noise=None, est=False):
        other = 1 - self._cur
        begin = bool(flags & hip.PIMD_BEGIN)
        hip.pimd_step(self._u, self._w, self._force, self._ctab, self._mode_tab, self._hk if hk is None else hk, self._mol_ptr,
                      self._mol_ptr_host, self.n_beads, flags, pos_out=self._pos[other] if begin else None,
                      pos_pending=self._pos[self._cur] if begin else None, mass=self.masses if est else None,
                      sigma=self._sigma if noise is not None else None, noise=noise, est_out=self._est if est else None)
        if begin:
            self._cur = other

    def _reduce(self):
        """the per-slot and per-system sums of the estimator terms of the last finish"""
        hip.md_kinetic(self._est[:, 0].contiguous(), self._mol_ptr, out=self._ke)
        per_slot = hip.segment_sum(self._est, self._mol_ptr, self.n_mol)                       # [B, 4] fp32
        self._sums = per_slot.view(self.n_systems, self.n_beads, 4).double().sum(1)            # [G, 4] fp64: kinetic, spring, virial

    def _finish(self):
        """the second half kick with the current forces, and the estimator terms at the full step"""
        self._launch(hip.PIMD_FINISH, est=True)
        self._reduce()

    def _ensure_state(self):
        if self._force is None:
            with torch.no_grad():
                self._evaluate()
                # (the estimator terms of the initial state from the kernel that computes every later one: a kick of zero length)
                self._launch(hip.PIMD_FINISH, hk=self._hk_zero, est=True)
                self._reduce()

    def _advance(self, pending: bool):
        noise = None
        if self._sigma is not None:
            noise = torch.randn((self.n_atoms, 3), generator=self.generator, device=self._w.device, dtype=torch.float32)
        self._launch((hip.PIMD_FINISH | hip.PIMD_BEGIN) if pending else hip.PIMD_BEGIN, noise=noise)
        self._evaluate()

    @property
    def velocities(self):
        """bead velocities fp32 [N,3], back-transformed from the mode velocities"""
        return self._to_beads(self._w.double()).float()

    @property
    def mode_positions(self):
        return self._u.clone()

    @property
    def mode_velocities(self):
        return self._w.clone()

    # ------------------------------------------------------------------------------------------
    def run(self, n_steps: int, record_every: int = 0) -> PathIntegralTrajectory:
        """Dynamics.run for ring polymers: one model() call over all G P beads and one nnhip_pimd_step(finish | begin) per step,
        the launch split at recorded steps; nothing in the loop reads the device.  run(a); run(b) leaves the bits of run(a + b)
        and record_every changes no bit.  With a thermostat exactly one torch.randn((N, 3)) per step is drawn from the generator."""
        return super().run(n_steps, record_every)

    def _new_trajectory(self, cls, recorded):
        traj = super()._new_trajectory(cls if issubclass(cls, PathIntegralTrajectory) else PathIntegralTrajectory, recorded)
        R, N, G, dev = len(recorded), self.n_atoms, self.n_systems, self._w.device
        n = N // self.n_beads
        traj.mode_pos, traj.mode_vel = torch.empty_like(traj.pos), torch.empty_like(traj.pos)
        for name in ('potential', 'kinetic_virial', 'kinetic_primitive', 'ring_polymer_energy'):
            setattr(traj, name, torch.empty(R, G, dtype=torch.float64, device=dev))
        traj.centroid = torch.empty(R, n, 3, dtype=torch.float32, device=dev)
        traj.radius_of_gyration = torch.empty(R, n, dtype=torch.float32, device=dev)
        return traj

    def _store(self, traj, r: int):
        P = self.n_beads
        x = self._pos[self._cur]
        traj.pos[r].copy_(x)
        traj.vel[r].copy_(self.velocities)
        traj.mode_pos[r].copy_(self._u)
        traj.mode_vel[r].copy_(self._w)
        traj.potential_energy[r].copy_(self._energy)
        traj.kinetic_energy[r].copy_(self._ke)
        v_sum = self._energy.reshape(self.n_systems, P).double().sum(1)
        traj.potential[r].copy_(v_sum / P)
        traj.kinetic_virial[r].copy_(self._virial_const - self._sums[:, 2] / (2.0 * P))
        traj.kinetic_primitive[r].copy_(self._primitive_const - self._sums[:, 1] / P)
        traj.ring_polymer_energy[r].copy_(self._sums[:, 0] + self._sums[:, 1] + v_sum)
        beads = x.double()[self._rows[self._centroid_rows]]                                    # [n, P, 3]
        c = beads.mean(1)
        traj.centroid[r].copy_(c)
        traj.radius_of_gyration[r].copy_(torch.sqrt(((beads - c[:, None, :]) ** 2).sum(2).mean(1)))
