"""Biased molecular dynamics on collective variables on the HIP path: multiple-walker (well-tempered) metadynamics and umbrella
restraints.  G systems x W walkers are the B = G W molecules of ONE model() call per step, integrated together by `Dynamics`
(csrc/md.hip), and one launch per step (nnhip_bias_step, csrc/bias.hip) forms the collective variables and their gradients from
the device positions, sums the hills the walkers of a group share, adds the harmonic restraints, applies the chain rule to the
model's forces and -- every `pace` steps -- deposits one hill per walker, with no host read in the loop.

A group is the W walkers of one system, the consecutive molecules g W .. g W + W - 1 (ReplicaExchange's layout).  The walkers of a
group share one hill list (Raiteri, Laio, Gervasio, Micheletti and Parrinello 2006): it fills W times faster than one walker's.
The bias is V(s) = sum_h w_h exp(-sum_d (s_d - c_hd)^2 / (2 sigma_d^2)); a deposit adds a hill at every walker's current s of
height w0 (plain metadynamics) or w0 exp(-V(s) / (k_B dT)) with dT = (bias_factor - 1) T (well-tempered: Barducci, Bussi and
Parrinello 2008), V being the bias before any deposit of that step.  Static restraints U = sum_d kappa_d (s_d - s0_d)^2 / 2, one
(kappa, s0) per walker and variable, make every walker an umbrella window; with no hills they are all there is.

Collective variables: ('distance', i, j), ('angle', i, j, k) with the vertex j, ('torsion', i, j, k, l); indices local to the
molecule, at most two variables per system.  They are computed on the positions as stored: unwrapped, NO minimum image is taken.
Differences of a torsion are wrapped into (-pi, pi].

Not done here: grids for the bias, walls, further variables (coordination numbers, RMSD, path variables), more than two
variables, a hill cutoff, bias exchange, metadynamics on top of replica exchange or path integrals, reweighting (WHAM / MBAR),
PLUMED input, minimum-image variables.

Units: as in newtonnet_amd/dynamics.py (Angstrom, eV, amu, fs, K); angles and torsions in radians."""
from __future__ import annotations

import math

import numpy as np
import torch

from newtonnet_amd import hip
from newtonnet_amd.dynamics import Dynamics, Trajectory, _check_devices, _check_system, _check_temperature
from newtonnet_amd.vibrations import K_BOLTZMANN

KINDS = {'distance': (hip.BIAS_DISTANCE, 2), 'angle': (hip.BIAS_ANGLE, 3), 'torsion': (hip.BIAS_TORSION, 4)}
TWO_PI32 = float(np.float32(2.0 * math.pi))       # the period the kernel wraps a torsion's differences with


def _is_int(v) -> bool:
    if isinstance(v, bool):
        return False
    try:
        return int(v) == v
    except (TypeError, ValueError):
        return False


def check_cvs(cvs, counts) -> np.ndarray:
    """the variable table int32 [G, 2, 5] = (kind, a, b, c, d) of `cvs`, refused without touching the device.  cvs: one list for
    all systems, or one list per system; counts: the atom count of every system"""
    G = len(counts)
    if not isinstance(cvs, (list, tuple)):
        raise ValueError(f'cvs: a list of variables, or one list per system, expected (got {type(cvs).__name__})')
    per_system = len(cvs) > 0 and all(isinstance(e, (list, tuple)) and (len(e) == 0 or not isinstance(e[0], str)) for e in cvs)
    if per_system and len(cvs) != G:
        raise ValueError(f'cvs: one list per system ({G}) expected (got {len(cvs)})')
    table = np.zeros((G, hip.BIAS_MAX_CVS, 5), dtype=np.int32)
    for g in range(G):
        mine = cvs[g] if per_system else cvs
        if len(mine) > hip.BIAS_MAX_CVS:
            raise ValueError(f'cvs: at most {hip.BIAS_MAX_CVS} variables per system (got {len(mine)})')
        for d, cv in enumerate(mine):
            if not isinstance(cv, (list, tuple)) or len(cv) == 0 or cv[0] not in KINDS:
                raise ValueError(f"cvs: ('distance', i, j), ('angle', i, j, k) or ('torsion', i, j, k, l) expected (got {cv!r})")
            kind, arity = KINDS[cv[0]]
            if len(cv) != arity + 1:
                raise ValueError(f'cvs: a {cv[0]} takes {arity} atoms (got {cv!r})')
            idx = cv[1:]
            if not all(_is_int(i) and 0 <= i < counts[g] for i in idx):
                raise ValueError(f'cvs: atom indices in 0 .. {counts[g] - 1}, local to the molecule, expected (got {cv!r}, system {g})')
            if len({int(i) for i in idx}) != arity:
                raise ValueError(f'cvs: the atoms of a variable must differ (got {cv!r})')
            table[g, d, 0] = kind
            table[g, d, 1:1 + arity] = [int(i) for i in idx]
    return table


def check_bias_arguments(n_cv, temperature, friction, hill_height, hill_width, pace, bias_factor, walkers, restraint_k,
                         restraint_center, hill_capacity, n_systems):
    """(height, widths fp64 [2], pace, gamma or None, walkers, kappa, centre fp64 [G, W, 2], capacity), refused without touching the
    device.  n_cv: the largest number of variables of any system"""
    G = n_systems
    if not _is_int(walkers) or walkers < 1:
        raise ValueError(f'walkers: an integer >= 1 expected (got {walkers!r})')
    if not _is_int(pace) or pace < 0:
        raise ValueError(f'pace: an integer >= 0 expected (got {pace!r})')
    if not _is_int(hill_capacity) or hill_capacity < 1:
        raise ValueError(f'hill_capacity: an integer >= 1 expected (got {hill_capacity!r})')
    W, pace = int(walkers), int(pace)
    try:
        height = float(hill_height)
    except (TypeError, ValueError):
        height = float('nan')
    if not (height >= 0.0 and math.isfinite(height)):
        raise ValueError(f'hill_height: a finite value >= 0 eV expected (got {hill_height!r})')
    try:
        w = np.array(hill_width, dtype=np.float64)
        w = np.broadcast_to(w, (n_cv,)).copy() if w.ndim == 0 else w
    except (TypeError, ValueError):
        raise ValueError(f'hill_width: a number or one per variable expected (got {hill_width!r})') from None
    if w.ndim != 1 or w.shape[0] != n_cv:
        raise ValueError(f'hill_width: a number or one per variable ({n_cv}) expected (got {hill_width!r})')
    if not (np.isfinite(w).all() and (w > 0.0).all()):
        raise ValueError(f'hill_width: finite values > 0 expected (got {hill_width!r})')
    widths = np.ones(hip.BIAS_MAX_CVS)
    widths[:n_cv] = w
    gamma = None
    if bias_factor is not None:
        try:
            gamma = float(bias_factor)
        except (TypeError, ValueError):
            gamma = float('nan')
        if not (gamma > 1.0 and math.isfinite(gamma)):
            raise ValueError(f'bias_factor: None (plain metadynamics) or a finite value > 1 expected (got {bias_factor!r})')
    depositing = pace > 0 and height > 0.0
    if depositing and n_cv == 0:
        raise ValueError('hills need at least one collective variable')
    if depositing and not float(friction) > 0.0:
        raise ValueError('friction: depositing hills needs a thermostat, a value > 0 per fs (friction = 0 goes with pace = 0 or '
                         'hill_height = 0)')
    if gamma is not None and temperature is None:
        raise ValueError('bias_factor needs a temperature')
    if (restraint_k is None) != (restraint_center is None):
        raise ValueError('restraint_k and restraint_center come together')
    kappa, centre = np.zeros((G, W, hip.BIAS_MAX_CVS)), np.zeros((G, W, hip.BIAS_MAX_CVS))
    if restraint_k is not None:
        for name, src, dst in (('restraint_k', restraint_k, kappa), ('restraint_center', restraint_center, centre)):
            if isinstance(src, torch.Tensor):
                src = src.detach().cpu().numpy()
            try:
                dst[:, :, :n_cv] = np.broadcast_to(np.array(src, dtype=np.float64), (G, W, n_cv))
            except (TypeError, ValueError):
                raise ValueError(f'{name}: values that broadcast to [{G}, {W}, {n_cv}] (systems, walkers, variables) expected') from None
        if not (np.isfinite(kappa).all() and (kappa >= 0.0).all() and np.isfinite(centre).all()):
            raise ValueError('restraint_k: finite values >= 0, and restraint_center: finite values, expected')
    return height, widths, pace, gamma, W, kappa, centre, int(hill_capacity)


def hill_parameters(n_cv_of_system, widths, height, gamma, temperatures) -> np.ndarray:
    """hill_par fp32 [G, 4] = (1 / sigma_0^2, 1 / sigma_1^2, w0, 1 / (k_B dT)), formed in fp64 and rounded once; an unused variable
    gets 1 / sigma^2 = 0, plain metadynamics (gamma None) 1 / (k_B dT) = 0"""
    G = len(n_cv_of_system)
    par = np.zeros((G, 4))
    for g in range(G):
        for d in range(n_cv_of_system[g]):
            par[g, d] = 1.0 / (widths[d] * widths[d])
        par[g, 2] = height
        if gamma is not None:
            par[g, 3] = 1.0 / (K_BOLTZMANN * (gamma - 1.0) * temperatures[g])
    return par.astype(np.float32)


class BiasedTrajectory(Trajectory):
    """What Metadynamics.run recorded: Trajectory's tensors over the B = G W walkers, and

    cv                fp32 [Rec,B,2]  the collective variables at pos (0 for an unused one)
    bias_energy       fp32 [Rec,B]    V(s) of the group's hills; at a deposit step, before the deposit
    restraint_energy  fp32 [Rec,B]    U(s) of the walker's restraints
    n_hills           int64 [Rec]     hills in every group's list after that step
    potential_energy stays the MODEL's energy: the biased potential is potential_energy + bias_energy + restraint_energy."""

    def __init__(self, *a):
        super().__init__(*a)
        self.cv = self.bias_energy = self.restraint_energy = self.n_hills = None


class Metadynamics(Dynamics):
    """G systems x W walkers advanced together on the device under a bias on collective variables.

    model, z, pos, cell, batch, masses, fixed, timestep, generator: as for Dynamics, describing the G systems; each is replicated
    `walkers` times, group-major (molecule g W + j is walker j of system g), and none of the caller's tensors is modified.
    cvs: one list for all systems or one list per system, each of 0 .. 2 variables ('distance', i, j), ('angle', i, j, k),
    ('torsion', i, j, k, l), indices local to the molecule.  temperature (K): a number or [G]; friction (1 / fs): 0 = microcanonical
    in the restrained potential (no hills then).  hill_height (eV), hill_width (per variable, Angstrom or radians), pace: a
    deposit happens in the force evaluation of every step whose global number is a positive multiple of pace; pace = 0 or
    hill_height = 0 deposits nothing (umbrella sampling).  bias_factor: None = plain, gamma > 1 = well-tempered with dT = (gamma - 1)
    T.  restraint_k, restraint_center: broadcast to [G, W, n_cv] (eV per unit^2, unit).  hill_capacity: rows allocated per group at
    first; the list is doubled on the device when a deposit would not fit."""

    def __init__(self, model, z, pos, cell, batch, cvs, temperature, friction, hill_height, hill_width, pace, bias_factor=None,
                 walkers=1, restraint_k=None, restraint_center=None, timestep=0.5, masses=None, fixed=None, generator=None,
                 hill_capacity=1024):
        # ---- everything that can be refused without touching the device
        N, G, timestep, friction = _check_system(model, z, pos, cell, batch, masses, None, fixed, timestep, friction)
        _check_temperature(temperature, G)
        if friction > 0.0 and temperature is None:
            raise ValueError('friction > 0 (Langevin dynamics) needs a temperature')
        if batch.dtype not in (torch.int32, torch.int64) or (N and (int(batch.min()) < 0 or int(batch.max()) >= G)):
            raise ValueError(f'batch: integers in 0 .. {G - 1} expected')
        counts_host = np.bincount(batch.detach().cpu().numpy(), minlength=G).tolist()
        table = check_cvs(cvs, counts_host)
        n_cv_of_system = [int((table[g, :, 0] != 0).sum()) for g in range(G)]
        n_cv = max(n_cv_of_system, default=0)
        height, widths, self.pace, self.bias_factor, W, kappa, centre, capacity = check_bias_arguments(
            n_cv, temperature, friction, hill_height, hill_width, pace, bias_factor, walkers, restraint_k, restraint_center,
            hill_capacity, G)
        dev = _check_devices(pos, generator, z=z, cell=cell, batch=batch, masses=masses, fixed=fixed, temperature=temperature)
        self.n_systems, self.n_walkers = G, W
        self.hill_height, self.hill_width = height, widths[:n_cv].copy()
        self.cvs = table
        self._depositing = self.pace > 0 and height > 0.0
        # ---- the replicated batch: the atoms of system g, W times in a row (as ReplicaExchange lays its ladders out)
        with torch.no_grad():
            counts = torch.bincount(batch.long(), minlength=G)
            ptr = torch.zeros(G + 1, dtype=torch.long, device=dev)
            ptr[1:] = torch.cumsum(counts, 0)
            rep_batch = torch.repeat_interleave(torch.arange(G * W, device=dev), counts.repeat_interleave(W))
            rep_ptr = torch.zeros(G * W + 1, dtype=torch.long, device=dev)
            rep_ptr[1:] = torch.cumsum(counts.repeat_interleave(W), 0)
            system = torch.div(rep_batch, W, rounding_mode='floor')
            src = ptr[system] + (torch.arange(rep_batch.numel(), device=dev) - rep_ptr[rep_batch])
            T_rep = temperature
            T_host = [0.0] * G
            if isinstance(temperature, torch.Tensor) and temperature.dim() > 0:
                T_rep = temperature.reshape(-1).repeat_interleave(W)
                T_host = temperature.detach().double().cpu().reshape(-1).tolist()
            elif temperature is not None:
                T_host = [float(temperature)] * G
            if self.bias_factor is not None and not all(t > 0.0 and math.isfinite(t) for t in T_host):
                raise ValueError('bias_factor needs temperatures > 0 K')
            super().__init__(model, z[src], pos[src], cell.repeat_interleave(W, dim=0), rep_batch.to(batch.dtype),
                             masses=None if masses is None else masses.reshape(-1)[src], temperature=T_rep, friction=friction,
                             timestep=timestep, fixed=None if fixed is None else fixed[src], generator=generator)
            B = self.n_mol
            self._group_ptr_host = (torch.arange(G + 1, dtype=torch.int32) * W).contiguous()
            self._group_ptr = self._group_ptr_host.to(dev)
            self._mol_ptr_host = self._mol_ptr.cpu()
            self._cv_def = torch.from_numpy(np.repeat(table, W, axis=0)).to(dev).contiguous()                   # [B, 2, 5]
            restraint = np.stack([kappa, centre], axis=-1).astype(np.float32)                                    # [G, W, 2, 2]
            self._restraint = torch.from_numpy(restraint.reshape(B, hip.BIAS_MAX_CVS, 2)).to(dev).contiguous()
            self._hill_par = torch.from_numpy(hill_parameters(n_cv_of_system, widths, height, self.bias_factor, T_host)).to(dev)
            self._hills = torch.zeros(G, capacity, 4, dtype=torch.float32, device=dev)
            self._bias_force = torch.empty(N * W, 3, dtype=torch.float32, device=dev)
            self._cv = torch.zeros(B, hip.BIAS_MAX_CVS, dtype=torch.float32, device=dev)
            self._bias = torch.zeros(B, 2, dtype=torch.float32, device=dev)
            self._status = torch.zeros(B, dtype=torch.int32, device=dev)
            self._model_force = None
            self.n_deposits = 0
            self._deposit_now = False

    # ------------------------------------------------------------------------------------------
    def _evaluate(self):
        """the model's forces and energies at the current positions (touching gradient_force settles the deferred call first, as in
        Dynamics._evaluate), then ONE launch: the biased forces into the driver's own buffer -- which the integrator reads from
        here on -- and, when this step deposits, the walkers' hills.  The launch writes neither position buffer."""
        out = self.model(self.z, self._pos[self._cur], self.cell, self.batch)
        self._model_force = out.gradient_force
        self._energy = out.energy
        deposit, self._deposit_now = self._deposit_now, False
        if deposit:
            self._reserve(self.n_deposits + 1)
        hip.bias_step(self._pos[self._cur], self._model_force, self._mol_ptr, self._mol_ptr_host, self._group_ptr,
                      self._group_ptr_host, self._cv_def, self._restraint, self._hill_par, self._hills, self.n_deposits,
                      hip.BIAS_DEPOSIT if deposit else 0, self._bias_force, self._cv, self._bias, self._status)
        if deposit:
            self.n_deposits += 1
        self._force = self._bias_force

    def _reserve(self, n_deposits: int):
        """room for n_deposits deposits per group: the list is reallocated at twice the capacity and copied on the device"""
        capacity = self._hills.shape[1]
        if n_deposits * self.n_walkers <= capacity:
            return
        while n_deposits * self.n_walkers > capacity:
            capacity *= 2
        grown = torch.zeros(self.n_systems, capacity, 4, dtype=torch.float32, device=self._hills.device)
        grown[:, :self._hills.shape[1]].copy_(self._hills)
        self._hills = grown

    # ------------------------------------------------------------------------------------------
    @property
    def n_hills(self) -> int:
        """hills in every group's list"""
        return self.n_deposits * self.n_walkers

    @property
    def hills(self):
        """per group: (centres fp32 [H, n_cv], heights fp32 [H]) of the deposited hills, in (deposit, walker) order"""
        H = self.n_hills
        return [(self._hills[g, :H, :max(int((self.cvs[g, :, 0] != 0).sum()), 1)].clone(), self._hills[g, :H, 2].clone())
                for g in range(self.n_systems)]

    @property
    def model_forces(self):
        """the model's forces at the current positions, before the bias"""
        self._ensure_state()
        return self._model_force

    @property
    def collective_variables(self):
        self._ensure_state()
        return self._cv.clone()

    @property
    def bias_energy(self):
        self._ensure_state()
        return self._bias[:, 0].clone()

    @property
    def restraint_energy(self):
        self._ensure_state()
        return self._bias[:, 1].clone()

    @property
    def status(self):
        """int32 [B]: bit d set = variable d had no gradient at the last evaluation; hip.BIAS_STATUS_INVALID = the walker's tables
        were refused on the device"""
        self._ensure_state()
        return self._status.clone()

    def _periods(self, g: int):
        return tuple(TWO_PI32 if self.cvs[g, d, 0] == hip.BIAS_TORSION else 0.0 for d in range(hip.BIAS_MAX_CVS))

    def bias_on_grid(self, points) -> torch.Tensor:
        """fp32 [G, M]: V of every group's hills at `points` ([M] for one variable, [M, 2] for two; a tensor or numbers), through
        the kernel's own hill sum"""
        p = torch.as_tensor(points, dtype=torch.float32, device=self._hills.device)
        if p.dim() == 1:
            p = torch.stack([p, torch.zeros_like(p)], dim=1)
        if p.dim() != 2 or p.shape[1] != hip.BIAS_MAX_CVS:
            raise ValueError(f'points: [M] or [M, {hip.BIAS_MAX_CVS}] expected (got {tuple(p.shape)})')
        p = p.contiguous()
        return torch.stack([hip.bias_eval(self._hills, self._hill_par, g, self.n_hills, p, self._periods(g))
                            for g in range(self.n_systems)])

    def free_energy(self, points) -> torch.Tensor:
        """fp32 [G, M]: the free-energy estimate at `points`, -gamma / (gamma - 1) V for well-tempered and -V for plain
        metadynamics, shifted to a minimum of 0 per group"""
        V = self.bias_on_grid(points)
        F = free_energy_factor(self.bias_factor) * V
        return F - F.min(dim=1, keepdim=True).values if F.shape[1] else F

    # ------------------------------------------------------------------------------------------
    def run(self, n_steps: int, record_every: int = 0) -> BiasedTrajectory:
        """Dynamics.run with the bias: every step is model() -> bias_step -> md_step, and nothing in the loop reads the device.
        Deposits are counted by the global step number: run(a); run(b) leaves the bits of run(a + b), and record_every changes no
        bit.  The generator's stream is exactly Dynamics's."""
        n_steps, recorded = self._recorded_steps(n_steps, record_every)
        dev = self._vel.device
        with torch.no_grad():
            self._ensure_state()
            traj = self._new_trajectory(BiasedTrajectory, recorded)
            Rec, B = len(recorded), self.n_mol
            traj.cv = torch.empty(Rec, B, hip.BIAS_MAX_CVS, dtype=torch.float32, device=dev)
            traj.bias_energy = torch.empty(Rec, B, dtype=torch.float32, device=dev)
            traj.restraint_energy = torch.empty(Rec, B, dtype=torch.float32, device=dev)
            n_hills = []
            r = 0
            pending = False
            for k in range(1, n_steps + 1):
                self._deposit_now = self._depositing and (self.step_count + k) % self.pace == 0
                self._advance(pending)
                pending = True
                if k == recorded[r]:
                    self._finish()
                    pending = False
                    self._store_biased(traj, r, n_hills)
                    r += 1
            if n_steps == 0:
                self._store_biased(traj, 0, n_hills)
            self.step_count += n_steps
            traj.n_hills = torch.tensor(n_hills, dtype=torch.int64, device=dev)
        return traj

    def _store_biased(self, traj, r: int, n_hills: list):
        self._store(traj, r)
        traj.cv[r].copy_(self._cv)
        traj.bias_energy[r].copy_(self._bias[:, 0])
        traj.restraint_energy[r].copy_(self._bias[:, 1])
        n_hills.append(self.n_hills)


def free_energy_factor(bias_factor) -> float:
    """F = factor x V: -gamma / (gamma - 1) for well-tempered metadynamics, -1 for plain"""
    return -1.0 if bias_factor is None else -float(bias_factor) / (float(bias_factor) - 1.0)
