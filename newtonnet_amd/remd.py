"""Replica-exchange molecular dynamics (parallel tempering) on the HIP path: G systems x R temperatures are the B = G R molecules of
ONE model() call per step, integrated together by `Dynamics` (BAOAB Langevin, csrc/md.hip), and every `exchange_every` steps one
launch (nnhip_remd_exchange, csrc/remd.hip) attempts a Metropolis swap between every other pair of neighbouring temperatures in
every ladder, with no host round trip of energies, decisions, velocities or noise amplitudes.

A ladder is the R replicas of one system, the consecutive molecules g R .. g R + R - 1 (its slots).  An exchange swaps the
TEMPERATURES of two slots (Sugita and Okamoto 1999): slot s holds rank_of_slot[s], its index into the ladder's temperature list,
positions and forces stay where they are, the velocities of the two slots are rescaled by sqrt(T_new / T_old) and their Langevin
sigma rows are copied from a table.  Pair (k, k + 1) of ranks is accepted with probability min(1, exp((beta_k - beta_{k+1})
(E_k - E_{k+1}))); even attempts try the pairs (0, 1), (2, 3), ..., odd ones (1, 2), (3, 4), ....  The uniform numbers come from
Philox4x32-10 keyed by `exchange_seed` and counted by (attempt, ladder, pair): they are a stream of their own, so the generator's
stream is exactly Dynamics's -- one Maxwell-Boltzmann draw, then one randn per step -- and a pair of seeds reproduces a run bit
for bit.

The acceptance test uses fp32 model energies: E_a - E_b is resolved to one fp32 ulp of |E|, 2 meV for aspirin with the shipped
per-element shifts (|E| = 1.76e4 eV), against k_B T = 26 meV at 300 K.

Not done here: exchanging coordinates instead of temperatures, Hamiltonian exchange, swaps between non-neighbours, adaptive
ladders, replicas of unequal size, compacting or re-ordering the batch, reweighting (WHAM / MBAR), an in-kernel Gaussian generator
for the Langevin noise.

Units: as in newtonnet_amd/dynamics.py (Angstrom, eV, amu, fs, K)."""
from __future__ import annotations

import math

import numpy as np
import torch

from newtonnet_amd import hip
from newtonnet_amd.dynamics import Dynamics, Trajectory, _check_devices, _check_system, langevin_coefficients
from newtonnet_amd.vibrations import K_BOLTZMANN


def check_temperatures(temperatures, n_systems: int) -> np.ndarray:
    """the ladders as fp64 [G, R], refused without touching the device: `temperatures` is [R] (every system the same ladder) or
    [G, R]; positive, finite, non-decreasing along R, 2 <= R <= hip.REMD_MAX_REPLICAS"""
    if isinstance(temperatures, torch.Tensor):
        temperatures = temperatures.detach().cpu().numpy()
    try:
        T = np.array(temperatures, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'temperatures: numbers [R] or [G, R] expected (got {temperatures!r})') from None
    if T.ndim == 1:
        T = np.broadcast_to(T, (n_systems, T.shape[0])).copy()
    if T.ndim != 2 or T.shape[0] != n_systems:
        raise ValueError(f'temperatures: [R] or [{n_systems}, R] expected (got shape {tuple(np.shape(temperatures))})')
    R = T.shape[1]
    if not 2 <= R <= hip.REMD_MAX_REPLICAS:
        raise ValueError(f'temperatures: 2 .. {hip.REMD_MAX_REPLICAS} replicas per ladder expected (got {R})')
    if not (np.isfinite(T).all() and (T > 0.0).all()):
        raise ValueError('temperatures: finite values > 0 K expected')
    if (np.diff(T, axis=1) < 0.0).any():
        raise ValueError('temperatures: a non-decreasing ladder expected')
    return T


def check_exchange_arguments(exchange_every, friction, exchange_seed):
    """(exchange_every, exchange_seed) as ints, refused without touching the device"""
    try:
        ok = int(exchange_every) == exchange_every and exchange_every >= 0 and not isinstance(exchange_every, bool)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'exchange_every: an integer >= 0 expected (got {exchange_every!r})')
    try:
        friction_ok = float(friction) > 0.0 and math.isfinite(float(friction))
    except (TypeError, ValueError):
        friction_ok = False
    if not friction_ok:
        raise ValueError(f'friction: a finite value > 0 per fs expected, an exchange needs a thermostat (got {friction!r})')
    if isinstance(exchange_seed, bool) or not isinstance(exchange_seed, (int, np.integer)) or not 0 <= int(exchange_seed) < 2 ** 64:
        raise ValueError(f'exchange_seed: an int in 0 .. 2^64 - 1 expected (got {exchange_seed!r})')
    return int(exchange_every), int(exchange_seed)


def ladder_coefficients(T: np.ndarray):
    """(dbeta, scale_up, scale_down) fp32 [G, R] of ladders T fp64 [G, R]: entry k belongs to the pair (k, k + 1) -- 1 / (k_B T_k) -
    1 / (k_B T_{k+1}), sqrt(T_{k+1} / T_k) and sqrt(T_k / T_{k+1}), formed in fp64 and rounded once; the last entry of a ladder is
    unused (0, 1, 1)"""
    dbeta, up, down = np.zeros_like(T), np.ones_like(T), np.ones_like(T)
    dbeta[:, :-1] = 1.0 / (K_BOLTZMANN * T[:, :-1]) - 1.0 / (K_BOLTZMANN * T[:, 1:])
    up[:, :-1] = np.sqrt(T[:, 1:] / T[:, :-1])
    down[:, :-1] = np.sqrt(T[:, :-1] / T[:, 1:])
    return dbeta.astype(np.float32), up.astype(np.float32), down.astype(np.float32)


class ReplicaTrajectory(Trajectory):
    """What ReplicaExchange.run recorded: Trajectory's tensors over the B = G R slots (a slot is a continuous trajectory whose
    temperature changes), and

    rank                 int32 [Rec,B]   the rank every slot was integrated under up to that frame (a recorded frame carries the
                                         velocities and the rank from BEFORE an exchange at the same step)
    temperature_of_slot  fp64 [Rec,B]    the ladder temperature of that rank
    exchange_step        int64 [A]       the steps of this call at which an exchange was attempted
    delta, u             fp32 [A,G,R-1]  per pair: (beta_k - beta_{k+1}) (E_k - E_{k+1}) and the uniform number (0 where the pair
                                         was not attempted: the other parity)
    accepted             bool [A,G,R-1]
    """

    def __init__(self, *a):
        super().__init__(*a)
        self.rank = self.exchange_step = self.delta = self.u = self.accepted = None
        self._ladders = None           # fp64 [G, R] on the device

    @property
    def temperature_of_slot(self):
        G, R = self._ladders.shape
        return torch.gather(self._ladders.unsqueeze(0).expand(self.rank.shape[0], G, R), 2,
                            self.rank.view(-1, G, R).long()).reshape(-1, G * R)

    def by_temperature(self):
        """The canonical trajectory at each temperature: dict(pos, vel fp32 [Rec,G,R,n,3], potential_energy, kinetic_energy fp32
        [Rec,G,R], slot int64 [Rec,G,R]) -- entry [f, g, k] is the slot of ladder g that held rank k at frame f.  pos and vel need
        systems of one size (else they are left out)."""
        G, R = self._ladders.shape
        Rec = self.rank.shape[0]
        slot = torch.argsort(self.rank.view(Rec, G, R).long(), dim=2)              # the inverse permutation
        out = dict(slot=slot, potential_energy=torch.gather(self.potential_energy.view(Rec, G, R), 2, slot),
                   kinetic_energy=torch.gather(self.kinetic_energy.view(Rec, G, R), 2, slot))
        N = self.pos.shape[1]
        if N % (G * R) == 0 and bool((self._counts == N // (G * R)).all()):
            n = N // (G * R)
            idx = slot.view(Rec, G, R, 1, 1).expand(Rec, G, R, n, 3)
            out['pos'] = torch.gather(self.pos.view(Rec, G, R, n, 3), 2, idx)
            out['vel'] = torch.gather(self.vel.view(Rec, G, R, n, 3), 2, idx)
        return out


class ReplicaExchange(Dynamics):
    """G systems x R temperatures advanced together on the device, with Metropolis exchanges between neighbouring temperatures.

    model, z, pos, cell, batch, masses, fixed, timestep, generator: as for Dynamics, describing the G systems; each is replicated R
    times, ladder-major (molecule g R + s is replica s of system g), and none of the caller's tensors is modified.  temperatures:
    [R] or [G, R] in K, positive, finite, non-decreasing, 2 <= R <= hip.REMD_MAX_REPLICAS; replica s starts at rank s, with
    Maxwell-Boltzmann velocities at its temperature.  friction (1 / fs) > 0: an exchange needs a thermostat.  exchange_every: an
    exchange is attempted after every step whose global number is a multiple of it (0: never).  exchange_seed: the seed of the
    exchange decisions, separate from `generator`."""

    def __init__(self, model, z, pos, cell, batch, temperatures, exchange_every, friction, timestep=0.5, masses=None, fixed=None,
                 generator=None, exchange_seed=0):
        # ---- everything that can be refused without touching the device
        N, G, timestep, friction = _check_system(model, z, pos, cell, batch, masses, None, fixed, timestep, friction)
        T = check_temperatures(temperatures, G)
        self.exchange_every, self.exchange_seed = check_exchange_arguments(exchange_every, friction, exchange_seed)
        dev = _check_devices(pos, generator, z=z, cell=cell, batch=batch, masses=masses, fixed=fixed)
        R = T.shape[1]
        self.n_systems, self.n_replicas = G, R
        # ---- the replicated batch: the atoms of system g, R times in a row
        with torch.no_grad():
            counts = torch.bincount(batch.long(), minlength=G)
            ptr = torch.zeros(G + 1, dtype=torch.long, device=dev)
            ptr[1:] = torch.cumsum(counts, 0)
            rep_batch = torch.repeat_interleave(torch.arange(G * R, device=dev), counts.repeat_interleave(R))
            rep_ptr = torch.zeros(G * R + 1, dtype=torch.long, device=dev)
            rep_ptr[1:] = torch.cumsum(counts.repeat_interleave(R), 0)
            system = torch.div(rep_batch, R, rounding_mode='floor')
            src = ptr[system] + (torch.arange(rep_batch.numel(), device=dev) - rep_ptr[rep_batch])
            self.ladders = torch.tensor(T, dtype=torch.float64, device=dev)                     # [G, R]
            super().__init__(model, z[src], pos[src], cell.repeat_interleave(R, dim=0), rep_batch.to(batch.dtype),
                             masses=None if masses is None else masses.reshape(-1)[src],
                             temperature=self.ladders.reshape(-1), friction=friction, timestep=timestep,
                             fixed=None if fixed is None else fixed[src], generator=generator)
            B = self.n_mol
            free = None if fixed is None else ~fixed[src]
            # row k: every atom's sigma at rank k of its ladder -- the expression Dynamics forms its own sigma with, so a row copied
            # into sigma is bitwise what a Dynamics at that temperature would hold
            rows = []
            for k in range(R):
                sigma = langevin_coefficients(timestep, friction, self.ladders[:, k].repeat_interleave(R), self.masses, self.batch)[1]
                rows.append(sigma if free is None else sigma * free)
            self._sigma_table = torch.stack(rows).contiguous()
            dbeta, up, down = ladder_coefficients(T)
            self._dbeta, self._scale_up, self._scale_down = (torch.from_numpy(a.reshape(-1)).to(dev) for a in (dbeta, up, down))
            self._ladder_ptr_host = (torch.arange(G + 1, dtype=torch.int32) * R).contiguous()
            self._ladder_ptr = self._ladder_ptr_host.to(dev)
            self._mol_ptr_host = self._mol_ptr.cpu()
            self._stream_id = torch.arange(G, dtype=torch.int32, device=dev)
            self._rank_of_slot = torch.arange(R, dtype=torch.int32, device=dev).repeat(G).contiguous()
            self._slot_of_rank = self._rank_of_slot.clone()
            self._n_attempt = torch.zeros(B, dtype=torch.int32, device=dev)
            self._n_accept = torch.zeros(B, dtype=torch.int32, device=dev)
            self._delta = torch.zeros(B, dtype=torch.float32, device=dev)
            self._u = torch.zeros(B, dtype=torch.float32, device=dev)
            self._accepted = torch.zeros(B, dtype=torch.int32, device=dev)
            self.attempt_count = 0

    # ------------------------------------------------------------------------------------------
    @property
    def rank_of_slot(self):
        """int64 [G, R]: the rank (index into the ladder's temperatures) every slot holds now"""
        return self._rank_of_slot.view(self.n_systems, self.n_replicas).long()

    @property
    def slot_of_rank(self):
        return self._slot_of_rank.view(self.n_systems, self.n_replicas).long()

    @property
    def n_attempt(self):
        return self._n_attempt.view(self.n_systems, self.n_replicas)[:, :-1].long()

    @property
    def n_accept(self):
        return self._n_accept.view(self.n_systems, self.n_replicas)[:, :-1].long()

    @property
    def acceptance(self):
        """fp32 [G, R-1]: accepted / attempted exchanges of every pair since construction (NaN where none was attempted)"""
        return self.n_accept.float() / self.n_attempt.float()

    def _exchange(self):
        """one attempt on the energies just evaluated: self._energy was touched by _evaluate, which settled the deferred call"""
        hip.remd_exchange(self._energy, self._mol_ptr, self._mol_ptr_host, self._ladder_ptr, self._ladder_ptr_host, self._stream_id,
                          self._dbeta, self._scale_up, self._scale_down, self._sigma_table, self._rank_of_slot, self._slot_of_rank,
                          self._vel, self._sigma, self._n_attempt, self._n_accept, self.attempt_count % 2 ** 32, self.exchange_seed,
                          delta_out=self._delta, u_out=self._u, accepted_out=self._accepted)
        self.attempt_count += 1

    def run(self, n_steps: int, record_every: int = 0) -> ReplicaTrajectory:
        """Dynamics.run with exchange attempts: after every step whose global number (step_count) is a multiple of exchange_every
        the fused integrator launch is split, as at a recorded step -- finish, the record if one is due, ONE exchange launch,
        begin -- and nothing in the loop reads the device.  Attempt numbers, and with them the parity, run on across calls:
        run(a); run(b) leaves the bits of run(a + b), and record_every changes no bit."""
        n_steps, recorded = self._recorded_steps(n_steps, record_every)
        G, R, dev = self.n_systems, self.n_replicas, self._vel.device
        steps, deltas, us, accs = [], [], [], []
        with torch.no_grad():
            self._ensure_state()
            traj = self._new_trajectory(ReplicaTrajectory, recorded)
            traj.rank = torch.empty(len(recorded), self.n_mol, dtype=torch.int32, device=dev)
            traj._ladders = self.ladders
            r = 0
            pending = False
            for k in range(1, n_steps + 1):
                self._advance(pending)
                pending = True
                record = k == recorded[r]
                attempt = self.exchange_every > 0 and (self.step_count + k) % self.exchange_every == 0
                if record or attempt:
                    self._finish()
                    pending = False
                if record:
                    self._store(traj, r)
                    traj.rank[r].copy_(self._rank_of_slot)
                    r += 1
                if attempt:
                    self._exchange()
                    steps.append(self.step_count + k)
                    deltas.append(self._delta.clone())
                    us.append(self._u.clone())
                    accs.append(self._accepted.clone())
            if n_steps == 0:
                self._store(traj, 0)
                traj.rank[0].copy_(self._rank_of_slot)
            self.step_count += n_steps

            def log(frames, dtype):
                if not frames:
                    return torch.zeros(0, G, R - 1, dtype=dtype, device=dev)
                return torch.stack(frames).view(-1, G, R)[:, :, :-1].contiguous()
            traj.exchange_step = torch.tensor(steps, dtype=torch.int64, device=dev)
            traj.delta, traj.u, traj.accepted = log(deltas, torch.float32), log(us, torch.float32), log(accs, torch.int32) != 0
        return traj
