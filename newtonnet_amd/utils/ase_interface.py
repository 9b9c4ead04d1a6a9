"""ASE calculator for the MI355X hot path -- mirror of newtonnet/utils/ase_interface.py:18-142.

Same constructor, `implemented_properties`, `calculate()` contract and result shapes as the reference's
MLAseCalculator.  `ase` is optional at import time: when it is installed the class derives from
ase.calculators.calculator.Calculator; otherwise a minimal stand-in base keeps the same attributes
(`results`, `atoms`) so that any object exposing get_atomic_numbers / get_positions(wrap=True) / get_cell /
get_pbc works (this image has no ase; the parity tests drive it with such an object against K1).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from newtonnet_amd.layers.precision import get_precision_by_string
from newtonnet_amd.layers.scalers import get_scaler_by_string
from newtonnet_amd.models.output import (DerivativeProperty, get_aggregator_by_string, get_output_by_string)

try:  # pragma: no cover - ase is not in the build image
    from ase.calculators.calculator import Calculator as _Base
    _HAVE_ASE = True
except Exception:  # noqa: BLE001
    _HAVE_ASE = False

    class _Base:
        """Just enough of ase.calculators.calculator.Calculator for calculate()."""
        def __init__(self, **kwargs):
            self.results = {}
            self.atoms = None
            self.parameters = dict(kwargs)

        def calculate(self, atoms=None, properties=None, system_changes=None):
            self.atoms = atoms


def _current_key(k: str) -> str:
    """Parameter names of the pre-2.0 checkpoint layout (scripts/md17_model/training_1/models/best_model.pt) -> current."""
    k = k.replace('embedding_layer.edge_embedding.frequencies', 'embedding_layers.edge_embedding.embedding.frequencies')
    return k.replace('embedding_layer.', 'embedding_layers.')


class _ReferenceUnpickler(__import__('pickle').Unpickler):
    """Whole-module pickles written by the reference name classes of the `newtonnet` package (and of `les`).  When those
    import, they are used as they are (and converted through state_dict()); when they do not -- this package does not depend
    on the reference -- each missing class becomes an attribute-only nn.Module stand-in: nn.Module's own __setstate__
    restores `_parameters` / `_modules`, which is all state_dict() needs."""
    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except (ImportError, AttributeError):
            if module.split('.')[0] in ('newtonnet', 'les'):
                return type(name, (torch.nn.Module,), {'__module__': module})
            raise


class _ReferencePickle:
    """pickle_module for torch.load (needs Unpickler and load)."""
    __name__ = 'newtonnet_amd_reference_pickle'
    Unpickler = _ReferenceUnpickler

    @staticmethod
    def load(f, **kw):
        return _ReferenceUnpickler(f, **kw).load()


def _is_single(atoms) -> bool:
    return hasattr(atoms, 'get_positions')


class MLAseCalculator(_Base):
    implemented_properties = ['energy', 'free_energy', 'forces', 'stress', 'hessian']
    # the reference additionally lists 'charges', 'bec' (ase_interface.py:19): outside the hot path.  'hessian' is served by
    # NewtonNet.hessian (a method, not an output head: no head surgery for it)

    def __init__(self, model_path, properties: list = None, device: str = None, precision: str = 'float32',
                 skin: float = 0.5, capture: bool = False, **kwargs):
        """
        model_path: path of a whole-module pickle (torch.save(model), trainer.py:219) of a newtonnet_amd NewtonNet,
                    a state_dict file (.pt/.npz with the reference's key names), or a NewtonNet instance.
        properties: subset of implemented_properties; default: what the model predicts.
        device:     'cuda' (default when available).  The HIP path has no CPU implementation.
        precision:  'float32' / 'single' (the HIP path computes in fp32).
        skin:       Verlet skin in Angstrom for the single-structure (MD-loop) path: the neighbor list is built once with
                    cutoff + skin and reused until an atom has moved more than skin / 2; candidates outside the cutoff at a
                    given step contribute exactly zero, so the results are the exact-list results up to fp32 summation order.
                    0 rebuilds the exact list on every call (the reference's behaviour, ase_interface.py:52-81).
        capture:    replay the step of the MD-loop path from a HIP graph (one launch instead of ~45).  Off by default:
                    on ROCm 7.2 / MI355X the replay measured the same 0.43 ms per step as direct launches (the ~45
                    dependent dispatches cost ~8 us each on the GPU either way) and every list rebuild re-captures.
        """
        _Base.__init__(self, **kwargs)
        self.device = torch.device(device) if device is not None else torch.device(
            'cuda' if torch.cuda.is_available() else 'cpu')
        self.dtype = get_precision_by_string(precision)
        self.properties = properties
        self.skin = float(skin)
        self.capture = bool(capture)
        self._md = None          # state of the MD-loop path (list, static buffers, captured graph)
        self.md_stats = {'steps': 0, 'rebuilds': 0}
        self.model = self.load_model(model_path)

    # ------------------------------------------------------------------ ase_interface.py:52-81
    def calculate(self, atoms=None, properties=None, system_changes=None):
        _Base.calculate(self, atoms, self.properties, system_changes)
        if _is_single(atoms) and self.skin > 0 and self.device.type == 'cuda' and 'hessian' not in self.properties:
            return self._calculate_md(atoms)
        if _is_single(atoms):
            atoms = [atoms]
        z, pos, cell, batch = self.format_data(atoms)
        n_frames, n_atoms = len(atoms), len(atoms[0])
        pred = self.model(z, pos, cell, batch)
        if 'energy' in self.properties:
            self.results['energy'] = pred.energy.cpu().detach().numpy().squeeze()
        if 'free_energy' in self.properties:
            self.results['free_energy'] = pred.energy.cpu().detach().numpy().squeeze()
        if 'forces' in self.properties:
            force = pred.gradient_force.cpu().detach().numpy()
            self.results['forces'] = force.reshape(n_frames, n_atoms, 3).squeeze()
        if 'stress' in self.properties:
            stress = pred.stress.cpu().detach().numpy()
            self.results['stress'] = stress[:, [0, 1, 2, 1, 0, 0], [0, 1, 2, 2, 2, 1]].squeeze()
        del pred
        if 'hessian' in self.properties:   # ase_interface.py:75-77, with the per-frame shape the reference intends
            blocks, _ = self.model.hessian(z, pos, cell, batch, blocks=True)
            h = blocks.to(self.dtype).cpu().numpy()
            self.results['hessian'] = h.reshape(n_frames, n_atoms, 3, n_atoms, 3).squeeze()

    def vibrations(self, atoms_or_list, project: bool = True, solver: str = 'lds'):
        """Harmonic analysis of one structure or a list of equally sized ones (NewtonNet.normal_modes): (frequencies
        [n_frames, 3 n_atoms] in cm^-1, imaginary ones negative; modes [n_frames, 3 n_atoms, n_atoms, 3], row k = mode k in
        mass-weighted coordinates), squeezed for one frame.  Masses from atoms.get_masses() when the object has it, else
        standard atomic weights.  solver: 'lds' (structures of up to 42 atoms), 'auto' (larger ones, up to 512 atoms, through the
        blocked solver) or 'blocked', as in NewtonNet.normal_modes.  A method of its own: not a property of calculate()."""
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        n_frames, n_atoms = len(atoms), len(atoms[0])
        if any(len(a) != n_atoms for a in atoms):
            raise ValueError('vibrations: frames of different sizes cannot share one array; call it per frame, or use '
                             'model.normal_modes (packed per molecule)')
        z, pos, cell, batch = self.format_data(atoms)
        masses = None
        if all(hasattr(a, 'get_masses') for a in atoms):
            masses = torch.tensor(np.concatenate([np.asarray(a.get_masses(), dtype=np.float64) for a in atoms]),
                                  dtype=torch.float32, device=pos.device)
        nm = self.model.normal_modes(z, pos, cell, batch, masses=masses, project=project, solver=solver)
        freq = nm.frequencies.cpu().numpy().reshape(n_frames, 3 * n_atoms)
        modes = nm.modes.cpu().numpy().reshape(n_frames, 3 * n_atoms, n_atoms, 3)
        return (freq[0], modes[0]) if n_frames == 1 else (freq, modes)

    def phonons(self, atoms_or_list, supercell, asr: bool = True, solver: str = 'lds'):
        """Phonons of one crystal or a list of crystals (NewtonNet.phonons): a newtonnet_amd.phonons.Phonons over the
        primitive cells given, ready for frequencies(q), band_structure(points, n) and mesh(n1, n2, n3).  supercell: three
        integers, or one triple per structure.  Masses from atoms.get_masses() when the objects have it, else standard atomic
        weights.  The structures may differ in size.  solver: 'lds' (up to 32 atoms per primitive cell), 'auto' or 'blocked' (up
        to 256), as NewtonNet.phonons takes it.  A method of its own: not a property of calculate()."""
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        z, pos, cell, batch = self.format_data(atoms)
        masses = None
        if all(hasattr(a, 'get_masses') for a in atoms):
            masses = torch.tensor(np.concatenate([np.asarray(a.get_masses(), dtype=np.float64) for a in atoms]),
                                  dtype=torch.float32, device=pos.device)
        return self.model.phonons(z, pos.float(), cell.float(), batch, supercell, masses=masses, asr=asr, solver=solver)

    def gruneisen(self, atoms_or_list, supercell, strain='volume', delta: float = 0.01, asr: bool = True, solver: str = 'lds'):
        """Mode Grueneisen parameters of one crystal or a list of crystals (NewtonNet.gruneisen): a newtonnet_amd.gruneisen.Gruneisen
        over the primitive cells given, ready for frequencies(q), band_structure(points, n) and mesh(n1, n2, n3).  strain: 'volume',
        'voigt' or symmetric matrices [K, 3, 3]; delta: the strain step of the central difference.  supercell, masses, solver: as
        phonons() takes them.  A method of its own: not a property of calculate()."""
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        z, pos, cell, batch = self.format_data(atoms)
        masses = None
        if all(hasattr(a, 'get_masses') for a in atoms):
            masses = torch.tensor(np.concatenate([np.asarray(a.get_masses(), dtype=np.float64) for a in atoms]),
                                  dtype=torch.float32, device=pos.device)
        return self.model.gruneisen(z, pos.float(), cell.float(), batch, supercell, strain=strain, delta=delta, masses=masses, asr=asr,
                                    solver=solver)

    def elastic_constants(self, atoms_or_list, supercell, relaxed: bool = True, solver: str = 'lds'):
        """Elastic constants of one crystal or a list of crystals (NewtonNet.elastic_constants): a
        newtonnet_amd.elastic.ElasticConstants over the primitive cells given (C in eV / A^3; .gpa() converts).  supercell:
        three integers, or one triple per structure.  relaxed=True adds the relaxed-ion term (it assumes relaxed atoms).  The
        structures may differ in size.  solver: as NewtonNet.elastic_constants takes it.  A method of its own: not a property of
        calculate()."""
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        z, pos, cell, batch = self.format_data(atoms)
        return self.model.elastic_constants(z, pos.float(), cell.float(), batch, supercell, relaxed=relaxed, solver=solver)

    def sample(self, atoms, n_samples: int, temperature: float, quantum: bool = False, seed=None, solver: str = 'lds'):
        """n_samples geometries of one structure drawn from its harmonic distribution at `temperature` (K), as an
        [n_samples, n_atoms, 3] array in Angstrom (NewtonNet.sample_displacements: classical normal-mode sampling, or Wigner
        sampling with quantum=True).  Masses from atoms.get_masses() when the object has it, else standard atomic weights.
        seed: of the device generator that draws the amplitudes (None: torch's global one).  solver: 'lds' (structures of up to 42
        atoms), 'auto' (larger ones, up to 512 atoms, through the blocked solver and the tiled sampling kernel) or 'blocked', as in
        NewtonNet.sample_displacements."""
        from newtonnet_amd import vibrations as _v
        _v._check_solver(solver)
        z, pos, cell, batch = self.format_data([atoms])
        masses = None
        if hasattr(atoms, 'get_masses'):
            masses = torch.tensor(np.asarray(atoms.get_masses(), dtype=np.float64), dtype=torch.float32, device=pos.device)
        gen = None
        if seed is not None:
            gen = torch.Generator(device=pos.device)
            gen.manual_seed(int(seed))
        out = self.model.sample_displacements(z, pos, cell, batch, n_samples, temperature, quantum=quantum, masses=masses,
                                              generator=gen, solver=solver)
        return out.pos.cpu().numpy().reshape(int(n_samples), len(atoms), 3)

    def run_md(self, atoms_or_list, n_steps: int, timestep: float = 0.5, temperature=None, friction: float = 0.0,
               record_every: int = 0, seed=None, constraints=None, constraint_tolerance: float = 1e-5,
               constraint_max_iter: int = 150):
        """n_steps of molecular dynamics of one structure or a list of equally sized ones, all advanced together on the device
        (NewtonNet.dynamics): timestep in fs, friction in 1 / fs (0: microcanonical; > 0: Langevin at `temperature`, K).  Masses
        from atoms.get_masses() when the objects have it, else standard atomic weights; initial velocities from
        atoms.get_momenta() (amu Angstrom per Angstrom sqrt(amu / eV), ase's unit) when they have it, else Maxwell-Boltzmann at
        `temperature`, or zero without one.  seed: of the device generator behind velocities and noise (None: torch's global one).
        Returns a dict of numpy arrays over the R recorded steps (record_every, 2 record_every, ... and the last; 0: the last
        only): positions and velocities [R, n_frames, n_atoms, 3], energy and kinetic_energy [R, n_frames], step [R]; one
        structure drops the frame axis.  The Atoms objects are not modified.
        constraints: None, 'h-bonds' (every X-H bond length kept at its present value) or (pairs [C,2], lengths [C] or None) with
        atom indices within ONE frame (arrays, lists or tensors on any device), applied to every frame; constraint_tolerance and
        constraint_max_iter as for Dynamics, which has the details.  The dict then has constraint_failures (int32 [n_frames], the
        launches in which a frame's constraint solve failed: 0 for a sound run; one structure drops the frame axis here too)."""
        from newtonnet_amd import dynamics as _d
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        if not atoms:
            raise ValueError('run_md: at least one structure expected')
        n_frames, n_atoms = len(atoms), len(atoms[0])
        if any(len(a) != n_atoms for a in atoms):
            raise ValueError('run_md: frames of different sizes cannot share one array; use model.dynamics (packed per molecule)')
        if int(n_steps) != n_steps or n_steps < 0:
            raise ValueError(f'n_steps: an integer >= 0 expected (got {n_steps!r})')
        if int(record_every) != record_every or record_every < 0:
            raise ValueError(f'record_every: an integer >= 0 expected (got {record_every!r})')
        if not (float(timestep) > 0.0) or not (float(friction) >= 0.0):
            raise ValueError(f'timestep > 0 fs and friction >= 0 per fs expected (got {timestep!r}, {friction!r})')
        if float(friction) > 0.0 and temperature is None:
            raise ValueError('friction > 0 (Langevin dynamics) needs a temperature')
        _d._check_temperature(temperature, n_frames)
        if self.device.type != 'cuda':
            raise RuntimeError('newtonnet_amd dynamics run on an MI355X (ROCm) device only: make the calculator with device="cuda"')
        z, pos, cell, batch = self.format_data(atoms)
        masses = velocities = gen = None
        if all(hasattr(a, 'get_masses') for a in atoms):
            masses = torch.tensor(np.concatenate([np.asarray(a.get_masses(), dtype=np.float64) for a in atoms]),
                                  dtype=torch.float32, device=pos.device)
        if all(hasattr(a, 'get_momenta') for a in atoms):
            p = np.concatenate([np.asarray(a.get_momenta(), dtype=np.float64).reshape(-1, 3) for a in atoms])
            m = masses.cpu().double().numpy() if masses is not None else _d.table_masses(z.cpu()).double().numpy()
            velocities = torch.tensor(p / m[:, None], dtype=torch.float32, device=pos.device)
        if seed is not None:
            gen = torch.Generator(device=pos.device)
            gen.manual_seed(int(seed))
        if isinstance(temperature, (list, tuple, np.ndarray)):
            temperature = torch.tensor(np.asarray(temperature, dtype=np.float64), dtype=torch.float32, device=pos.device)
        kw = {}
        if constraints is not None:
            if not isinstance(constraints, str):
                pairs, lengths = constraints
                pairs, lengths = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (pairs, lengths))
                pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
                if pairs.size and (pairs.min() < 0 or pairs.max() >= n_atoms):
                    raise ValueError(f'constraints: atom indices within one frame (0 .. {n_atoms - 1}) expected')
                pairs = (pairs[None, :, :] + n_atoms * np.arange(n_frames)[:, None, None]).reshape(-1, 2)
                if lengths is not None:
                    lengths = torch.from_numpy(np.tile(np.asarray(lengths, dtype=np.float32).reshape(-1), n_frames))
                constraints = (torch.from_numpy(pairs), lengths)
            kw = dict(constraints=constraints, constraint_tolerance=constraint_tolerance, constraint_max_iter=constraint_max_iter)
        dyn = self.model.dynamics(z, pos.float(), cell.float(), batch, masses=masses, velocities=velocities, temperature=temperature,
                                  friction=friction, timestep=timestep, generator=gen, **kw)
        traj = dyn.run(int(n_steps), int(record_every))
        R = traj.step.numel()
        out = dict(positions=traj.pos.cpu().numpy().reshape(R, n_frames, n_atoms, 3),
                   velocities=traj.vel.cpu().numpy().reshape(R, n_frames, n_atoms, 3),
                   energy=traj.potential_energy.cpu().numpy(), kinetic_energy=traj.kinetic_energy.cpu().numpy(),
                   step=traj.step.cpu().numpy())
        if constraints is not None:
            out['constraint_failures'] = dyn.constraint_failures.cpu().numpy()
        if n_frames == 1:
            for k in ('positions', 'velocities', 'energy', 'kinetic_energy'):
                out[k] = out[k][:, 0]
            if 'constraint_failures' in out:
                out['constraint_failures'] = out['constraint_failures'][0]
        return out

    def run_npt(self, atoms_or_list, n_steps: int, pressure, temperature, timestep: float = 0.5, friction: float = 0.0,
                compressibility: float = 4.5e-5, barostat_time: float = 1000.0, record_every: int = 0, seed=None):
        """n_steps of constant-pressure molecular dynamics of one periodic structure or a list of equally sized ones, all advanced
        together on the device (NewtonNet.constant_pressure: isotropic stochastic cell rescaling inside BAOAB).  pressure in bar
        and temperature in K (a number, or one value per structure), compressibility in 1 / bar, barostat_time and timestep in
        fs, friction in 1 / fs.  Masses, initial velocities and seed as in run_md.  The calculator's model needs a virial or
        stress head (properties with 'stress').  Returns run_md's dict and cell [R, n_frames, 3, 3], volume (Angstrom^3),
        pressure (bar: the internal pressure of the recorded state) and density (g / cm^3) [R, n_frames]; one structure drops
        the frame axis.  The Atoms objects are not modified."""
        from newtonnet_amd import dynamics as _d
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        if not atoms:
            raise ValueError('run_npt: at least one structure expected')
        n_frames, n_atoms = len(atoms), len(atoms[0])
        if any(len(a) != n_atoms for a in atoms):
            raise ValueError('run_npt: frames of different sizes cannot share one array; use model.constant_pressure (packed per '
                             'system)')
        if int(n_steps) != n_steps or n_steps < 0:
            raise ValueError(f'n_steps: an integer >= 0 expected (got {n_steps!r})')
        if int(record_every) != record_every or record_every < 0:
            raise ValueError(f'record_every: an integer >= 0 expected (got {record_every!r})')
        if temperature is None:
            raise ValueError('run_npt needs a temperature')
        if self.device.type != 'cuda':
            raise RuntimeError('newtonnet_amd dynamics run on an MI355X (ROCm) device only: make the calculator with device="cuda"')
        z, pos, cell, batch = self.format_data(atoms)
        masses = velocities = gen = None
        if all(hasattr(a, 'get_masses') for a in atoms):
            masses = torch.tensor(np.concatenate([np.asarray(a.get_masses(), dtype=np.float64) for a in atoms]),
                                  dtype=torch.float32, device=pos.device)
        if all(hasattr(a, 'get_momenta') for a in atoms):
            p = np.concatenate([np.asarray(a.get_momenta(), dtype=np.float64).reshape(-1, 3) for a in atoms])
            m = masses.cpu().double().numpy() if masses is not None else _d.table_masses(z.cpu()).double().numpy()
            velocities = torch.tensor(p / m[:, None], dtype=torch.float32, device=pos.device)
        if seed is not None:
            gen = torch.Generator(device=pos.device)
            gen.manual_seed(int(seed))
        per_frame = [torch.tensor(np.asarray(v, dtype=np.float64), dtype=torch.float32, device=pos.device)
                     if isinstance(v, (list, tuple, np.ndarray)) else v for v in (pressure, temperature)]
        dyn = self.model.constant_pressure(z, pos.float(), cell.float(), batch, per_frame[0], per_frame[1], masses=masses,
                                           velocities=velocities, friction=friction, timestep=timestep,
                                           compressibility=compressibility, barostat_time=barostat_time, generator=gen)
        traj = dyn.run(int(n_steps), int(record_every))
        R = traj.step.numel()
        out = dict(positions=traj.pos.cpu().numpy().reshape(R, n_frames, n_atoms, 3),
                   velocities=traj.vel.cpu().numpy().reshape(R, n_frames, n_atoms, 3),
                   energy=traj.potential_energy.cpu().numpy(), kinetic_energy=traj.kinetic_energy.cpu().numpy(),
                   cell=traj.cell.cpu().numpy(), volume=traj.volume.cpu().numpy(), pressure=traj.pressure.cpu().numpy(),
                   density=traj.density.cpu().numpy(), step=traj.step.cpu().numpy())
        if n_frames == 1:
            for k in out:
                if k != 'step':
                    out[k] = out[k][:, 0]
        return out

    def run_remd(self, atoms_or_list, temperatures, n_steps: int, exchange_every: int, friction: float, timestep: float = 0.5,
                 record_every: int = 0, seed=None, exchange_seed: int = 0):
        """n_steps of replica-exchange molecular dynamics (NewtonNet.replica_exchange) of one structure or a list of G equally
        sized ones: each is replicated over the R `temperatures` (K; [R], or [G, R]: one ladder per structure), all G R replicas
        advance together on the device (Langevin, friction in 1 / fs, > 0) and every exchange_every steps neighbouring temperatures
        attempt a Metropolis swap (0: never).  Masses from atoms.get_masses() when the objects have it; initial velocities are
        Maxwell-Boltzmann at each replica's temperature.  seed: of the device generator behind velocities and noise (None:
        torch's global one); exchange_seed: of the exchange decisions.  Returns a dict of numpy arrays over the Rec recorded steps,
        per SLOT (a continuous trajectory whose temperature changes): positions, velocities [Rec, G, R, n_atoms, 3], energy,
        kinetic_energy [Rec, G, R], rank int32 and temperature [Rec, G, R], step [Rec]; per TEMPERATURE, gathered by rank:
        positions_by_temperature, velocities_by_temperature, energy_by_temperature, kinetic_energy_by_temperature; the exchange log
        exchange_step [A], delta, u, accepted [A, G, R-1]; and acceptance [G, R-1].  One structure drops the G axis.  The Atoms
        objects are not modified."""
        from newtonnet_amd import dynamics as _d
        from newtonnet_amd import remd as _x
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        if not atoms:
            raise ValueError('run_remd: at least one structure expected')
        G, n_atoms = len(atoms), len(atoms[0])
        if any(len(a) != n_atoms for a in atoms):
            raise ValueError('run_remd: frames of different sizes cannot share one array; use model.replica_exchange (packed per '
                             'molecule)')
        _d.Dynamics._recorded_steps(n_steps, record_every)
        if not (float(timestep) > 0.0):
            raise ValueError(f'timestep > 0 fs expected (got {timestep!r})')
        T = _x.check_temperatures(temperatures, G)
        _x.check_exchange_arguments(exchange_every, friction, exchange_seed)
        if self.device.type != 'cuda':
            raise RuntimeError('newtonnet_amd dynamics run on an MI355X (ROCm) device only: make the calculator with device="cuda"')
        z, pos, cell, batch = self.format_data(atoms)
        masses = gen = None
        if all(hasattr(a, 'get_masses') for a in atoms):
            masses = torch.tensor(np.concatenate([np.asarray(a.get_masses(), dtype=np.float64) for a in atoms]),
                                  dtype=torch.float32, device=pos.device)
        if seed is not None:
            gen = torch.Generator(device=pos.device)
            gen.manual_seed(int(seed))
        rex = self.model.replica_exchange(z, pos.float(), cell.float(), batch, T, exchange_every, friction, timestep=timestep,
                                          masses=masses, generator=gen, exchange_seed=exchange_seed)
        traj = rex.run(int(n_steps), int(record_every))
        Rec, R = traj.step.numel(), T.shape[1]
        by_t = traj.by_temperature()
        out = dict(positions=traj.pos.cpu().numpy().reshape(Rec, G, R, n_atoms, 3),
                   velocities=traj.vel.cpu().numpy().reshape(Rec, G, R, n_atoms, 3),
                   energy=traj.potential_energy.cpu().numpy().reshape(Rec, G, R),
                   kinetic_energy=traj.kinetic_energy.cpu().numpy().reshape(Rec, G, R),
                   rank=traj.rank.cpu().numpy().reshape(Rec, G, R),
                   temperature=traj.temperature_of_slot.cpu().numpy().reshape(Rec, G, R),
                   positions_by_temperature=by_t['pos'].cpu().numpy(), velocities_by_temperature=by_t['vel'].cpu().numpy(),
                   energy_by_temperature=by_t['potential_energy'].cpu().numpy(),
                   kinetic_energy_by_temperature=by_t['kinetic_energy'].cpu().numpy(),
                   delta=traj.delta.cpu().numpy(), u=traj.u.cpu().numpy(), accepted=traj.accepted.cpu().numpy(),
                   acceptance=rex.acceptance.cpu().numpy())
        if G == 1:
            for k in ('positions', 'velocities', 'energy', 'kinetic_energy', 'rank', 'temperature', 'positions_by_temperature',
                      'velocities_by_temperature', 'energy_by_temperature', 'kinetic_energy_by_temperature'):
                out[k] = out[k][:, 0]
            for k in ('delta', 'u', 'accepted'):
                out[k] = out[k][:, 0]
            out['acceptance'] = out['acceptance'][0]
        out['step'], out['exchange_step'] = traj.step.cpu().numpy(), traj.exchange_step.cpu().numpy()
        return out

    def run_metad(self, atoms_or_list, cvs, n_steps: int, temperature, friction: float, hill_height: float, hill_width, pace: int,
                  bias_factor=None, walkers: int = 1, restraint_k=None, restraint_center=None, timestep: float = 0.5,
                  record_every: int = 0, seed=None, hill_capacity: int = 1024):
        """n_steps of biased molecular dynamics (NewtonNet.metadynamics) of one structure or a list of G equally sized ones: each
        is replicated over `walkers` walkers that share one list of Gaussian hills on the collective variables `cvs` (0 .. 2 of
        ('distance', i, j), ('angle', i, j, k), ('torsion', i, j, k, l); one list for all structures or one per structure), all G W
        walkers advance together on the device and every `pace` steps each deposits a hill of hill_height (eV; well-tempered with
        bias_factor > 1) and hill_width (per variable).  pace = 0 or hill_height = 0 with restraint_k / restraint_center (they
        broadcast to [G, W, n_cv]) is umbrella sampling.  Masses from atoms.get_masses() when the objects have it.  seed: of the
        device generator behind velocities and noise (None: torch's global one).  Returns a dict of numpy arrays over the Rec
        recorded steps: positions, velocities [Rec, G, W, n_atoms, 3], energy (the model's), kinetic_energy, bias_energy,
        restraint_energy [Rec, G, W], cv [Rec, G, W, 2], n_hills, step [Rec], and the hills hill_centers [G, H, 2], hill_heights
        [G, H].  One structure drops the G axis.  The Atoms objects are not modified."""
        from newtonnet_amd import dynamics as _d
        from newtonnet_amd import metadynamics as _m
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        if not atoms:
            raise ValueError('run_metad: at least one structure expected')
        G, n_atoms = len(atoms), len(atoms[0])
        if any(len(a) != n_atoms for a in atoms):
            raise ValueError('run_metad: frames of different sizes cannot share one array; use model.metadynamics (packed per '
                             'molecule)')
        _d.Dynamics._recorded_steps(n_steps, record_every)
        if not (float(timestep) > 0.0):
            raise ValueError(f'timestep > 0 fs expected (got {timestep!r})')
        table = _m.check_cvs(cvs, [n_atoms] * G)
        n_cv = max(int((table[g, :, 0] != 0).sum()) for g in range(G))
        W = _m.check_bias_arguments(n_cv, temperature, friction, hill_height, hill_width, pace, bias_factor, walkers, restraint_k,
                                    restraint_center, hill_capacity, G)[4]
        if self.device.type != 'cuda':
            raise RuntimeError('newtonnet_amd dynamics run on an MI355X (ROCm) device only: make the calculator with device="cuda"')
        z, pos, cell, batch = self.format_data(atoms)
        masses = gen = None
        if all(hasattr(a, 'get_masses') for a in atoms):
            masses = torch.tensor(np.concatenate([np.asarray(a.get_masses(), dtype=np.float64) for a in atoms]),
                                  dtype=torch.float32, device=pos.device)
        if seed is not None:
            gen = torch.Generator(device=pos.device)
            gen.manual_seed(int(seed))
        meta = self.model.metadynamics(z, pos.float(), cell.float(), batch, cvs, temperature, friction, hill_height, hill_width, pace,
                                       bias_factor=bias_factor, walkers=walkers, restraint_k=restraint_k,
                                       restraint_center=restraint_center, timestep=timestep, masses=masses, generator=gen,
                                       hill_capacity=hill_capacity)
        traj = meta.run(int(n_steps), int(record_every))
        Rec, H = traj.step.numel(), meta.n_hills
        out = dict(positions=traj.pos.cpu().numpy().reshape(Rec, G, W, n_atoms, 3),
                   velocities=traj.vel.cpu().numpy().reshape(Rec, G, W, n_atoms, 3),
                   energy=traj.potential_energy.cpu().numpy().reshape(Rec, G, W),
                   kinetic_energy=traj.kinetic_energy.cpu().numpy().reshape(Rec, G, W),
                   bias_energy=traj.bias_energy.cpu().numpy().reshape(Rec, G, W),
                   restraint_energy=traj.restraint_energy.cpu().numpy().reshape(Rec, G, W),
                   cv=traj.cv.cpu().numpy().reshape(Rec, G, W, 2),
                   hill_centers=meta._hills[:, :H, :2].cpu().numpy(), hill_heights=meta._hills[:, :H, 2].cpu().numpy())
        if G == 1:
            for k in ('positions', 'velocities', 'energy', 'kinetic_energy', 'bias_energy', 'restraint_energy', 'cv'):
                out[k] = out[k][:, 0]
            out['hill_centers'], out['hill_heights'] = out['hill_centers'][0], out['hill_heights'][0]
        out['step'], out['n_hills'] = traj.step.cpu().numpy(), traj.n_hills.cpu().numpy()
        return out

    def run_pimd(self, atoms_or_list, n_beads: int, temperature, n_steps: int, timestep: float = 0.25,
                 centroid_friction: float = 0.0, mode_friction: float = 1.0, record_every: int = 0, seed=None):
        """n_steps of path-integral molecular dynamics (NewtonNet.path_integral) of one structure or a list of G equally sized ones:
        each becomes a ring polymer of n_beads beads starting coincident at the structure, all G n_beads beads advance together on
        the device at `temperature` (K; a number or [G]).  centroid_friction (1 / fs) and mode_friction (dimensionless): both 0 =
        RPMD, centroid 0 = thermostatted RPMD, both > 0 = PILE.  Masses from atoms.get_masses() when the objects have it.  seed: of
        the device generator behind the initial velocities and the noise (None: torch's global one).  Returns a dict of numpy
        arrays over the Rec recorded steps: positions, velocities, mode_positions, mode_velocities [Rec, G, P, n_atoms, 3], energy
        [Rec, G, P], potential, kinetic_virial, kinetic_primitive, ring_polymer_energy [Rec, G], centroid [Rec, G, n_atoms, 3],
        radius_of_gyration [Rec, G, n_atoms], step [Rec].  One structure drops the G axis.  The Atoms objects are not modified."""
        from newtonnet_amd import dynamics as _d
        from newtonnet_amd import pimd as _p
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        if not atoms:
            raise ValueError('run_pimd: at least one structure expected')
        G, n_atoms = len(atoms), len(atoms[0])
        if any(len(a) != n_atoms for a in atoms):
            raise ValueError('run_pimd: frames of different sizes cannot share one array; use model.path_integral (packed per '
                             'molecule)')
        _d.Dynamics._recorded_steps(n_steps, record_every)
        if not (float(timestep) > 0.0):
            raise ValueError(f'timestep > 0 fs expected (got {timestep!r})')
        P = _p.check_beads(n_beads)
        _p.check_temperature(temperature, G)
        _p.check_frictions(centroid_friction, mode_friction)
        if self.device.type != 'cuda':
            raise RuntimeError('newtonnet_amd dynamics run on an MI355X (ROCm) device only: make the calculator with device="cuda"')
        z, pos, cell, batch = self.format_data(atoms)
        masses = gen = None
        if all(hasattr(a, 'get_masses') for a in atoms):
            masses = torch.tensor(np.concatenate([np.asarray(a.get_masses(), dtype=np.float64) for a in atoms]),
                                  dtype=torch.float32, device=pos.device)
        if seed is not None:
            gen = torch.Generator(device=pos.device)
            gen.manual_seed(int(seed))
        pi = self.model.path_integral(z, pos.float(), cell.float(), batch, P, temperature, timestep=timestep,
                                      centroid_friction=centroid_friction, mode_friction=mode_friction, masses=masses, generator=gen)
        traj = pi.run(int(n_steps), int(record_every))
        Rec = traj.step.numel()
        out = dict(positions=traj.pos.cpu().numpy().reshape(Rec, G, P, n_atoms, 3),
                   velocities=traj.vel.cpu().numpy().reshape(Rec, G, P, n_atoms, 3),
                   mode_positions=traj.mode_pos.cpu().numpy().reshape(Rec, G, P, n_atoms, 3),
                   mode_velocities=traj.mode_vel.cpu().numpy().reshape(Rec, G, P, n_atoms, 3),
                   energy=traj.potential_energy.cpu().numpy().reshape(Rec, G, P),
                   potential=traj.potential.cpu().numpy(), kinetic_virial=traj.kinetic_virial.cpu().numpy(),
                   kinetic_primitive=traj.kinetic_primitive.cpu().numpy(),
                   ring_polymer_energy=traj.ring_polymer_energy.cpu().numpy(),
                   centroid=traj.centroid.cpu().numpy().reshape(Rec, G, n_atoms, 3),
                   radius_of_gyration=traj.radius_of_gyration.cpu().numpy().reshape(Rec, G, n_atoms))
        if G == 1:
            out = {k: v[:, 0] for k, v in out.items()}
        out['step'] = traj.step.cpu().numpy()
        return out

    def relax(self, atoms_or_list, fmax: float = 0.01, max_steps: int = 500, memory: int = 16, maxstep: float = 0.2,
              alpha: float = 70.0, check_every: int = 10, fixed=None, form: str = 'wave', wg_min_atoms=None):
        """Relax one structure or a list of equally sized ones to a minimum, all stepped together on the device
        (NewtonNet.relaxation): L-BFGS without line search in ase.optimize.LBFGS's convention, until the largest atomic force of a
        structure is below fmax (eV / Angstrom) or max_steps steps have been taken.  fixed: bool array [n_atoms], the same atoms
        held in every structure.  form, wg_min_atoms: the launch form of NewtonNet.relaxation ('wave', 'workgroup' for large
        structures, 'auto').  Returns a dict of numpy arrays: positions [n_frames, n_atoms, 3], energy, fmax, converged,
        n_steps [n_frames]; one structure drops the frame axis.  The Atoms objects are not modified."""
        from newtonnet_amd import relax as _r
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        if not atoms:
            raise ValueError('relax: at least one structure expected')
        n_frames, n_atoms = len(atoms), len(atoms[0])
        if any(len(a) != n_atoms for a in atoms):
            raise ValueError('relax: frames of different sizes cannot share one array; use model.relaxation (packed per molecule)')
        _r.check_arguments(fmax, memory, maxstep, alpha)
        _r.check_run_arguments(max_steps, check_every, 0)
        _r.check_form(form, wg_min_atoms)
        if fixed is not None:
            fixed = np.asarray(fixed)
            if fixed.dtype != np.bool_ or fixed.shape != (n_atoms,):
                raise ValueError(f'fixed: a bool array [{n_atoms}] expected')
        if self.device.type != 'cuda':
            raise RuntimeError('newtonnet_amd relaxations run on an MI355X (ROCm) device only: make the calculator with device="cuda"')
        z, pos, cell, batch = self.format_data(atoms)
        held = None if fixed is None else torch.from_numpy(np.tile(fixed, n_frames)).to(pos.device)
        rel = self.model.relaxation(z, pos.float(), cell.float(), batch, fmax=fmax, memory=memory, maxstep=maxstep, alpha=alpha,
                                    fixed=held, form=form, wg_min_atoms=wg_min_atoms)
        res = rel.run(int(max_steps), int(check_every))
        out = dict(positions=res.pos.cpu().numpy().reshape(n_frames, n_atoms, 3), energy=res.energy.cpu().numpy(),
                   fmax=res.fmax.cpu().numpy(), converged=res.converged.cpu().numpy(), n_steps=res.n_steps.cpu().numpy())
        if n_frames == 1:
            out = {k: v[0] for k, v in out.items()}
        return out

    def relax_cell(self, atoms_or_list, fmax: float = 0.01, max_steps: int = 500, memory: int = 16, maxstep: float = 0.2,
                   alpha: float = 70.0, pressure=0.0, mask=None, hydrostatic: bool = False, constant_volume: bool = False,
                   cell_factor=None, check_every: int = 10, fixed=None, form: str = 'wave', wg_min_atoms=None):
        """Relax the atoms and the cell of one periodic structure or a list of equally sized ones, all stepped together on the
        device (NewtonNet.cell_relaxation: ASE's UnitCellFilter under L-BFGS), until the largest generalised force of a structure
        (atoms and cell rows alike) is below fmax (eV / Angstrom) or max_steps steps have been taken.  pressure in bar (a number,
        or one value per structure); mask: six 0/1 flags xx, yy, zz, yz, xz, xy; fixed: bool array [n_atoms], the same atoms held
        (at their scaled positions) in every structure; form, wg_min_atoms: the launch form of NewtonNet.cell_relaxation ('wave',
        'workgroup' for large structures, 'auto').  The calculator's model needs a virial or stress head (properties with
        'stress').  Returns a dict of numpy arrays: positions [n_frames, n_atoms, 3], cell and stress (bar) [n_frames, 3, 3],
        volume, energy, enthalpy, fmax, converged, failed, n_steps [n_frames]; one structure drops the frame axis.  The Atoms
        objects are not modified."""
        from newtonnet_amd import cellrelax as _c
        from newtonnet_amd import relax as _r
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        if not atoms:
            raise ValueError('relax_cell: at least one structure expected')
        n_frames, n_atoms = len(atoms), len(atoms[0])
        if any(len(a) != n_atoms for a in atoms):
            raise ValueError('relax_cell: frames of different sizes cannot share one array; use model.cell_relaxation (packed per '
                             'system)')
        _r.check_arguments(fmax, memory, maxstep, alpha)
        _r.check_run_arguments(max_steps, check_every, 0)
        if isinstance(pressure, (list, tuple, np.ndarray)):
            pressure = torch.tensor(np.asarray(pressure, dtype=np.float64))
        _c.check_cell_arguments(n_frames, pressure, mask, hydrostatic, constant_volume, cell_factor)
        _c.check_model(self.model, 'relax_cell')
        _r.check_form(form, wg_min_atoms)
        if fixed is not None:
            fixed = np.asarray(fixed)
            if fixed.dtype != np.bool_ or fixed.shape != (n_atoms,):
                raise ValueError(f'fixed: a bool array [{n_atoms}] expected')
        if self.device.type != 'cuda':
            raise RuntimeError('newtonnet_amd relaxations run on an MI355X (ROCm) device only: make the calculator with device="cuda"')
        z, pos, cell, batch = self.format_data(atoms)
        held = None if fixed is None else torch.from_numpy(np.tile(fixed, n_frames)).to(pos.device)
        rel = self.model.cell_relaxation(z, pos.float(), cell.float(), batch, fmax=fmax, memory=memory, maxstep=maxstep, alpha=alpha,
                                         pressure=pressure, mask=mask, hydrostatic=hydrostatic, constant_volume=constant_volume,
                                         cell_factor=cell_factor, fixed=held, form=form, wg_min_atoms=wg_min_atoms)
        res = rel.run(int(max_steps), int(check_every))
        out = dict(positions=res.pos.cpu().numpy().reshape(n_frames, n_atoms, 3), cell=res.cell.cpu().numpy(),
                   stress=res.stress.cpu().numpy(), volume=res.volume.cpu().numpy(), energy=res.energy.cpu().numpy(),
                   enthalpy=res.enthalpy.cpu().numpy(), fmax=res.fmax.cpu().numpy(), converged=res.converged.cpu().numpy(),
                   failed=res.failed.cpu().numpy(), n_steps=res.n_steps.cpu().numpy())
        if n_frames == 1:
            out = {k: v[0] for k, v in out.items()}
        return out

    def neb(self, images_or_list_of_bands, spring: float = 0.1, fmax: float = 0.05, max_steps: int = 500, climb: bool = True,
            climb_below=None, dt: float = 0.1, dt_max: float = 1.0, maxstep: float = 0.2, check_every: int = 10, fixed=None):
        """Nudged-elastic-band saddle search of one band (a list of Atoms-like images in path order, the first and last being the
        fixed endpoints) or a list of bands, all stepped together on the device (NewtonNet.band): improved tangents, FIRE, a
        climbing image switched on below climb_below (None: 5 fmax), until the largest NEB force of a band is below fmax (eV /
        Angstrom) or max_steps steps have been taken.  Every image of a band has the same atoms; bands may differ.  fixed: bool
        array [n_atoms] (only when all bands have n_atoms atoms per image), the same atoms held in every image.  Returns a dict of
        numpy arrays: positions (per band [n_images, n_atoms, 3]), energy (per band [n_images]), fmax, converged, climbing,
        n_steps, saddle_image (index within the band), barrier_forward, barrier_reverse [n_bands]; one band drops the band axis,
        several bands give lists for positions and energy.  The Atoms objects are not modified."""
        from newtonnet_amd import neb as _n
        from newtonnet_amd import relax as _r
        arg = list(images_or_list_of_bands)
        if not arg:
            raise ValueError('neb: at least one band expected')
        single = _is_single(arg[0])
        bands = [arg] if single else [list(b) for b in arg]
        counts = [len(b) for b in bands]
        for k, b in enumerate(bands):
            if not 3 <= len(b) <= _n.hip.NEB_MAX_IMAGES:
                raise ValueError(f'neb: band {k} has {len(b)} images (3 .. {_n.hip.NEB_MAX_IMAGES} expected)')
            if any(len(a) != len(b[0]) for a in b):
                raise ValueError(f'neb: the images of band {k} have different sizes')
        _n.check_arguments(spring, fmax, climb_below, dt, dt_max, maxstep)
        _r.check_run_arguments(max_steps, check_every, 0)
        sizes = [len(b[0]) for b in bands]
        if fixed is not None:
            fixed = np.asarray(fixed)
            if fixed.dtype != np.bool_ or any(fixed.shape != (n,) for n in sizes):
                raise ValueError(f'fixed: a bool array [{sizes[0]}] expected, and every band with that many atoms per image')
        if self.device.type != 'cuda':
            raise RuntimeError('newtonnet_amd band searches run on an MI355X (ROCm) device only: make the calculator with '
                               'device="cuda"')
        z, pos, cell, batch = self.format_data([a for b in bands for a in b])
        held = None if fixed is None else torch.from_numpy(np.tile(fixed, sum(counts))).to(pos.device)
        band = self.model.band(z, pos.float(), cell.float(), batch, counts, spring=spring, fmax=fmax, climb=climb,
                               climb_below=climb_below, fixed=held, dt=dt, dt_max=dt_max, maxstep=maxstep)
        res = band.run(int(max_steps), int(check_every))
        p, e = res.pos.cpu().numpy(), res.energy.cpu().numpy()
        first = np.concatenate([[0], np.cumsum(counts)])
        atom0 = np.concatenate([[0], np.cumsum([c * n for c, n in zip(counts, sizes)])])
        out = dict(positions=[p[atom0[k]:atom0[k + 1]].reshape(counts[k], sizes[k], 3) for k in range(len(bands))],
                   energy=[e[first[k]:first[k + 1]] for k in range(len(bands))], fmax=res.fmax.cpu().numpy(),
                   converged=res.converged.cpu().numpy(), climbing=res.climbing.cpu().numpy(), n_steps=res.n_steps.cpu().numpy(),
                   saddle_image=res.saddle_image.cpu().numpy() - first[:-1], barrier_forward=res.barrier_forward.cpu().numpy(),
                   barrier_reverse=res.barrier_reverse.cpu().numpy())
        if single:
            out = {k: v[0] for k, v in out.items()}
        return out

    def irc(self, atoms_or_list, direction=None, max_steps: int = 1000, speed: float = 0.02, error_target: float = 1.5e-3,
            timestep: float = 0.25, timestep_min: float = 0.01, timestep_max: float = 2.0, initial_displacement: float = 0.1,
            fmax: float = 0.01, check_every: int = 10, record_every: int = 1, fixed=None):
        """Follow the intrinsic reaction coordinate from one saddle geometry or a list of equally sized ones down both sides, all
        paths stepped together on the device (NewtonNet.reaction_path: damped velocity Verlet, one force evaluation and one launch
        per step), until every path has stopped or max_steps steps have been taken.  direction: array [n_atoms, 3] (one structure)
        or [n_frames, n_atoms, 3], or None for the lowest normal mode of every structure (a structure without an imaginary mode
        is refused).  fixed: bool array [n_atoms], the same atoms held in every structure.  Returns a dict; per structure
        `images` is the stitched path as a list of copies of its Atoms -- the backward branch reversed, the saddle, the forward
        branch, every record_every-th step (0: the end points alone) -- with info['energy'] (eV) and info['arc_length']
        (amu^1/2 Angstrom, negative on the backward branch) set; `arc`, `energy` [K] and `positions` [K, n_atoms, 3] hold the same
        as numpy arrays; status, n_steps, fmax, arc_length [n_frames, 2] describe the forward and the backward branch.  One
        structure drops the frame axis.  The Atoms objects passed in are not modified."""
        import copy
        from newtonnet_amd import irc as _i
        from newtonnet_amd import relax as _r
        single = _is_single(atoms_or_list)
        atoms = [atoms_or_list] if single else list(atoms_or_list)
        if not atoms:
            raise ValueError('irc: at least one structure expected')
        n_frames, n_atoms = len(atoms), len(atoms[0])
        if any(len(a) != n_atoms for a in atoms):
            raise ValueError('irc: frames of different sizes cannot share one array; use model.reaction_path (packed per molecule)')
        _i.check_arguments(speed, error_target, timestep, timestep_min, timestep_max, initial_displacement, fmax)
        _r.check_run_arguments(max_steps, check_every, record_every)
        if fixed is not None:
            fixed = np.asarray(fixed)
            if fixed.dtype != np.bool_ or fixed.shape != (n_atoms,):
                raise ValueError(f'fixed: a bool array [{n_atoms}] expected')
        if direction is not None:
            direction = np.asarray(direction, dtype=np.float32)
            if direction.shape not in ((n_frames, n_atoms, 3),) + (((n_atoms, 3),) if n_frames == 1 else ()):
                raise ValueError(f'direction: an array [{n_frames}, {n_atoms}, 3] expected (got {direction.shape})')
        if self.device.type != 'cuda':
            raise RuntimeError('newtonnet_amd reaction paths run on an MI355X (ROCm) device only: make the calculator with '
                               'device="cuda"')
        z, pos, cell, batch = self.format_data(atoms)
        held = None if fixed is None else torch.from_numpy(np.tile(fixed, n_frames)).to(pos.device)
        along = None if direction is None else torch.from_numpy(direction.reshape(-1, 3).copy()).to(pos.device)
        path = self.model.reaction_path(z, pos.float(), cell.float(), batch, direction=along, both=True, speed=speed,
                                        error_target=error_target, timestep=timestep, timestep_min=timestep_min,
                                        timestep_max=timestep_max, initial_displacement=initial_displacement, fmax=fmax, fixed=held)
        res = path.run(int(max_steps), int(check_every), int(record_every))
        out = dict(images=[], arc=[], energy=[], positions=[])
        for b, a in enumerate(atoms):
            arc, energy, xyz = (t.cpu().numpy() for t in res.profile(b))
            images = []
            for k in range(len(arc)):
                image = copy.deepcopy(a)
                if hasattr(image, 'set_positions'):
                    image.set_positions(xyz[k].astype(np.float64))
                else:
                    image.positions = xyz[k].astype(np.float64)
                if not isinstance(getattr(image, 'info', None), dict):
                    image.info = {}
                image.info['energy'], image.info['arc_length'] = float(energy[k]), float(arc[k])
                images.append(image)
            out['images'].append(images), out['arc'].append(arc), out['energy'].append(energy), out['positions'].append(xyz)
        for k, t in (('status', res.status), ('n_steps', res.n_steps), ('fmax', res.fmax), ('arc_length', res.arc_length)):
            out[k] = t.cpu().numpy().reshape(n_frames, 2)
        if single:
            out = {k: v[0] for k, v in out.items()}
        return out

    def find_saddle(self, atoms_or_list, direction=None, fmax: float = 0.001, max_evaluations: int = 1000,
                    dimer_length: float = 0.01, rotation_tolerance: float = 5.0, max_rotations: int = 8, memory: int = 16,
                    maxstep: float = 0.2, alpha: float = 70.0, check_every: int = 10, fixed=None, solver: str = 'lds'):
        """Dimer-method saddle search from one guessed transition geometry or a list of equally sized ones, all stepped together
        on the device (NewtonNet.saddle_search: gradients only, one force evaluation and one launch per step), until every
        structure's largest atomic force is below fmax (eV / Angstrom) with a negative curvature along its mode, or
        max_evaluations evaluations have been made.  direction: array [n_atoms, 3] (one structure) or [n_frames, n_atoms, 3], the
        start direction of each dimer, or None for the lowest normal mode of every structure.  fixed: bool array [n_atoms], the
        same atoms held in every structure.  Returns a dict of numpy arrays: positions, mode [n_frames, n_atoms, 3], energy, fmax,
        curvature, converged, n_steps, n_evaluations, n_rotations [n_frames]; one structure drops the frame axis.  The Atoms objects
        are not modified."""
        from newtonnet_amd import dimer as _d
        from newtonnet_amd.vibrations import _check_solver
        atoms = [atoms_or_list] if _is_single(atoms_or_list) else list(atoms_or_list)
        if not atoms:
            raise ValueError('find_saddle: at least one structure expected')
        n_frames, n_atoms = len(atoms), len(atoms[0])
        if any(len(a) != n_atoms for a in atoms):
            raise ValueError('find_saddle: frames of different sizes cannot share one array; use model.saddle_search (packed per '
                             'molecule)')
        _d.check_arguments(fmax, dimer_length, rotation_tolerance, max_rotations, memory, maxstep, alpha)
        _d.check_run_arguments(max_evaluations, check_every, 0)
        _check_solver(solver)
        if fixed is not None:
            fixed = np.asarray(fixed)
            if fixed.dtype != np.bool_ or fixed.shape != (n_atoms,):
                raise ValueError(f'fixed: a bool array [{n_atoms}] expected')
        if direction is not None:
            direction = np.asarray(direction, dtype=np.float32)
            if direction.shape not in ((n_frames, n_atoms, 3),) + (((n_atoms, 3),) if n_frames == 1 else ()):
                raise ValueError(f'direction: an array [{n_frames}, {n_atoms}, 3] expected (got {direction.shape})')
        if self.device.type != 'cuda':
            raise RuntimeError('newtonnet_amd saddle searches run on an MI355X (ROCm) device only: make the calculator with '
                               'device="cuda"')
        z, pos, cell, batch = self.format_data(atoms)
        held = None if fixed is None else torch.from_numpy(np.tile(fixed, n_frames)).to(pos.device)
        along = None if direction is None else torch.from_numpy(direction.reshape(-1, 3).copy()).to(pos.device)
        search = self.model.saddle_search(z, pos.float(), cell.float(), batch, direction=along, fmax=fmax, dimer_length=dimer_length,
                                          rotation_tolerance=rotation_tolerance, max_rotations=max_rotations, memory=memory,
                                          maxstep=maxstep, alpha=alpha, fixed=held, solver=solver)
        res = search.run(int(max_evaluations), int(check_every))
        out = dict(positions=res.pos.cpu().numpy().reshape(n_frames, n_atoms, 3),
                   mode=res.mode.cpu().numpy().reshape(n_frames, n_atoms, 3), energy=res.energy.cpu().numpy(),
                   fmax=res.fmax.cpu().numpy(), curvature=res.curvature.cpu().numpy(), converged=res.converged.cpu().numpy(),
                   n_steps=res.n_steps.cpu().numpy(), n_evaluations=res.n_evaluations.cpu().numpy(),
                   n_rotations=res.n_rotations.cpu().numpy())
        if n_frames == 1:
            out = {k: v[0] for k, v in out.items()}
        return out

    # ------------------------------------------------------------------ MD-loop latency path
    def _calculate_md(self, atoms):
        """One structure per call, called thousands of times by an MD driver (simulate.py:21-30): keep everything that does
        not change between steps on the device -- the candidate neighbor list (cutoff + skin), the parameter struct, the
        workspace and output buffers -- re-evaluate only the edge geometry, and replay the launches from a HIP graph."""
        from newtonnet_amd import hip
        z = np.asarray(atoms.get_atomic_numbers())
        pos = np.asarray(atoms.get_positions(wrap=True), dtype=np.float64)
        try:
            free = np.asarray(atoms.get_positions(), dtype=np.float64)       # unwrapped: what the skin criterion follows
        except TypeError:
            free = pos
        cell = np.array(getattr(atoms.get_cell(), 'array', atoms.get_cell()), dtype=np.float64).reshape(3, 3).copy()
        cell[~np.asarray(atoms.get_pbc(), dtype=bool)] = 0.0
        st = self._md
        stale = st is None or st['z'].shape != z.shape or not np.array_equal(st['z'], z) \
            or not np.array_equal(st['cell'] != 0, cell != 0)
        if not stale:
            # Verlet criterion with a moving cell (NPT): a pair inside the cutoff now was inside cutoff + skin at build time
            # as long as  2 max|dr| + strain * (cutoff + skin) <= skin   (dr: unwrapped displacement since the build)
            moved = float(np.sqrt(np.max(np.sum((free - st['ref']) ** 2, axis=1))))
            strain = 0.0
            if np.any(cell != 0) and not np.array_equal(st['cell'], cell):
                ref = np.where(st['cell'].any(axis=1, keepdims=True), st['cell'], np.eye(3))
                cur = np.where(cell.any(axis=1, keepdims=True), cell, np.eye(3))
                strain = float(np.linalg.norm(np.linalg.solve(ref, cur) - np.eye(3), 2))
            stale = 2.0 * moved + strain * (st['cutoff'] + self.skin) > self.skin
        if stale:
            st = self._md_build(z, pos, free, cell)
        elif not np.array_equal(st['cell_now'], cell):
            st['cell_now'] = cell.copy()
            st['cell_dev'].copy_(torch.tensor(cell[None], dtype=torch.float32), non_blocking=False)
        # (a big system is kept in the spatial order of its last list build: _md_build)
        order = st['order']
        st['pos_host'].copy_(torch.from_numpy((pos if order is None else pos[order]).astype(np.float32)))
        if not st['zero_copy_in']:
            st['pos'].copy_(st['pos_host'], non_blocking=True)
        if st['graph'] is not None:
            st['graph'].replay()
        else:
            self._md_step(st)
        if not st['zero_copy']:
            st['out_host'].copy_(st['buf'], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        self.md_stats['steps'] += 1
        n = len(z)
        res = st['out_host'].numpy()
        if 'energy' in self.properties:
            self.results['energy'] = res[0].copy()
        if 'free_energy' in self.properties:
            self.results['free_energy'] = res[0].copy()
        if 'forces' in self.properties:
            if st['order'] is None:
                self.results['forces'] = res[1:1 + 3 * n].reshape(n, 3).copy()
            else:
                forces = np.empty((n, 3), dtype=res.dtype)
                forces[st['order']] = res[1:1 + 3 * n].reshape(n, 3)
                self.results['forces'] = forces
        if 'stress' in self.properties:
            stress = -res[1 + 3 * n:10 + 3 * n].reshape(3, 3) / np.float32(np.linalg.det(cell))
            self.results['stress'] = stress[[0, 1, 2, 1, 0, 0], [0, 1, 2, 2, 2, 1]]

    def _md_build(self, z, pos, free, cell):
        from newtonnet_amd import hip
        from newtonnet_amd.models.output import StressOutput, VirialOutput
        dev, model = self.device, self.model
        emb = model.embedding_layers.edge_embedding
        n = len(z)
        want_forces = any(isinstance(l, DerivativeProperty) for l in model.output_layers)
        want_virial = any(isinstance(l, (VirialOutput, StressOutput)) for l in model.output_layers)
        st = dict(z=z.copy(), cell=cell.copy(), cell_now=cell.copy(), ref=free.copy(), graph=None, want_forces=want_forces,
                  want_virial=want_virial, order=None)
        # one big system: the list, the device arrays and every step until the next rebuild use the atoms in Morton order of
        # cells (hip.spatial_order -- partner rows close together whatever order the Atoms object
        # has); positions are gathered and forces scattered on the host, energy and stress are sums
        from newtonnet_amd.models import newtonnet as nn_mod
        order_min = model.__dict__.get('_spatial_order_min', nn_mod._SPATIAL_ORDER_MIN)
        if order_min > 0 and n >= order_min:
            # (hip.spatial_order: the library's own kernels, csrc/graph.hip)
            st['order'] = hip.spatial_order(torch.tensor(pos, dtype=torch.float32, device=dev),
                                            torch.tensor(z, dtype=torch.long, device=dev), float(emb.cutoff))[0].cpu().numpy().astype(np.int64)
            z, pos = z[st['order']], pos[st['order']]
        st['z_dev'] = torch.tensor(z, dtype=torch.long, device=dev)
        st['pos'] = torch.tensor(pos, dtype=torch.float32, device=dev)
        st['cell_dev'] = torch.tensor(cell[None], dtype=torch.float32, device=dev)
        st['batch'] = torch.zeros(n, dtype=torch.long, device=dev)
        st['pos_host'] = torch.tensor(pos, dtype=torch.float32).pin_memory()
        # (reading the positions in place from the pinned host array as well measured no gain: 393 vs 388 us; off by default)
        st['zero_copy_in'] = os.environ.get('NNHIP_MD_ZERO_COPY_IN', '0') != '0'
        pos_dev = st['pos']
        if st['zero_copy_in']:
            st['pos'] = st['pos_host']
        st['freq'] = emb.embedding.frequencies
        st['cutoff'] = float(emb.cutoff)
        st['model'] = model._hip_model(list(model.output_properties).index('energy'))
        st['g'] = hip.build_graph(pos_dev, st['cell_dev'], st['batch'], st['cutoff'] + self.skin, st['freq'], cell_host=cell[None],
                                  envelope=emb.envelope_id)
        st['prep'] = hip.prepare(st['model'], dev)     # parameters are fixed while the calculator owns the model (eval)
        g = st['g']
        # Results (energy, forces, virial: a few hundred bytes) are written by the last kernels STRAIGHT into pinned host memory
        # (hipHostMalloc memory is mapped into the device's address space on ROCm): no device->host copy per step, whose DMA
        # start-up latency was ~80 us of the ~390 us step.  NNHIP_MD_ZERO_COPY=0 restores the device buffer + copy.
        st['zero_copy'] = os.environ.get('NNHIP_MD_ZERO_COPY', '1') != '0'
        st['out_host'] = torch.zeros(1 + 3 * n + 9, dtype=torch.float32).pin_memory()
        st['buf'] = st['out_host'] if st['zero_copy'] else torch.zeros(1 + 3 * n + 9, dtype=torch.float32, device=dev)
        st['out'] = dict(energy=st['buf'][0:1], forces=st['buf'][1:1 + 3 * n].view(n, 3) if want_forces else None,
                         virial=st['buf'][1 + 3 * n:].view(1, 3, 3) if want_virial else None,
                         atom_energy=torch.empty(n, dtype=torch.float32, device=dev), atom_node=None, force_node=None)
        need = hip.lib().nnhip_workspace_bytes(n, g.n_edges, 1, st['model'].n_layers)
        st['ws'] = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        self._md_step(st)                      # warm-up on the current stream (one-time kernel attributes, lazy loads)
        if self.capture:
            try:
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    self._md_step(st)
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                    self._md_step(st)
                st['graph'] = graph
            except Exception as exc:  # noqa: BLE001 -- capture is an optimisation; fall back to plain launches
                import warnings
                warnings.warn(f'HIP graph capture of the MD step failed ({exc}); using direct launches')
                st['graph'] = None
                torch.cuda.synchronize()
        self._md = st
        self.md_stats['rebuilds'] += 1
        return st

    def _md_step(self, st):
        from newtonnet_amd import hip
        hip.refresh_graph(st['g'], st['pos'], st['cell_dev'], st['batch'], st['cutoff'], st['freq'])
        hip.energy_forces(st['model'], st['z_dev'], st['pos'], st['cell_dev'], st['g'], want_forces=st['want_forces'],
                          want_virial=st['want_virial'], want_nodes=False, workspace=st['ws'], out=st['out'],
                          prepared=st['prep'])

    # ------------------------------------------------------------------ ase_interface.py:83-129
    def load_model(self, model):
        """model: a NewtonNet of this package, ANY nn.Module with the reference's parameter names (e.g. the reference's own
        NewtonNet), a state_dict, or the path of a whole-module pickle (torch.save(model), trainer.py:219 -- written by
        this package OR by the reference, ase_interface.py:87), a state_dict file or an .npz of arrays.  Anything that is
        not already a newtonnet_amd NewtonNet is rebuilt from its state_dict (the key names are identical by construction)."""
        from newtonnet_amd.models import NewtonNet
        if isinstance(model, torch.nn.Module):
            pass
        elif isinstance(model, dict):
            model = self._from_state_dict(model)
        elif str(model).endswith('.npz'):
            with np.load(model) as f:
                sd = {k: torch.from_numpy(f[k]) for k in f.files}
            model = self._from_state_dict(sd)
        else:
            obj = torch.load(model, map_location='cpu', weights_only=False, pickle_module=_ReferencePickle)
            model = self._from_state_dict(obj) if isinstance(obj, dict) else obj
        if not isinstance(model, NewtonNet):
            if not isinstance(model, torch.nn.Module):
                raise TypeError(f'expected a NewtonNet module, a state_dict or a path, got {type(model)}')
            model = self._from_module(model)
        if self.properties is None:
            self.properties = [{'energy': 'energy', 'gradient_force': 'forces', 'stress': 'stress'}[k]
                               for k in model.output_properties if k in ('energy', 'gradient_force', 'stress')]
            if model.__dict__.get('_hessian_head_dropped'):
                self.properties.append('hessian')
        else:
            key_map = {'energy': 'energy', 'free_energy': 'energy', 'forces': 'gradient_force', 'stress': 'stress'}
            keys_to_keep = ['energy']
            for prop in self.properties:
                if prop == 'hessian':        # NewtonNet.hessian: no output head
                    continue
                if prop not in key_map:
                    raise NotImplementedError(f"property '{prop}' is outside the MI355X hot path")
                key = key_map[prop]
                keys_to_keep.append(key)
                if key in model.output_properties:
                    continue
                model.output_properties.append(key)
                model.output_layers.append(get_output_by_string(key))
                model.scalers.append(get_scaler_by_string(key))
                model.aggregators.append(get_aggregator_by_string(key))
            for i in reversed([i for i, k in enumerate(model.output_properties) if k not in keys_to_keep]):
                model.output_properties.pop(i)
                model.output_layers.pop(i)
                model.scalers.pop(i)
                model.aggregators.pop(i)
        model.to(self.dtype)
        model.to(self.device)
        model.eval()
        model.embedding_layers.requires_dr = any(isinstance(l, DerivativeProperty) for l in model.output_layers)
        return model

    @staticmethod
    def _from_state_dict(sd, cutoff: float = 5.0, activation: str = 'swish', output_properties=None):
        """Rebuild a NewtonNet from the reference's parameter names; the sizes are read off the tensors.  Keys of the
        pre-2.0 layout of the shipped MD17 checkpoint (`embedding_layer.*`) are renamed."""
        from newtonnet_amd.models import NewtonNet
        sd = {_current_key(k): v for k, v in sd.items()}
        n_layers = 0
        while f'interaction_layers.{n_layers}.equiv_update.weight' in sd:
            n_layers += 1
        F = sd['embedding_layers.node_embedding.weight'].shape[1]
        nb = sd['embedding_layers.edge_embedding.embedding.frequencies'].numel()
        props = list(output_properties) if output_properties else ['energy', 'gradient_force']
        model = NewtonNet(cutoff=cutoff, n_features=F, n_basis=nb, n_interactions=n_layers, activation=activation,
                          layer_norm='interaction_layers.0.layer_norm.weight' in sd, output_properties=props)
        model.to(torch.float64)
        model.load_state_dict({k: v.to(torch.float64) for k, v in sd.items()})
        return model

    @classmethod
    def _from_module(cls, obj):
        """A module that is not this package's NewtonNet -- the reference's own class, or the attribute-only stand-in the
        unpickler builds when the reference package is not importable: read the hyper-parameters the state_dict does not
        carry (cutoff, activation, output heads) off the module tree, then rebuild from state_dict()."""
        sd = {k: v.detach().cpu() for k, v in obj.state_dict().items()}
        emb = getattr(obj, 'embedding_layers', None) or getattr(obj, 'embedding_layer', None)
        cutoff = 5.0
        ee = getattr(emb, 'edge_embedding', None)
        for holder, attr in ((getattr(ee, 'norm', None), 'r'), (getattr(ee, 'radius_graph', None), 'r'), (ee, 'cutoff')):
            if holder is not None and hasattr(holder, attr):
                cutoff = float(getattr(holder, attr))
                break
        activation = 'swish'
        layers = getattr(obj, 'interaction_layers', None)
        if layers is not None and len(layers):
            act = layers[0].message_nodepart[1]
            names = {'SiLU': 'swish', 'ReLU': 'relu', 'ELU': 'elu', 'LeakyReLU': 'leaky_relu', 'Tanh': 'tanh',
                     'Sigmoid': 'sigmoid', 'Softplus': 'softplus', 'GELU': 'gelu', 'ShiftedSoftplus': 'ssp'}
            if type(act).__name__ not in names:
                raise NotImplementedError(f'activation module {type(act).__name__} is outside the MI355X hot path')
            activation = names[type(act).__name__]
        props = [k for k in getattr(obj, 'output_properties', ['energy', 'gradient_force'])]
        # a reference HessianOutput head (output.py:134-152) holds no parameters: drop it, NewtonNet.hessian serves 'hessian'
        had_hessian = 'hessian' in props
        props = [k for k in props if k != 'hessian']
        for k in props:
            if k not in ('energy', 'gradient_force', 'direct_force', 'virial', 'stress'):
                raise NotImplementedError(f"output property '{k}' of the loaded model is outside the MI355X hot path")
        model = cls._from_state_dict(sd, cutoff=cutoff, activation=activation, output_properties=props)
        if had_hessian:
            model.__dict__['_hessian_head_dropped'] = True
        return model

    # ------------------------------------------------------------------ ase_interface.py:131-142
    def format_data(self, atoms_list):
        zs, ps, cs, bs = [], [], [], []
        for b, atoms in enumerate(atoms_list):
            z = np.asarray(atoms.get_atomic_numbers())
            pos = np.asarray(atoms.get_positions(wrap=True), dtype=np.float64)
            cell = np.array(getattr(atoms.get_cell(), 'array', atoms.get_cell()), dtype=np.float64).reshape(3, 3).copy()
            pbc = np.asarray(atoms.get_pbc(), dtype=bool)
            cell[~pbc] = 0.0
            zs.append(z)
            ps.append(pos)
            cs.append(cell)
            bs.append(np.full(len(z), b))
        z = torch.tensor(np.concatenate(zs), dtype=torch.long, device=self.device)
        pos = torch.tensor(np.concatenate(ps), dtype=self.dtype, device=self.device)
        cell = torch.tensor(np.stack(cs), dtype=self.dtype, device=self.device)
        batch = torch.tensor(np.concatenate(bs), dtype=torch.long, device=self.device)
        return z, pos, cell, batch
