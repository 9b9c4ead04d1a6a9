"""The host side that the device-resident optimisers share (relax.py, cellrelax.py, neb.py, dimer.py, irc.py): the device check
of a constructor, the two position buffers and their swap, the model evaluation, and the stepping loop of run() with its
trajectory.  What a step does on the device is the driver's: its _launch, its state tensors, its frame and its result."""
from __future__ import annotations

import torch


def check_run_arguments(max_steps, check_every, record_every, first='max_steps'):
    """the three numbers of a run(), refused without touching the device; `first` is the name the driver gives the first one"""
    for name, v in ((first, max_steps), ('check_every', check_every), ('record_every', record_every)):
        if int(v) != v or v < 0:
            raise ValueError(f'{name}: an integer >= 0 expected (got {v!r})')
    return int(max_steps), int(check_every), int(record_every)


class Stepper:
    """Base of a driver that steps B systems together, one model() call and one launch per step.  A driver states:

    NOUN         what it runs, for the refusal of CPU tensors ('relaxations')
    CHECK_ONLY   the flag of the launch that measures the state reached and moves nothing
    TRAJ         its trajectory fields after traj_step: (name, trailing shape, dtype) each, a size of the shape being an int or the
                 name of an attribute of the driver ('n_atoms'); _frame() returns one tensor per field, in this order
    _active      int32 tensor, set by the constructor: its zeros are the systems still being stepped
    _launch(flags=0), _frame(), _result()

    and the model's inputs as self.model, self.z, self.cell, self.batch (or its own _evaluate)."""
    NOUN, CHECK_ONLY, TRAJ = None, None, ()

    def _check_device(self, pos, **tensors):
        """pos on a ROCm device and every tensor given by name (None: absent) on the same one; returns the device"""
        if not pos.is_cuda:
            raise RuntimeError(f'newtonnet_amd {self.NOUN} run on an MI355X (ROCm) device only: move the model and the inputs to '
                               '"cuda"')
        for name, t in tensors.items():
            if t is not None and t.device != pos.device:
                raise ValueError(f'{name} is on {t.device}, pos on {pos.device}')
        return pos.device

    def _init_buffers(self, pos):
        """two position buffers, the first being `pos` (the driver's own copy): a step reads one and writes the other, so the
        forward call queued on the one it read can still be repeated from it (NewtonNet._forward_deferred)"""
        self._pos = [pos, torch.empty_like(pos)]
        self._cur = 0
        self._force = self._energy = None
        self.step_count = 0

    def _evaluate(self):
        """forces and energies at the current positions.  Touching gradient_force and energy settles the deferred record of the
        call -- a repeat, if one is needed, happens HERE, from the buffer the call was queued with and before any kernel writes a
        buffer"""
        out = self.model(self.z, self._pos[self._cur], self.cell, self.batch)
        self._force = out.gradient_force
        self._energy = out.energy

    def _ensure_state(self):
        if self._force is None:
            with torch.no_grad():
                self._evaluate()

    def _begin(self):
        """what a driver keeps of the state a run starts from (ReactionPath: the start of its paths)"""

    @property
    def positions(self):
        return self._pos[self._cur].detach().clone()

    @property
    def forces(self):
        self._ensure_state()
        return self._force

    @property
    def potential_energy(self):
        self._ensure_state()
        return self._energy

    @property
    def n_steps(self):
        return self._n_steps.long()

    def run(self, max_steps: int, check_every: int = 10, record_every: int = 0):
        """Up to max_steps steps of every system that is still active, then the result at the state reached.  Every check_every
        steps the host reads ONE number, the count of active systems, and stops when it is 0 (check_every = 0: never reads, always
        max_steps launches).  A system that is no longer active is frozen bit for bit, so check_every changes no bit of any result.
        record_every > 0 records the steps record_every, 2 record_every, ... of this call that were taken, and the last one, each
        numbered since the driver was made; recording changes no bit either.  May be called again to continue: run(a); run(b)
        leaves the bits of run(a + b)."""
        return self._run(*check_run_arguments(max_steps, check_every, record_every))

    def _run(self, max_steps, check_every, every):
        frames = []
        with torch.no_grad():
            self._ensure_state()
            self._begin()
            active, taken = self._active, 0
            for k in range(1, max_steps + 1):
                self._launch()
                self._evaluate()
                taken = k
                if every and k % every == 0:
                    frames.append((self.step_count + k,) + self._frame())
                if check_every and k % check_every == 0 and int((active == 0).sum()) == 0:
                    break
            if every and taken and (not frames or frames[-1][0] != self.step_count + taken):
                frames.append((self.step_count + taken,) + self._frame())
            self.step_count += taken
            # the state reached: its forces are evaluated already; a check-only launch measures it (fmax and what else the driver
            # reports) and moves nothing -- it copies the positions into the other buffer
            self._launch(self.CHECK_ONLY)
            result = self._result()
            if every:
                dev = self._pos[0].device
                result.traj_step = torch.tensor([f[0] for f in frames], dtype=torch.int64, device=dev)
                for j, (name, shape, dtype) in enumerate(self.TRAJ, start=1):
                    if frames:
                        field = torch.stack([f[j] for f in frames])
                    else:
                        sizes = [getattr(self, s) if isinstance(s, str) else s for s in shape]
                        field = torch.zeros(0, *sizes, dtype=dtype, device=dev)
                    setattr(result, 'traj_' + name, field)
        return result
