"""The stepping loop that the five device optimisers share (newtonnet_amd/stepper.py), run on the CPU with a fake driver: which
steps are recorded, how a run continues, when it stops, and how often it launches, evaluates and reads.  The expected values are
written out from the contract of Stepper.run; the drivers' GPU suites cover the same behaviours on the device."""
from types import SimpleNamespace

import pytest
import torch

from newtonnet_amd.stepper import Stepper, check_run_arguments

CHECK_ONLY = 4
NEVER = 1000          # a stop[b] that no test reaches


class _Reads:
    """the fake's `active` tensor as the loop sees it: every comparison (the loop's one host read) is logged with the step"""

    def __init__(self, tensor, owner):
        self.tensor, self.owner = tensor, owner

    def __eq__(self, other):
        self.owner.reads.append(self.owner.launches.count('step'))
        return self.tensor == other


class _Fake(Stepper):
    """B systems of 2 atoms at 0: a step adds 1 to every coordinate of an active system, system b goes inactive after stop[b]
    steps and is frozen from then on, and the check-only launch moves nothing"""
    CHECK_ONLY = CHECK_ONLY
    TRAJ = (('pos', ('n_atoms', 3), torch.float32), ('taken', ('n_mol',), torch.int64))

    def __init__(self, stop):
        self.n_mol, self.n_atoms = len(stop), 2 * len(stop)
        self._owner = torch.arange(self.n_mol).repeat_interleave(2)
        self._stop = torch.tensor(stop, dtype=torch.int32)
        self._status = torch.zeros(self.n_mol, dtype=torch.int32)
        self._taken = torch.zeros(self.n_mol, dtype=torch.int32)
        self._init_buffers(torch.zeros(self.n_atoms, 3))
        self.launches, self.evaluations, self.reads = [], 0, []
        self._active = _Reads(self._status, self)

    def _evaluate(self):
        self.evaluations += 1
        self._force = -self._pos[self._cur]
        self._energy = self._pos[self._cur].sum().reshape(1)

    def _launch(self, flags=0):
        other = 1 - self._cur
        self._pos[other].copy_(self._pos[self._cur])
        if flags & CHECK_ONLY:
            self.launches.append('check')
        else:
            self.launches.append('step')
            moving = self._status == 0
            self._pos[other] += moving[self._owner][:, None].float()
            self._taken += moving.int()
            self._status[moving & (self._taken >= self._stop)] = 1
        self._cur = other

    def _frame(self):
        return self._pos[self._cur].clone(), self._taken.long()

    def _result(self):
        return SimpleNamespace(pos=self._pos[self._cur].clone(), taken=self._taken.long())


@pytest.mark.parametrize('max_steps, record_every, steps', [(7, 3, [3, 6, 7]), (6, 3, [3, 6]), (0, 3, [])])
def test_recorded_steps(max_steps, record_every, steps):
    r = _Fake([NEVER, NEVER]).run(max_steps, check_every=0, record_every=record_every)
    assert r.traj_step.dtype == torch.int64 and r.traj_step.tolist() == steps
    # every field exists with the declared trailing shape and dtype, frames or none
    assert r.traj_pos.shape == (len(steps), 4, 3) and r.traj_pos.dtype == torch.float32
    assert r.traj_taken.shape == (len(steps), 2) and r.traj_taken.dtype == torch.int64
    assert r.traj_pos[:, 0, 0].tolist() == [float(s) for s in steps]          # a frame holds the state after its step
    assert r.traj_taken[:, 1].tolist() == steps


def test_no_trajectory_without_record_every():
    r = _Fake([NEVER, NEVER]).run(5, check_every=0, record_every=0)
    assert not [name for name in vars(r) if name.startswith('traj_')]
    assert r.taken.tolist() == [5, 5]


def test_a_run_continues_the_one_before():
    """The contract: a call records the multiples of record_every of THIS call and its last step, numbered since construction.
    So run(4) records its step 3 and its last step 4, and run(3) after it records its step 3, which is step 7 since construction.
    (With the multiples counted since construction the lists would still be [3, 4] and [6, 7]: a call always records its last
    step, as (7, 3) -> [3, 6, 7] above shows, so no reading of the contract gives [3] for run(4).)"""
    s = _Fake([NEVER, NEVER])
    assert s.run(4, check_every=0, record_every=3).traj_step.tolist() == [3, 4]
    assert s.step_count == 4
    r = s.run(3, check_every=0, record_every=3)
    assert r.traj_step.tolist() == [7] and r.traj_pos[:, 0, 0].tolist() == [7.0]
    assert s.step_count == 7
    whole = _Fake([NEVER, NEVER]).run(7, check_every=0, record_every=3)
    assert torch.equal(r.pos, whole.pos) and torch.equal(r.pos, torch.full((4, 3), 7.0))
    assert r.taken.tolist() == whole.taken.tolist() == [7, 7]


def test_stopping():
    s = _Fake([2, 5])
    r = s.run(20, check_every=2)
    assert s.launches == ['step'] * 6 + ['check']          # not 5 (no read at step 5) and not max_steps
    assert s.reads == [2, 4, 6]
    assert r.taken.tolist() == [2, 5]
    never = _Fake([2, 5])
    r0 = never.run(20, check_every=0)
    assert never.launches == ['step'] * 20 + ['check'] and never.reads == []
    # a system that is no longer active is frozen, so how often the host looks changes nothing
    assert torch.equal(r.pos[:2], torch.full((2, 3), 2.0)) and torch.equal(r0.pos[:2], torch.full((2, 3), 2.0))
    assert torch.equal(r.pos[2:], torch.full((2, 3), 5.0)) and torch.equal(r0.pos, r.pos)


def test_counts_of_a_call():
    s = _Fake([NEVER])
    s.run(3, check_every=0)
    assert s.launches == ['step'] * 3 + ['check']          # one check-only launch, after the loop
    assert s.evaluations == 1 + 3                          # the first run evaluates the start state, then once per step
    s.run(2, check_every=0)
    assert s.launches == ['step'] * 3 + ['check'] + ['step'] * 2 + ['check']
    assert s.evaluations == 1 + 3 + 2
    s.run(0)
    assert s.launches[-2:] == ['check', 'check'] and s.launches.count('step') == 5 and s.evaluations == 6
    fresh = _Fake([NEVER])
    r = fresh.run(0)
    assert fresh.launches == ['check'] and fresh.evaluations == 1 and torch.equal(r.pos, torch.zeros(2, 3))
    # the check-only launch copies the state into the other buffer: the current one holds it either way
    assert torch.equal(s.positions, torch.full((2, 3), 5.0))


def test_run_arguments_are_refused():
    for bad in ((-1, 10, 0), (2.5, 10, 0), (5, -1, 0), (5, 10, -2), (5, 1.5, 0)):          # (test_relax_host.py's list)
        with pytest.raises(ValueError):
            check_run_arguments(*bad)
        with pytest.raises(ValueError):
            _Fake([NEVER]).run(*bad)
    assert check_run_arguments(5, 0, 0) == (5, 0, 0)
    with pytest.raises(ValueError, match='max_steps'):
        check_run_arguments(-1, 10, 0)
    for k, name in enumerate(('max_evaluations', 'check_every', 'record_every')):           # (test_dimer_host.py's list)
        for bad in (-1, 2.5):
            args = [1, 1, 0]
            args[k] = bad
            with pytest.raises(ValueError, match=name):
                check_run_arguments(*args, 'max_evaluations')


def test_device_check():
    s = _Fake([NEVER])
    s.NOUN = 'relaxations'
    with pytest.raises(RuntimeError, match='newtonnet_amd relaxations run on an MI355X'):
        s._check_device(torch.zeros(2, 3), z=torch.zeros(2), fixed=None)
