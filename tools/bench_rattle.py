"""What X-H constraints cost per step of batched molecular dynamics on one MI355X: aspirin (the eight frames of
tests/golden/case_aspirin8_rand.npz, repeated) with its 8 X-H bond lengths constrained ('h-bonds': nnhip_md_step_constrained,
csrc/rattle.hip) against Dynamics.run without constraints (nnhip_md_step) on the same batch, at 1024, 128 and 1 molecules.
Microcanonical from Maxwell-Boltzmann velocities at 300 K, --steps steps (200) after --warmup (20), wall clock around a
synchronised region, ms per step: the MEDIAN of three interleaved runs of each leg, all three listed, every run from the same
start with a Dynamics of its own.  Both legs run at the same
time step (--timestep, 0.5 fs), so the difference is the launch and nothing else; that constraints allow 2 fs where the free run
needs 0.5 fs is a statement about the time step, not a timing, and is not measured here.  Also: the mean and the largest sweep
count of the constrained launches (read once after the timed region).
Prints one JSON line and writes it to profiles/rattle_aspirin.json (--out).
usage: python tools/bench_rattle.py [--steps 200] [--warmup 20] [--timestep 0.5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import util  # noqa: E402


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def aspirins(n_mol):
    z, pos, cell, batch, _ = util.case_inputs('aspirin8_rand', torch.float32)
    reps = -(-n_mol // 8)
    z, pos = z.repeat(reps)[:21 * n_mol], pos.repeat(reps, 1)[:21 * n_mol]
    batch = torch.repeat_interleave(torch.arange(n_mol), 21)
    return z.cuda(), pos.cuda(), torch.zeros(n_mol, 3, 3, device='cuda'), batch.cuda()


def legs(model, n_mol, steps, warmup, timestep):
    z, pos, cell, batch = aspirins(n_mol)
    make = dict(free=lambda: model.dynamics(z, pos, cell, batch, temperature=300.0, timestep=timestep,
                                            generator=torch.Generator(device='cuda').manual_seed(0)),
                constrained=lambda: model.dynamics(z, pos, cell, batch, temperature=300.0, timestep=timestep, constraints='h-bonds',
                                                   generator=torch.Generator(device='cuda').manual_seed(0)))
    # every timed run starts from the same geometry with a Dynamics of its own: the seeded weights are no physical potential, and
    # over a picosecond molecules drift apart (fewer edges, a cheaper model call), which would favour whichever leg ran longer
    runs = dict(free=[], constrained=[])
    sweeps, failures = [], 0
    for _ in range(3):
        for k in ('free', 'constrained'):
            dyn = make[k]()
            dyn.run(warmup)
            runs[k].append(round(timed(lambda n: dyn.run(n), steps), 4))
            if k == 'constrained':
                sweeps.append(dyn.constraint_sweeps.float())
                failures += int(dyn.constraint_failures.sum())
                n_con = int(dyn.constraint_pairs.shape[0])
    sweeps = torch.stack(sweeps)
    out = dict(n_mol=n_mol, n_atoms=21 * n_mol, constraints_per_molecule=n_con // n_mol)
    for k in runs:
        out[k + '_ms'] = float(np.median(runs[k]))
        out[k + '_runs_ms'] = runs[k]
    out['constrained_minus_free_ms'] = round(out['constrained_ms'] - out['free_ms'], 4)
    out['sweeps_mean'], out['sweeps_max'] = round(float(sweeps.mean()), 2), int(sweeps.max())
    out['constraint_failures'] = failures
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--timestep', type=float, default=0.5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    rec = dict(steps=a.steps, warmup=a.warmup, thermostat='none (velocity-Verlet RATTLE)', timestep_fs=a.timestep,
               sweeps='the largest sweep count of the last launch of each timed run, per molecule: mean and max over molecules and runs',
               sizes=[legs(model, n, a.steps, a.warmup, a.timestep) for n in (1024, 128, 1)])
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'rattle_aspirin.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
