"""What a step of batched reaction-path following costs on one MI355X: 1024 synthetic aspirins (bench.synthetic_aspirin) and one
aspirin, --steps steps (200) after --warmup (20), wall clock around a synchronised region (the region and warm-up of
tools/bench_relax.py), ms per step of
  (a) ReactionPath.run: model() + one nnhip_irc_step launch per step (csrc/irc.hip), check_every = 0, record_every = 0
  (b) a bare loop of model() calls on the same batch, forces touched every step -- the floor
each the MEDIAN of --repeats (3) runs taken alternately, and the launch's share (a - b) / b of the bare step.  The structures are
no saddles and the seeded weights no trained surface: at the default speed every path has turned within 100 steps, and a stopped
path costs the launch next to nothing.  So that a RUNNING path's whole step is timed -- damping, drift, arc length, error estimate,
cube root -- every path starts along the positive components of its own forces (downhill, and a direction the sign convention of
`direction` leaves alone; both=False), 1e-3 amu^1/2 A away, at a speed of 1e-4 A/fs with the time step pinned to 0.05 fs: it moves
about 1e-5 A per step and none can pass a minimum inside the timed region; fmax is 1e-6 eV/A.  The paths that
have stopped by the end are counted (expected: 0).
Prints one JSON line and writes it to profiles/irc_aspirin.json (--out).
usage: python tools/bench_irc.py [--steps 200] [--warmup 20] [--mols 1024] [--repeats 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tests import util  # noqa: E402


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def legs(model, inputs, steps, warmup, repeats):
    z, pos, cell, batch = inputs
    along = model(z, pos, cell, batch).gradient_force.detach().clamp(min=0.0)
    path = model.reaction_path(z, pos, cell, batch, direction=along, both=False, fmax=1e-6, speed=1e-4, timestep=0.05,
                               timestep_min=0.05, timestep_max=0.05, initial_displacement=1e-3)

    def run(n):
        path.run(n, check_every=0, record_every=0)

    def bare(n):
        for _ in range(n):
            model(path.z, pos, path.cell, path.batch).gradient_force
    run(warmup)
    bare(warmup)
    t_run, t_bare = [], []
    for _ in range(repeats):
        t_run.append(timed(run, steps))
        t_bare.append(timed(bare, steps))
    res = path.run(0)
    a, b = statistics.median(t_run), statistics.median(t_bare)
    return dict(n_paths=int(path.n_mol), n_atoms=int(path.n_atoms), steps_taken_min=int(res.n_steps.min()),
                steps_taken_max=int(res.n_steps.max()), stopped_paths=int((res.status != 0).sum()),
                timestep_fs_median=round(float(path.timestep.median()), 4), reaction_path_run_ms=round(a, 4),
                bare_model_loop_ms=round(b, 4), runs_ms=[round(t, 4) for t in t_run], bare_ms=[round(t, 4) for t in t_bare],
                launch_share_of_bare_step=round((a - b) / b, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--mols', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    rec = dict(steps=a.steps, warmup=a.warmup, repeats=a.repeats,
               batch=legs(model, bench.synthetic_aspirin(a.mols, 0, 'cuda'), a.steps, a.warmup, a.repeats),
               single=legs(model, bench.synthetic_aspirin(1, 0, 'cuda'), a.steps, a.warmup, a.repeats))
    b = rec['batch']
    rec['us_per_path_step'] = round(1e3 * b['reaction_path_run_ms'] / b['n_paths'], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'irc_aspirin.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
