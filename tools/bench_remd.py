"""What replica exchange adds to a step of batched molecular dynamics on one MI355X: --ladders (128) ladders of --replicas (8)
synthetic aspirin replicas each (bench.synthetic_aspirin) and one ladder of 8, --steps steps (200) after --warmup (20),
exchange_every = --every (10), wall clock around a synchronised region (the region and warm-up of tools/bench_md.py), ms per step of
  (a) ReplicaExchange.run: Dynamics's step, plus at every attempt the split of the fused integrator launch and one
      nnhip_remd_exchange launch (csrc/remd.hip)
  (b) Dynamics.run on the same replicated batch, temperature ladder and friction -- what the package could do without exchanges: the
      floor
and the difference per attempt, (a - b) x every, in microseconds.  Temperatures 300 .. 600 K, geometric; friction 0.01 / fs; seeded
weights.  --repeat (3) runs of each leg, interleaved; the figures are the medians and every run is kept in the record.  Prints one
JSON line and writes it to profiles/remd_aspirin.json (--out).
usage: python tools/bench_remd.py [--steps 200] [--warmup 20] [--ladders 128] [--replicas 8] [--every 10] [--repeat 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tests import util  # noqa: E402

FRICTION = 0.01


def timed(fn, steps, warmup):
    fn(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def legs(model, n_ladders, n_replicas, every, steps, warmup, repeat):
    z, pos, cell, batch = bench.synthetic_aspirin(n_ladders, 0, 'cuda')
    T = np.geomspace(300.0, 600.0, n_replicas)
    t_rex, t_dyn = [], []
    for r in range(repeat):
        gen = torch.Generator(device='cuda').manual_seed(r)
        rex = model.replica_exchange(z, pos, cell, batch, T, every, FRICTION, generator=gen, exchange_seed=r)
        t_rex.append(timed(lambda n: rex.run(n), steps, warmup))
        gen = torch.Generator(device='cuda').manual_seed(r)
        dyn = model.dynamics(rex.z, pos.view(n_ladders, -1, 3).repeat_interleave(n_replicas, 0).reshape(-1, 3), rex.cell, rex.batch,
                             temperature=rex.ladders.reshape(-1), friction=FRICTION, generator=gen)
        t_dyn.append(timed(lambda n: dyn.run(n), steps, warmup))
    a, b = statistics.median(t_rex), statistics.median(t_dyn)
    attempts = int(rex.n_attempt.sum())
    return dict(n_ladders=n_ladders, n_replicas=n_replicas, n_atoms=int(rex.n_atoms), exchange_every=every,
                remd_run_ms=round(a, 4), dynamics_run_ms=round(b, 4), remd_runs_ms=[round(t, 4) for t in t_rex],
                dynamics_runs_ms=[round(t, 4) for t in t_dyn], us_per_attempt=round(1e3 * (a - b) * every, 2),
                share_of_dynamics_step=round((a - b) / b, 4),
                acceptance_last_run=round(float(rex.n_accept.sum()) / max(attempts, 1), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--ladders', type=int, default=128)
    ap.add_argument('--replicas', type=int, default=8)
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    rec = dict(steps=a.steps, warmup=a.warmup, repeat=a.repeat,
               batch=legs(model, a.ladders, a.replicas, a.every, a.steps, a.warmup, a.repeat),
               single=legs(model, 1, a.replicas, a.every, a.steps, a.warmup, a.repeat))
    b = rec['batch']
    rec['us_per_molecule_step'] = round(1e3 * b['remd_run_ms'] / (b['n_ladders'] * b['n_replicas']), 4)
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'remd_aspirin.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
