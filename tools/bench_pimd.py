"""What path-integral molecular dynamics costs next to classical batched molecular dynamics on one MI355X: --systems (128) ring
polymers of --beads (8) synthetic aspirin beads each (bench.synthetic_aspirin) and one ring polymer of 8, --steps steps (200) after
--warmup (20), wall clock around a synchronised region (the region and warm-up of tools/bench_md.py), ms per step of
  (a) PathIntegral.run: one model call over all systems x beads molecules and one nnhip_pimd_step launch (csrc/pimd.hip)
  (b) Dynamics.run on the same replicated batch, temperature and friction -- the same model call with nnhip_md_step in the place
      of nnhip_pimd_step: the floor
  (c) single only: Dynamics.run on the one system itself (one molecule), what a classical run of it costs
and the overhead (a - b) / b.  300 K, 0.25 fs, PILE with centroid friction 0.01 / fs (Dynamics: Langevin with the same friction, so
both legs draw one randn per step); seeded weights.  --repeat (3) runs of each leg, interleaved; the figures are the medians and
every run is kept in the record.  Prints one JSON line and writes it to profiles/pimd_aspirin.json (--out).
usage: python tools/bench_pimd.py [--steps 200] [--warmup 20] [--systems 128] [--beads 8] [--repeat 3]"""
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

FRICTION, TEMPERATURE, TIMESTEP = 0.01, 300.0, 0.25


def timed(fn, steps, warmup):
    fn(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def legs(model, n_systems, n_beads, steps, warmup, repeat, alone=False):
    z, pos, cell, batch = bench.synthetic_aspirin(n_systems, 0, 'cuda')
    t_pi, t_dyn, t_one = [], [], []
    for r in range(repeat):
        gen = torch.Generator(device='cuda').manual_seed(r)
        pi = model.path_integral(z, pos, cell, batch, n_beads, TEMPERATURE, timestep=TIMESTEP, centroid_friction=FRICTION, generator=gen)
        t_pi.append(timed(lambda n: pi.run(n), steps, warmup))
        gen = torch.Generator(device='cuda').manual_seed(r)
        dyn = model.dynamics(pi.z, pos.view(n_systems, -1, 3).repeat_interleave(n_beads, 0).reshape(-1, 3), pi.cell, pi.batch,
                             temperature=TEMPERATURE, friction=FRICTION, timestep=TIMESTEP, generator=gen)
        t_dyn.append(timed(lambda n: dyn.run(n), steps, warmup))
        if alone:
            gen = torch.Generator(device='cuda').manual_seed(r)
            one = model.dynamics(z, pos, cell, batch, temperature=TEMPERATURE, friction=FRICTION, timestep=TIMESTEP, generator=gen)
            t_one.append(timed(lambda n: one.run(n), steps, warmup))
    a, b = statistics.median(t_pi), statistics.median(t_dyn)
    rec = dict(n_systems=n_systems, n_beads=n_beads, n_molecules=n_systems * n_beads, n_atoms=int(pi.n_atoms),
               pimd_run_ms=round(a, 4), dynamics_run_ms=round(b, 4), pimd_runs_ms=[round(t, 4) for t in t_pi],
               dynamics_runs_ms=[round(t, 4) for t in t_dyn], us_per_step_over_dynamics=round(1e3 * (a - b), 2),
               overhead_over_dynamics=round((a - b) / b, 4))
    if alone:
        rec.update(dynamics_one_molecule_ms=round(statistics.median(t_one), 4), dynamics_one_molecule_runs_ms=[round(t, 4) for t in t_one])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--systems', type=int, default=128)
    ap.add_argument('--beads', type=int, default=8)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    rec = dict(steps=a.steps, warmup=a.warmup, repeat=a.repeat,
               batch=legs(model, a.systems, a.beads, a.steps, a.warmup, a.repeat),
               single=legs(model, 1, a.beads, a.steps, a.warmup, a.repeat, alone=True))
    b = rec['batch']
    rec['us_per_bead_step'] = round(1e3 * b['pimd_run_ms'] / b['n_molecules'], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'pimd_aspirin.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
