"""What the bias on collective variables adds to a step of batched molecular dynamics on one MI355X: synthetic aspirin walkers
(bench.synthetic_aspirin) in three shapes -- 1 group of 1024 walkers, 128 groups of 8 and one group of 8 -- each with 0, about 1e4
and about 1e5 hills in every group's list, --steps steps (200) after --warmup (20), wall clock around a synchronised region (the
region and warm-up of tools/bench_md.py), ms per step of
  (a) Metadynamics.run: Dynamics's step plus one nnhip_bias_step launch (csrc/bias.hip) -- a torsion and a distance, their
      gradients, the sum over the group's hills, two restraints, the chain rule -- per step
  (b) Dynamics.run on the same replicated batch with the same friction, on the same commit -- the same model call and the same
      randn: the floor
and the difference in microseconds per step.  The hills are written into the list before the timed region (centres scattered
around the walkers' starting values) and nothing is deposited in it, so every timed step sums the stated number of hills.  300 K;
friction 0.01 / fs; seeded weights.  --repeat (3) runs of each leg, interleaved; the figures are the medians and every run is kept
in the record.  Prints one JSON line and writes it to profiles/metad_aspirin.json (--out).
usage: python tools/bench_metad.py [--steps 200] [--warmup 20] [--repeat 3]"""
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

FRICTION = 0.01
CVS = [('torsion', 1, 6, 10, 8), ('distance', 7, 12)]
SHAPES = ((1, 1024), (128, 8), (1, 8))            # (groups, walkers)
HILLS = (0, 10 ** 4, 10 ** 5)


def timed(fn, steps, warmup):
    fn(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def with_hills(meta, n_hills, seed):
    """about n_hills hills in every group's list: whole deposits of W hills, centres around the walkers' current values"""
    W = meta.n_walkers
    deposits = -(-n_hills // W)
    meta._reserve(deposits)
    H = deposits * W
    gen = torch.Generator(device='cuda').manual_seed(seed)
    cv = meta.collective_variables.view(meta.n_systems, W, 2).mean(1, keepdim=True)
    rows = meta._hills[:, :H]
    rows[:, :, :2] = cv + torch.randn((meta.n_systems, H, 2), generator=gen, device='cuda') * torch.tensor([0.5, 0.2], device='cuda')
    rows[:, :, 2] = 1e-3 / max(deposits, 1)
    meta.n_deposits = deposits
    meta._force = None                               # the state is evaluated again, under the hills
    return H


def legs(model, n_groups, n_walkers, steps, warmup, repeat):
    z, pos, cell, batch = bench.synthetic_aspirin(n_groups, 0, 'cuda')
    out = dict(n_groups=n_groups, n_walkers=n_walkers, hills=[])
    for n_hills in HILLS:
        t_meta, t_dyn = [], []
        for r in range(repeat):
            gen = torch.Generator(device='cuda').manual_seed(r)
            meta = model.metadynamics(z, pos, cell, batch, CVS, 300.0, FRICTION, 0.01, [0.35, 0.1], 0, bias_factor=8.0,
                                      walkers=n_walkers, restraint_k=[0.5, 2.0], restraint_center=[0.0, 3.0], generator=gen)
            H = with_hills(meta, n_hills, r)
            t_meta.append(timed(lambda n: meta.run(n), steps, warmup))
            gen = torch.Generator(device='cuda').manual_seed(r)
            dyn = model.dynamics(meta.z, pos.view(n_groups, -1, 3).repeat_interleave(n_walkers, 0).reshape(-1, 3), meta.cell,
                                 meta.batch, temperature=300.0, friction=FRICTION, generator=gen)
            t_dyn.append(timed(lambda n: dyn.run(n), steps, warmup))
        a, b = statistics.median(t_meta), statistics.median(t_dyn)
        out['n_atoms'] = int(meta.n_atoms)
        out['hills'].append(dict(hills_per_group=H, metad_run_ms=round(a, 4), dynamics_run_ms=round(b, 4),
                                 metad_runs_ms=[round(t, 4) for t in t_meta], dynamics_runs_ms=[round(t, 4) for t in t_dyn],
                                 us_per_step_added=round(1e3 * (a - b), 2), share_of_dynamics_step=round((a - b) / b, 4),
                                 status_bits=int(meta.status.sum())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    rec = dict(steps=a.steps, warmup=a.warmup, repeat=a.repeat, cvs=[list(cv) for cv in CVS],
               shapes=[legs(model, g, w, a.steps, a.warmup, a.repeat) for g, w in SHAPES])
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'metad_aspirin.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
