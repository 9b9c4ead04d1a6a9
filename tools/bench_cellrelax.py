"""What a step of batched variable-cell relaxation costs on one MI355X: the periodic 216-atom box of the test fixtures
(tests/golden/case_pbc216_rand.npz) as --systems (100) independent systems (21 600 atoms, the scale of BASELINE configs[2]), seeded
weights, fmax far below anything the run reaches (no system converges, check_every = 0: every launch is made), --steps steps (200)
after --warmup (20), wall clock around a synchronised region, the median of three runs per leg with the legs taking turns, ms per
step of
  cell  CellRelaxation.run: model() with the virial head + one nnhip_cell_lbfgs_step launch per step (csrc/cellrelax.hip)
  (a)   Relaxation.run with the same model, virial head included: what the n + 3 rows, the 3x3 prologue and the cell buffers add
  (b)   Relaxation.run with a model without the virial head: what the head costs
Prints one JSON line and writes profiles/cellrelax_batch.json (--out-dir).  No pass mark.
usage: python tools/bench_cellrelax.py [--steps 200] [--warmup 20] [--systems 100]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import util  # noqa: E402

KW = dict(fmax=1e-6, memory=16, maxstep=0.2, alpha=70.0)


def make_model(props):
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=list(props))
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    return model


def batch_of_boxes(n_systems):
    z, pos, cell, _, _ = util.case_inputs('pbc216_rand', torch.float32)
    n = pos.shape[0]
    return (z.repeat(n_systems).cuda(), pos.repeat(n_systems, 1).cuda(), cell.repeat(n_systems, 1, 1).cuda(),
            torch.repeat_interleave(torch.arange(n_systems), n).cuda())


def once(make, steps, warmup):
    """ms per step of run(steps, check_every=0) after run(warmup, check_every=0) of a fresh driver"""
    drv = make()
    drv.run(warmup, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = drv.run(steps, 0)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    assert int(res.n_steps.min()) == warmup + steps, 'a system converged: the legs would not make the same launches'
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--systems', type=int, default=100)
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    a = ap.parse_args()
    z, pos, cell, batch = batch_of_boxes(a.systems)
    with_virial, plain = make_model(('energy', 'gradient_force', 'virial')), make_model(('energy', 'gradient_force'))
    legs = dict(cell_relaxation_run_ms=lambda: with_virial.cell_relaxation(z, pos, cell, batch, **KW),
                relaxation_run_with_virial_head_ms=lambda: with_virial.relaxation(z, pos, cell, batch, **KW),
                relaxation_run_without_virial_head_ms=lambda: plain.relaxation(z, pos, cell, batch, **KW))
    times = {k: [] for k in legs}
    for _ in range(3):                       # the legs take turns, so a drift of the clocks falls on all of them alike
        for k, make in legs.items():
            times[k].append(once(make, a.steps, a.warmup))
    rec = dict(case='batch', n_systems=int(cell.shape[0]), n_atoms=int(pos.shape[0]), steps=a.steps, warmup=a.warmup, **KW)
    for k, v in times.items():
        rec[k] = round(statistics.median(v), 4)
        rec[k.replace('_ms', '_runs_ms')] = [round(t, 4) for t in v]
    rec['cell_rows_prologue_and_buffers_add_ms'] = round(rec['cell_relaxation_run_ms'] - rec['relaxation_run_with_virial_head_ms'], 4)
    rec['virial_head_adds_ms'] = round(rec['relaxation_run_with_virial_head_ms'] - rec['relaxation_run_without_virial_head_ms'], 4)
    rec['deferred_stats'] = with_virial.deferred_stats()
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, 'cellrelax_batch.json'), 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
