"""What an evaluation of the batched dimer-method saddle search costs on one MI355X, and what refining a band's climbing image with
it saves over tightening the band.

(1) 1024 synthetic aspirins (bench.synthetic_aspirin) and one aspirin, seeded weights, a seeded random direction per molecule:
--steps evaluations (200) after --warmup (20), wall clock around a synchronised region (the region and warm-up of
tools/bench_irc.py), ms per evaluation of
  (a) SaddleSearch.run: model() + one nnhip_dimer_step launch per evaluation (csrc/dimer.hip), check_every = 0, record_every = 0
  (b) a bare loop of model() calls on the same batch, forces touched every step -- the floor
each the MEDIAN of --repeats (3) runs taken alternately, and the launch's share (a - b) / b of the bare step.  fmax is 1e-6 eV/A so
that no molecule converges inside the timed region (the converged ones are counted; expected: 0).  A translate launch walks the
L-BFGS history, a rotate launch does not: the share of translate launches among the molecule-launches of the timed region is reported
(translations taken / evaluations consumed).
(2) The aspirin methyl-rotation saddle of tests/test_hip_dimer.py, shipped weights: the 7-image band stopped at its usual 0.01
eV/A, then (a) saddle_search from its climbing image along its tangent to fmax = 0.0005 eV/A, against (b) the same band run on to
0.0005 eV/A itself -- force evaluations (a band step is 7) and wall time of each, one run each after a warm-up run.
Prints one JSON line and writes it to profiles/dimer_aspirin.json (--out).
usage: python tools/bench_dimer.py [--steps 200] [--warmup 20] [--mols 1024] [--repeats 3]"""
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
from tests import neb_ref, util  # noqa: E402


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def legs(model, inputs, steps, warmup, repeats):
    z, pos, cell, batch = inputs
    direction = torch.randn(pos.shape, generator=torch.Generator().manual_seed(0)).to(pos.device)
    search = model.saddle_search(z, pos, cell, batch, direction=direction, fmax=1e-6)

    def run(n):
        search.run(n, check_every=0, record_every=0)

    def bare(n):
        for _ in range(n):
            model(z, pos, cell, batch).gradient_force
    run(warmup)
    bare(warmup)
    before = search.run(0)
    t_run, t_bare = [], []
    for _ in range(repeats):
        t_run.append(timed(run, steps))
        t_bare.append(timed(bare, steps))
    res = search.run(0)
    a, b = statistics.median(t_run), statistics.median(t_bare)
    evals = int((res.n_evaluations - before.n_evaluations).sum())
    return dict(n_mol=int(search.n_mol), n_atoms=int(search.n_atoms), converged=int(res.converged.sum()),
                translate_share_of_launches=round(int((res.n_steps - before.n_steps).sum()) / max(evals, 1), 4),
                rotations_per_translation=round(int((res.n_rotations - before.n_rotations).sum())
                                                / max(int((res.n_steps - before.n_steps).sum()), 1), 3),
                saddle_search_run_ms=round(a, 4), bare_model_loop_ms=round(b, 4), runs_ms=[round(t, 4) for t in t_run],
                bare_ms=[round(t, 4) for t in t_bare], launch_share_of_bare_step=round((a - b) / b, 4))


def refinement():
    """the band stopped at 0.01 eV/A, then the dimer against the band itself, both to 0.0005 eV/A"""
    from tests.test_hip_hessian import cuda, make_model
    z, pos, cell, batch, _ = util.case_inputs('aspirin8_ckpt', torch.float32)
    z, pos, cell, batch = cuda(z, pos, cell, batch)
    model = make_model(util.load_state('ckpt'))
    z1, c1, b1 = z[:21].contiguous(), cell[:1].contiguous(), batch[:21].contiguous()
    A = model.relaxation(z1, pos[:21], c1, b1).run(600, check_every=10).pos
    x0 = neb_ref.methyl_rotation_band(z1.cpu().numpy(), A.cpu().numpy().astype(np.float64), 7).astype(np.float32)
    x0 = torch.from_numpy(x0.reshape(-1, 3)).cuda()
    bb = torch.arange(7, device='cuda').repeat_interleave(21)
    c7 = torch.zeros(7, 3, 3, device='cuda')

    def band_to(fmax, steps):
        band = model.band(z1.repeat(7), x0, c7, bb, 7, spring=0.1, fmax=fmax, climb_below=0.05)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = band.run(steps, check_every=10)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def dimer_from(out):
        top = int(out.saddle_image[0])
        sl = slice(21 * top, 21 * (top + 1))
        search = model.saddle_search(z1, out.pos[sl].clone(), c1, b1, direction=out.tangent[sl].clone(), fmax=0.0005)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = search.run(2000, check_every=10)
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0
    loose, t_loose = band_to(0.01, 1000)
    dimer_from(loose)                                        # warm-up of both legs
    band_to(0.0005, 100)
    loose, t_loose = band_to(0.01, 1000)
    res, t_dimer = dimer_from(loose)
    tight, t_tight = band_to(0.0005, 6000)
    f_true = float(model(z1, res.pos.clone(), c1, b1).gradient_force.norm(dim=1).max())
    return dict(band_to_0p01=dict(steps=int(loose.n_steps[0]), evaluations=7 * int(loose.n_steps[0]), converged=bool(loose.converged[0]),
                                  wall_s=round(t_loose, 4)),
                dimer_to_0p0005=dict(evaluations=int(res.n_evaluations[0]), translations=int(res.n_steps[0]),
                                     rotations=int(res.n_rotations[0]), converged=bool(res.converged[0]), true_fmax=round(f_true, 7),
                                     curvature=round(float(res.curvature[0]), 5), wall_s=round(t_dimer, 4)),
                band_to_0p0005=dict(steps=int(tight.n_steps[0]), evaluations=7 * int(tight.n_steps[0]),
                                    evaluations_beyond_0p01=7 * (int(tight.n_steps[0]) - int(loose.n_steps[0])),
                                    converged=bool(tight.converged[0]), wall_s=round(t_tight, 4)))


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
    rec['us_per_molecule_evaluation'] = round(1e3 * b['saddle_search_run_ms'] / b['n_mol'], 4)
    rec['refinement'] = refinement()
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'dimer_aspirin.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
