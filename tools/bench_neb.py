"""What a step of the batched nudged elastic band costs on one MI355X: --bands (128) bands of 8 synthetic aspirin images each
(bench.synthetic_aspirin: the images of a band are 8 jittered aspirins, a path only in the sense of the kernel's arithmetic) and one
band of 8, --steps steps (200) after --warmup (20), wall clock around a synchronised region (the region and warm-up of
tools/bench_md.py and tools/bench_relax.py), ms per step of
  (a) Band.run: model() + one nnhip_neb_step launch per step (csrc/neb.hip), check_every = 0
  (b) a bare loop of model() calls on the same batch, forces and energies touched every step -- the floor
and the launch's share (a - b) / b of the bare step.  fmax is set so low (1e-6 eV/A) that no band converges and freezes inside the
timed region; seeded weights.  Prints one JSON line and writes it to profiles/neb_aspirin.json (--out).
usage: python tools/bench_neb.py [--steps 200] [--warmup 20] [--bands 128] [--images 8]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tests import util  # noqa: E402


def timed(fn, steps, warmup):
    fn(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def legs(model, n_bands, n_images, steps, warmup):
    z, pos, cell, batch = bench.synthetic_aspirin(n_bands * n_images, 0, 'cuda')
    band = model.band(z, pos, cell, batch, n_images, fmax=1e-6)
    t_run = timed(lambda n: band.run(n, check_every=0), steps, warmup)
    res = band.run(0)

    def bare(n):
        for _ in range(n):
            out = model(z, pos, cell, batch)
            out.gradient_force, out.energy
    t_bare = timed(bare, steps, warmup)
    return dict(n_bands=n_bands, n_images=n_images, n_atoms=int(pos.shape[0]), frozen_bands=int(res.converged.sum()),
                climbing_bands=int(res.climbing.sum()), band_run_ms=round(t_run, 4), bare_model_loop_ms=round(t_bare, 4),
                launch_share_of_bare_step=round((t_run - t_bare) / t_bare, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--bands', type=int, default=128)
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd.models import NewtonNet
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(util.load_state('rand', torch.float32), strict=False)
    model = model.cuda()
    model.eval()
    rec = dict(steps=a.steps, warmup=a.warmup, batch=legs(model, a.bands, a.images, a.steps, a.warmup),
               single=legs(model, 1, a.images, a.steps, a.warmup))
    b = rec['batch']
    rec['us_per_image_step'] = round(1e3 * b['band_run_ms'] / (b['n_bands'] * b['n_images']), 4)
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'neb_aspirin.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
