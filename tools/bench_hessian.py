"""Hessians/s and ms per Hessian of NewtonNet.hessian on one MI355X (newtonnet_amd/hessian.py), three cases:
  aspirin1     1 aspirin, replica scheme (R copies of the batch, one direction per copy and pass)
  ethanol32    32 ethanol molecules (replica scheme while R x N stays under the atom budget)
  aspirin1024  1024 aspirin conformers, blocks=True, direction loop (R = 1)
and, beside the first case, the fp64 reference-style CPU path: double backward of the oracle energy, one column per coordinate
(tests/hessian_ref.py; the reference's HessianOutput vmaps the same 3N double-backward calls).
Prints one JSON line per case.  usage: python tools/bench_hessian.py [--reps 5] [--no-cpu]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import util  # noqa: E402


def batch_of(pos_list, z_list):
    z = torch.cat([torch.as_tensor(z).long() for z in z_list])
    pos = torch.cat([torch.as_tensor(p).float() for p in pos_list])
    batch = torch.cat([torch.full((len(zz),), b, dtype=torch.long) for b, zz in enumerate(z_list)])
    cell = torch.zeros(len(z_list), 3, 3)
    return z.cuda(), pos.cuda(), cell.cuda(), batch.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-cpu', action='store_true')
    a = ap.parse_args()
    from newtonnet_amd import hessian as nh
    from newtonnet_amd.models import NewtonNet
    sd = util.load_state('ckpt', torch.float32)
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.load_state_dict(sd, strict=False)
    model = model.cuda()
    model.eval()
    f = util.load_npz('aspirin_frames.npz')
    rng = np.random.default_rng(0)
    asp = [f['train_pos'][k % 8] + rng.normal(scale=0.02, size=(21, 3)) for k in range(1024)]
    e = util.load_npz('case_ethanol4_rand.npz')
    eth_z = e['z'][e['batch'] == 0]
    eth_p = e['pos'][e['batch'] == 0]
    cases = {
        'aspirin1': (batch_of([f['train_pos'][0]], [f['z']]), False),
        'ethanol32': (batch_of([eth_p + rng.normal(scale=0.02, size=eth_p.shape) for _ in range(32)], [eth_z] * 32), False),
        'aspirin1024': (batch_of(asp, [f['z']] * 1024), True),
    }
    for name, (args, blocks) in cases.items():
        n_mol = args[2].shape[0]
        n_dirs = 3 * int(torch.bincount(args[3]).max())
        R = nh.replicas_for(args[1].shape[0], n_dirs)
        model.hessian(*args, blocks=blocks)          # warm-up (code objects, allocator)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            model.hessian(*args, blocks=blocks)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        t = float(np.median(ts))
        rec = dict(case=name, n_mol=n_mol, n_atoms=int(args[1].shape[0]), replicas=R, passes=-(-n_dirs // R),
                   blocks=blocks, ms_per_call=round(1e3 * t, 3), ms_per_hessian=round(1e3 * t / n_mol, 4),
                   hessians_per_s=round(n_mol / t, 1), reps=a.reps, spread_ms=[round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)])
        if name == 'aspirin1' and not a.no_cpu:
            from tests import hessian_ref as hr
            z, pos, cell, batch = (x.cpu() for x in args)
            sd64 = util.load_state('ckpt')
            t0 = time.perf_counter()
            H64 = hr.oracle_hessian(sd64, z, pos.double(), cell.double(), batch)
            rec['cpu_fp64_reference_style_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
            H = model.hessian(*args).cpu().double()
            rec['max_rel_err_vs_fp64'] = float((H - H64).abs().max() / H64.abs().max())
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
