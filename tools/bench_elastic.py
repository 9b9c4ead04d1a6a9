"""What the elastic constants cost on one MI355X: 64 crystals of 8 atoms on a 3 x 3 x 3 supercell (216 atoms each, 13 824 in the
batch, randomly initialised weights):
  (a) the six-strain Born step (elastic.born_pass: graph, value sweeps and six strain tangent passes) against six
      model.hessian_vector_product calls on the same batch (each with its own graph and value sweeps), and the six passes alone
      on one prepared batch against six nnhip_hessian_vp passes on it;
  (b) the whole model.elastic_constants call (Born step, force constants, fold, eigensolver, relaxation) against model.phonons
      alone on the same crystals.
Device events, medians of three runs.  Prints one JSON line and writes it to profiles/elastic.json.
usage: python tools/bench_elastic.py [--crystals 64]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_vibrations import event_ms  # noqa: E402

N_ATOMS, S = 8, (3, 3, 3)


def crystals(n_cry, dev):
    """2 x 2 x 2 jittered grids of H, C, O in symmetric cells of about 4.4 A"""
    rng = np.random.default_rng(0)
    grid = np.array([(i, j, k) for i in range(2) for j in range(2) for k in range(2)], dtype=np.float64)
    zs, ps, cs = [], [], []
    for _ in range(n_cry):
        cell = 4.4 * np.eye(3) + 0.15 * rng.standard_normal((3, 3))
        cell = 0.5 * (cell + cell.T)
        ps.append(((grid + 0.25) / 2.0 + 0.04 * rng.standard_normal((N_ATOMS, 3))) @ cell)
        zs.append(rng.choice([1, 6, 8], N_ATOMS))
        cs.append(cell)
    return (torch.tensor(np.concatenate(zs), dtype=torch.long, device=dev), torch.tensor(np.concatenate(ps), dtype=torch.float32, device=dev),
            torch.tensor(np.stack(cs), dtype=torch.float32, device=dev),
            torch.arange(n_cry, device=dev).repeat_interleave(N_ATOMS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--crystals', type=int, default=64)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from newtonnet_amd import elastic as el
    from newtonnet_amd import hessian as nh
    from newtonnet_amd import hip
    from newtonnet_amd import phonons as ph
    from newtonnet_amd.models import NewtonNet
    torch.manual_seed(0)
    model = NewtonNet(output_properties=['energy', 'gradient_force']).to('cuda')
    model.eval()
    z, pos, cell, batch = crystals(a.crystals, 'cuda')
    cells, Sc, counts = ph._checked_crystals(model, z, pos, cell, batch, S, None)
    sc = ph._supercell_batch(z, pos, cells, Sc, counts, pos.device)[:4]
    n = sc[1].shape[0]
    v = torch.randn(n, 3, device='cuda')
    with torch.no_grad():
        born = event_ms(lambda: el.born_pass(model, *sc), 3)
        hvp6 = event_ms(lambda: [nh.hessian_vector_product(model, *sc, v) for _ in range(6)], 3)
        p = nh._Pass(model, *sc, 1, None)
        eta = torch.zeros(a.crystals, 6, device='cuda')
        eta[:, 0] = 1.0
        g, d2, hv = torch.empty(n, 3, device='cuda'), torch.empty(a.crystals, 6, device='cuda'), torch.empty(n, 3, device='cuda')
        strain_only = event_ms(lambda: [nh._strain_pass(p, eta, g, d2) for _ in range(6)], 3)
        hvp_only = event_ms(lambda: [nh._chk(hip.lib().nnhip_hessian_vp(p.model_c, p.ws_c, C.byref(p.h), v.data_ptr(), hv.data_ptr(), p.st),
                                             'nnhip_hessian_vp') for _ in range(6)], 3)
        whole = event_ms(lambda: model.elastic_constants(z, pos, cell, batch, S), 3)
        clamped = event_ms(lambda: model.elastic_constants(z, pos, cell, batch, S, relaxed=False), 3)
        phon = event_ms(lambda: model.phonons(z, pos, cell, batch, S), 3)
        res = model.elastic_constants(z, pos, cell, batch, S)

    def r(t):
        return dict(ms=round(t[0], 3), min_ms=round(t[1], 3), max_ms=round(t[2], 3))
    rec = dict(crystals=a.crystals, atoms_per_cell=N_ATOMS, supercell=list(S), supercell_atoms=n, replicas=nh.replicas_for(n, 6),
               born_six_strains=r(born), six_hvp_calls=r(hvp6), six_strain_passes_alone=r(strain_only), six_hvp_passes_alone=r(hvp_only),
               elastic_constants=r(whole), elastic_constants_clamped=r(clamped), phonons_alone=r(phon),
               status_counts=torch.bincount(res.status.cpu(), minlength=8).tolist(), runs=3, device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line, flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'elastic.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
