"""The fp64 yardstick of tests/test_hip_cellrelax.py::test_boxes_converge_like_the_host_fp64_loop, on the CPU.

Runs tests/cellrelax_ref.minimise (the variable-cell L-BFGS of csrc/cellrelax.hip as a plain fp64 loop) on the oracle's fp64 energy,
forces and virial (oracle/newtonnet_ref.py) for the golden case pbc_batch2_rand with the seeded weights, hydrostatic=True, fmax =
0.05 eV/A, at most 300 steps, and prints what the test records as HOST_STEPS: the step count of every system, whether all converged,
and the range of V / V0 on the way.  One evaluation of the oracle takes about half a second, the loop a few minutes -- which is why
the test carries the result instead of running it.

    python tools/cellrelax_host_loop.py [max_steps]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import newtonnet_ref as ref        # noqa: E402
from tests import cellrelax_ref as cr          # noqa: E402
from tests import util                         # noqa: E402


def main():
    max_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    z, pos, cell, batch, _ = util.case_inputs('pbc_batch2_rand', torch.float32)
    sd = {k: v.double() for k, v in util.load_state('rand').items()}
    ptr = np.concatenate([[0], np.cumsum(np.bincount(batch.numpy()))])

    def efv(x, h):
        out = ref.energy_forces(sd, z, torch.from_numpy(x), torch.from_numpy(h), batch)
        return out['energy'].numpy(), out['forces'].numpy(), out['virial'].numpy()
    t0 = time.time()
    res = cr.minimise(efv, pos.numpy().astype(np.float64), cell.numpy().astype(np.float64), ptr, fmax=0.05, max_steps=max_steps,
                      flags=cr.HYDROSTATIC)
    ratio = res['volume_trace'] / res['volume_trace'][0]
    print(f'{len(res["enthalpy_trace"])} evaluations in {time.time() - t0:.0f} s')
    print('converged', res['converged'].tolist(), 'steps', res['n_steps'].tolist(), 'fmax', res['fmax'].tolist())
    print('V / V0: min', ratio.min(0).tolist(), 'max', ratio.max(0).tolist())
    print('enthalpy: first', res['enthalpy_trace'][0].tolist(), 'last', res['enthalpy_trace'][-1].tolist())


if __name__ == '__main__':
    main()
