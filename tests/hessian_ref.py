"""fp64 statement of the Hessian for the tests: H = d^2E/dpos^2 (cell fixed) of the pinned CPU oracle (oracle/newtonnet_ref.py),
by double backward -- the math of the reference's HessianOutput (newtonnet/models/output.py:134-152: grad(-gradient_force, pos)).

Also the input generators the Hessian tests share (jittered aspirins, the ethanol + aspirin pair, the short / long pair geometry)
and the pre-activation margin of a model, so that the CPU-only tests can check them without a device."""
import numpy as np
import torch

from oracle import newtonnet_ref as ref
from tests import util


def oracle_energy(sd, z, pos, cell, batch, cutoff=5.0):
    """energy [B] as a differentiable function of pos (fp64)."""
    n_mol = cell.shape[0]
    edge_index, disp = ref.radius_graph(pos, cell, batch, cutoff)
    freq = sd['embedding_layers.edge_embedding.embedding.frequencies'].to(pos.dtype)
    dist_edge, dir_edge = ref.edge_features(disp, cutoff, freq)
    atom_node = sd['embedding_layers.node_embedding.weight'][z]
    force_node = torch.zeros(z.shape[0], 3, atom_node.shape[1], dtype=pos.dtype)
    for l in range(ref.n_layers(sd)):
        atom_node, force_node = ref.interaction(sd, l, atom_node, force_node, dir_edge, dist_edge, edge_index)
    energy, _ = ref.energy_head(sd, 0, atom_node, z, batch, n_mol)
    return energy


def _select(envelope, activation):
    """envelope: 'polynomial' (p = 9), 'cosine' or ('polynomial', p)"""
    if isinstance(envelope, tuple):
        ref.set_envelope(envelope[0], envelope[1])
    else:
        ref.set_envelope(envelope)
    ref.set_activation(activation)


def _columns(sd, z, pos, cell, batch, cols, dtype):
    p = pos.detach().to(dtype).clone().requires_grad_(True)
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    e = oracle_energy(sdd, z, p, cell.to(dtype), batch).sum()
    (g,) = torch.autograd.grad(e, p, create_graph=True)
    g = g.reshape(-1)
    out = []
    for k in cols:
        (h,) = torch.autograd.grad(g[int(k)], p, retain_graph=True, allow_unused=True)
        out.append(torch.zeros_like(p) if h is None else h.detach())
    out = torch.stack(out) if out else torch.zeros(0, p.shape[0], 3, dtype=dtype)
    return out.to(torch.float64)


def _dense(sd, z, pos, cell, batch, dtype):
    n = pos.shape[0]
    cols = _columns(sd, z, pos, cell, batch, range(3 * n), dtype)
    return cols.reshape(n, 3, n, 3).permute(2, 3, 0, 1).contiguous()   # H[i,a,j,b] = d/dpos_jb (dE/dpos_ia)


def oracle_hessian_columns(sd, z, pos, cell, batch, cols, envelope='polynomial', activation='swish', dtype=torch.float64):
    """Columns H[:, :, cols // 3, cols % 3] as [len(cols), N, 3] (fp64).  dtype=torch.float32 runs the SAME double backward in
    fp32 (inputs and weights rounded once): its error against the fp64 result is the yardstick of what fp32 can give."""
    _select(envelope, activation)
    try:
        return _columns(sd, z, pos, cell, batch, cols, dtype)
    finally:
        _select('polynomial', 'swish')


def oracle_hessian(sd, z, pos, cell, batch, envelope='polynomial', activation='swish', dtype=torch.float64):
    """Dense [N,3,N,3] fp64."""
    _select(envelope, activation)
    try:
        return _dense(sd, z, pos, cell, batch, dtype)
    finally:
        _select('polynomial', 'swish')


def oracle_hessian_per_molecule(sd, z, pos, cell, batch, mols=None, envelope='polynomial', activation='swish', dtype=torch.float64,
                                workers=1):
    """{m: [n_m,3,n_m,3] fp64} -- every molecule ALONE through the oracle (molecules share no edges), so the cost is
    sum n_m^2 rather than (sum n_m)^2 and the oracle never sees a batch larger than one molecule.  workers > 1: the molecules
    on a thread pool (the double backward of one small molecule is a chain of small ops that leaves most cores idle)."""
    mols = [int(m) for m in (range(cell.shape[0]) if mols is None else mols) if int((batch == m).sum()) > 0]

    def one(m):
        idx = (batch == m).nonzero().reshape(-1)
        return _dense(sd, z[idx], pos[idx], cell[m:m + 1], torch.zeros(idx.numel(), dtype=torch.long), dtype)
    _select(envelope, activation)          # once, around the pool: the selection is module state of the oracle
    try:
        if workers > 1 and len(mols) > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(workers) as pool:
                return dict(zip(mols, pool.map(one, mols)))
        return {m: one(m) for m in mols}
    finally:
        _select('polynomial', 'swish')


def dense_from_blocks(blocks, batch):
    """dense [N,3,N,3] fp64 from {m: block} (atoms of a molecule contiguous)"""
    n = batch.numel()
    H = torch.zeros(n, 3, n, 3, dtype=torch.float64)
    for m, blk in blocks.items():
        idx = (batch == m).nonzero().reshape(-1)
        s0, k = int(idx[0]), idx.numel()
        H[s0:s0 + k, :, s0:s0 + k, :] = blk
    return H


def preactivation_margin(sd, z, pos, cell, batch, activation):
    """(row margin, layer margin, activation calls) of the fp64 oracle's forward pass.  Every activation call is one hidden
    layer (the three two-layer MLPs of each interaction layer, both hidden layers of the energy head) on a matrix h [rows, F]:
      row margin   = min over layers, rows and features of |h[r][f]| / max_f |h[r][f]|
      layer margin = min over layers of min |h| / max |h|
    A piecewise-linear activation (relu) takes the same branch in fp32 and fp64 wherever |h| is above the fp32 error of h, and
    that error is relative to the ROW: h[r] = W x[r] carries eps32 sqrt(F) |W| |x[r]|, whatever the other rows hold.  The pair
    rows of the edge MLPs are scaled by the cutoff envelope of their pair (a pair near the cutoff has a row 1e-6 of the largest),
    so the layer margin of an edge MLP is small for every set of weights; the row margin is what a seed can be chosen for."""
    _select('polynomial', activation)
    inner = ref._act
    rows, layers = [], []

    def spy(h):
        a = h.detach().abs().reshape(-1, h.shape[-1])
        if a.numel():
            top = a.max(dim=1, keepdim=True).values
            live = top.reshape(-1) > 0
            rows.append((a[live] / top[live]).min().item() if bool(live.any()) else 1.0)
            layers.append((a.min() / a.max()).item())
        return inner(h)
    ref._act = spy
    try:
        oracle_energy({k: v.double() for k, v in sd.items()}, z, pos.double(), cell.double(), batch)
    finally:
        _select('polynomial', 'swish')
    return min(rows), min(layers), len(rows)


# ---- shared inputs ------------------------------------------------------------------------------------------------------

RELU_SEED = 152      # seed of the randomly initialised models of the activation tests: the row margin of its relu model is 2.3e-5
                     # (test_hessian_host.py asserts it; 24 of the seeds 0 .. 599 reach 1e-5)


def jittered_aspirins(n, seed, spacing=20.0):
    """n copies of the first training frame of aspirin_frames.npz, each with its own N(0, 0.05 A) jitter, on a cubic grid
    `spacing` apart (grid coordinates stay small, so fp32 positions keep 1e-5 A).  z, pos fp32, cell (zeros), batch."""
    a = util.load_npz('aspirin_frames.npz')
    base = torch.from_numpy(a['train_pos'][0]).float()
    zb = torch.from_numpy(a['z']).long()
    gen = torch.Generator().manual_seed(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    k = torch.arange(n)
    origin = spacing * torch.stack([k % side, (k // side) % side, k // (side * side)], dim=1).float()
    pos = base[None] + 0.05 * torch.randn(n, 21, 3, generator=gen) + origin[:, None, :]
    return zb.repeat(n), pos.reshape(-1, 3).contiguous(), torch.zeros(n, 3, 3), torch.repeat_interleave(k, 21)


def ethanol_and_aspirin():
    """one ethanol (9 atoms, ethanol4_rand molecule 0) and one aspirin (21 atoms, aspirin1_rand): z, pos fp32, cell, batch"""
    z1, p1, _, b1, _ = util.case_inputs('ethanol4_rand', torch.float32)
    z2, p2, _, _, _ = util.case_inputs('aspirin1_rand', torch.float32)
    keep = b1 == 0
    z = torch.cat([z1[keep], z2])
    pos = torch.cat([p1[keep], p2 + 30.0])
    batch = torch.cat([torch.zeros(int(keep.sum()), dtype=torch.long), torch.ones(z2.shape[0], dtype=torch.long)])
    return z, pos, torch.zeros(2, 3, 3), batch


def short_and_long_pairs():
    """Six atoms, one molecule: a pair 0.7 A apart (x = 0.14, the small-x end of rbf''), a pair 4.999 A apart (x = 0.9998, where
    the envelope and its derivatives go to zero) and ordinary distances between them.  z, pos fp32, cell, batch."""
    pos = torch.tensor([[0.0, 0.0, 0.0], [0.7, 0.0, 0.0], [0.0, 4.999, 0.0], [1.9, 1.3, 0.4], [-1.2, 2.2, 1.1], [0.9, 3.1, -1.5]])
    d = (pos[:, None] - pos[None]).norm(dim=-1)
    assert abs(d[0, 1].item() - 0.7) < 1e-6 and abs(d[0, 2].item() - 4.999) < 1e-6 and d[0, 2].item() < 5.0
    return torch.tensor([1, 1, 8, 6, 7, 6]), pos, torch.zeros(1, 3, 3), torch.zeros(6, dtype=torch.long)


def pass_count(n_dirs, n_rep):
    """passes of the replica scheme and the live directions of the last one"""
    n = -(-n_dirs // n_rep)
    return n, n_dirs - (n - 1) * n_rep
