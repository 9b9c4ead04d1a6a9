"""Analytic Hessians and Hessian-vector products of the energy on the HIP path.

The reference's HessianOutput (newtonnet/models/output.py:134-152) returns H = d^2E/dpos^2 (cell fixed) as a dense [N,3,N,3]
tensor from a torch.vmap of 3N double-backward calls, in train mode only.  Here H v is one tangent-over-reverse pass of the
training kernels along v (include/newtonnet_hip.h: nnhip_hessian_vp; the three stages the training step lacks are in
csrc/hessian.hip), and the Hessian is built from one-hot directions on the device (nnhip_hessian_blocks): molecules never
share edges, so pass k fills column k of EVERY molecule's block at once and 3 max(n_b) passes give every block.

Replica scheme: a small batch would spend its passes waiting on launch latency, so while R x N atoms stay under
REPLICA_ATOM_BUDGET the batch is replicated R times into one graph and one value sweep, and every pass covers R directions,
one per replica.  Large batches take R = 1 (the direction loop).

Eval-only (training on Hessian labels is out of scope), fp32-grade products (no bf16 mode), current parameters on every call.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from newtonnet_amd import hip
from newtonnet_amd import train_fused

REPLICA_ATOM_BUDGET = 16384


def _chk(rc, what):
    if rc != 0:
        raise hip.HipLibraryError(f'{what} failed ({rc}): {hip.lib().nnhip_last_error().decode()}')


def _validate_model(model):
    if model.training:
        raise NotImplementedError('Hessians run in eval mode only (training on Hessian labels is not supported): call model.eval()')
    if 'energy' not in list(model.output_properties):
        raise NotImplementedError("the Hessian is the energy's: the model needs the 'energy' head (output_properties)")


def _validate(model, pos):
    _validate_model(model)
    if not pos.is_cuda:
        raise RuntimeError('newtonnet_amd Hessians run on an MI355X (ROCm) device only: move the model and the inputs to "cuda"')


class _Pass:
    """Values of one (possibly replicated) batch on a workspace without weight-gradient tables, plus the HVP buffers."""

    def __init__(self, model, z, pos, cell, batch, n_rep: int, blk_ptr: Optional[torch.Tensor]):
        emb = model.embedding_layers.edge_embedding
        n0, b0 = pos.shape[0], cell.shape[0]
        zc = z.long().reshape(-1)
        pd = hip._f32c(pos.detach(), 'pos')
        cd = hip._f32c(cell.detach(), 'cell')
        bc = batch.long().reshape(-1)
        if n_rep > 1:
            zc = zc.repeat(n_rep)
            pd = pd.repeat(n_rep, 1)
            cd = cd.repeat(n_rep, 1, 1)
            bc = torch.cat([bc + r * b0 for r in range(n_rep)])
        zc, pd, cd, bc = zc.contiguous(), pd.contiguous(), cd.contiguous(), bc.contiguous()
        with torch.no_grad():
            g = hip.build_graph(pd, cd, bc, emb.cutoff, emb.embedding.frequencies, want_rbf=True, z=zc, envelope=emb.envelope_id)
        ws = train_fused.TrainWorkspace(model, g.n_atoms, max(g.n_edges, 2), g.n_mol, pos.device, wgrad=False)
        runner = train_fused.Runner(model, zc, pd, cd, bc, g, ws)
        self.model_c, self.ws_c = runner._bind()
        ws.c.bf16_wgrad = 0                     # fp32-grade products whatever autocast says
        self.st = hip._stream(pos.device)
        _chk(hip.lib().nnhip_train_values(self.model_c, self.ws_c, self.st), 'nnhip_train_values')
        if C.sizeof(hip.HvpWs) != hip.lib().nnhip_hvp_ws_bytes():
            raise RuntimeError('nnhip_hvp_ws: the ctypes mirror and the library disagree (stale libnewtonnet_hip.so?)')
        L, E, N = ws.L, max(g.n_edges, 1), g.n_atoms

        def buf(*shape):
            return torch.empty(*shape, dtype=torch.float32, device=pos.device)
        self.dg_x, self.dg_u, self.dg_d = buf(L * E), buf(L * E * 4), buf(E, 4)
        self.v, self.hv = buf(max(N, 1), 3), buf(max(N, 1), 3)
        self.zeros_b = torch.zeros(max(g.n_mol, 1), dtype=torch.float32, device=pos.device)
        self.blk_ptr = blk_ptr
        h = self.h = hip.HvpWs()
        for name in ('dg_x', 'dg_u', 'dg_d', 'v', 'hv', 'zeros_b', 'blk_ptr'):
            t = getattr(self, name)
            setattr(h, name, t.data_ptr() if t is not None else None)
        h.n_rep, h.n_mol0 = n_rep, b0
        self.keep = (g, ws, runner, zc, pd, cd, bc)    # every buffer the C views point at stays alive with this object


def hessian_vector_product(model, z, pos, cell, batch, v) -> torch.Tensor:
    """H v [N,3] (fp32) for a direction v [N,3]: d^2E/dpos^2 applied to v, cell held fixed (block-diagonal over molecules)."""
    _validate(model, pos)
    n = pos.shape[0]
    vv = hip._f32c(v.detach().reshape(n, 3), 'v')
    out = torch.empty(n, 3, dtype=torch.float32, device=pos.device)
    if n == 0:
        return out
    p = _Pass(model, z, pos, cell, batch, 1, None)
    _chk(hip.lib().nnhip_hessian_vp(p.model_c, p.ws_c, C.byref(p.h), vv.data_ptr(), out.data_ptr(), p.st), 'nnhip_hessian_vp')
    return out


def voigt_strain(strain, n_mol: int) -> torch.Tensor:
    """[B,6] Voigt components (e1, e2, e3, e4, e5, e6 with engineering shears: e4 = 2 eps_yz, e5 = 2 eps_xz, e6 = 2 eps_xy) of a
    strain given as [B,6] or as symmetric [B,3,3] matrices (ValueError for a matrix that is not symmetric).  The symmetry check
    reads the matrices on the host (18 numbers per system; a strain that lives on the device costs one copy), so that it needs no
    device and raises before any kernel; the [B,6] form is taken as it is."""
    s = strain.detach()
    if tuple(s.shape) == (n_mol, 6):
        return s
    if tuple(s.shape) != (n_mol, 3, 3):
        raise ValueError(f'strain: [{n_mol},3,3] symmetric matrices or [{n_mol},6] Voigt components expected (got {tuple(s.shape)})')
    h = s.double().cpu()
    if n_mol and float((h - h.transpose(1, 2)).abs().max()) > 1e-6 * max(float(h.abs().max()), 1e-30):
        raise ValueError('strain: the matrices are not symmetric (a rotation is no strain); symmetrise them first')
    return torch.stack([s[:, 0, 0], s[:, 1, 1], s[:, 2, 2], s[:, 1, 2] + s[:, 2, 1], s[:, 0, 2] + s[:, 2, 0], s[:, 0, 1] + s[:, 1, 0]],
                       dim=1)


def _strain_pass(p: '_Pass', eta6: torch.Tensor, dgrad: torch.Tensor, d2: torch.Tensor):
    _chk(hip.lib().nnhip_strain_vp(p.model_c, p.ws_c, C.byref(p.h), eta6.data_ptr(), dgrad.data_ptr(), d2.data_ptr(), p.st),
         'nnhip_strain_vp')


def strain_vector_product(model, z, pos, cell, batch, strain) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dgrad [N,3], d2 [B,6]), fp32: the tangent of dE/dpos and of dE/d e_I (I = 1..6, Voigt with engineering shears) along a
    homogeneous strain of every system, x -> (1 + eps_b) x with the cell following.  strain: [B,3,3] symmetric or [B,6] Voigt, of
    any floating dtype and on any device (it is converted to fp32 on the device of pos).
    One tangent-over-reverse pass seeded on the edges (dd_e = eps d_e, periodic shifts included), so it serves molecules
    (cell = 0: the strain is the position direction v_i = eps pos_i) and periodic boxes alike."""
    _validate_model(model)
    n, n_mol = pos.shape[0], cell.shape[0]
    if tuple(pos.shape) != (n, 3) or tuple(cell.shape) != (n_mol, 3, 3) or batch.numel() != n or z.numel() != n:
        raise ValueError('z [N], pos [N,3], cell [B,3,3] and batch [N] expected')
    eta = voigt_strain(strain, n_mol)
    _validate(model, pos)
    eta6 = eta.to(device=pos.device, dtype=torch.float32).contiguous()
    dgrad = torch.zeros(n, 3, dtype=torch.float32, device=pos.device)
    d2 = torch.zeros(n_mol, 6, dtype=torch.float32, device=pos.device)
    if n == 0:
        return dgrad, d2
    _strain_pass(_Pass(model, z, pos, cell, batch, 1, None), eta6, dgrad, d2)
    return dgrad, d2


def replicas_for(n_atoms: int, n_dirs: int) -> int:
    """R of the replica scheme: as many copies of the batch as the atom budget allows, at most one per direction."""
    if n_atoms <= 0 or n_dirs <= 1:
        return 1
    return max(1, min(n_dirs, REPLICA_ATOM_BUDGET // n_atoms))


def hessian_blocks_counts(model, z, pos, cell, batch, replicas: Optional[int] = None,
                          n_dirs: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Packed per-molecule Hessians plus the atom counts: (blocks fp32 [sum_b 9 n_b^2], blk_ptr int64 [B] on the device, counts
    int64 [B] on the CPU); block b = blocks[blk_ptr[b]:][:9 n_b^2] viewed as [n_b, 3, n_b, 3].  `replicas`: R of the replica
    scheme (None: replicas_for).  The counts are what this function brings to the host for blk_ptr anyway; a consumer of the
    blocks (newtonnet_amd/vibrations.py) takes them from here for its own offsets and size checks instead of copying again.
    n_dirs: only the first n_dirs columns of every block are computed (None: all 3 max n_b; the other columns of the returned
    blocks are then not written) -- what newtonnet_amd/phonons.py needs of a supercell's Hessian are its home atoms' columns."""
    _validate(model, pos)
    n_mol = cell.shape[0]
    counts = torch.bincount(batch.long().reshape(-1), minlength=n_mol).cpu() if pos.shape[0] else torch.zeros(n_mol, dtype=torch.long)
    sizes = 9 * counts * counts
    blk_ptr = torch.cumsum(sizes, 0) - sizes
    total = int(sizes.sum())
    blocks = torch.empty(total, dtype=torch.float32, device=pos.device)
    blk_dev = blk_ptr.to(pos.device)
    n_all = 3 * int(counts.max()) if n_mol else 0
    n_dirs = n_all if n_dirs is None else max(0, min(int(n_dirs), n_all))
    if total == 0:
        return blocks, blk_dev, counts
    r = replicas_for(pos.shape[0], n_dirs) if replicas is None else max(1, min(int(replicas), n_dirs))
    p = _Pass(model, z, pos, cell, batch, r, blk_dev)
    _chk(hip.lib().nnhip_hessian_blocks(p.model_c, p.ws_c, C.byref(p.h), n_dirs, blocks.data_ptr(), p.st), 'nnhip_hessian_blocks')
    return blocks, blk_dev, counts


def hessian_blocks(model, z, pos, cell, batch, replicas: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Packed per-molecule Hessians: (blocks fp32 [sum_b 9 n_b^2], blk_ptr int64 [B]); block b = blocks[blk_ptr[b]:][:9 n_b^2]
    viewed as [n_b, 3, n_b, 3].  `replicas`: R of the replica scheme (None: replicas_for)."""
    return hessian_blocks_counts(model, z, pos, cell, batch, replicas)[:2]


def blocks_to_dense(blocks: torch.Tensor, blk_ptr: torch.Tensor, batch: torch.Tensor, n_atoms: int) -> torch.Tensor:
    """The reference's layout: dense [N,3,N,3], zero between molecules."""
    H = torch.zeros(n_atoms, 3, n_atoms, 3, dtype=blocks.dtype, device=blocks.device)
    counts = torch.bincount(batch.long().reshape(-1), minlength=blk_ptr.numel()).tolist()
    ptr = blk_ptr.tolist()
    s = 0
    for b, n in enumerate(counts):
        if n:
            H[s:s + n, :, s:s + n, :] = blocks[ptr[b]:ptr[b] + 9 * n * n].view(n, 3, n, 3)
        s += n
    return H


def hessian(model, z, pos, cell, batch, blocks: bool = False, replicas: Optional[int] = None):
    """blocks=False: dense [N,3,N,3] fp32 (the reference's HessianOutput layout); blocks=True: (blocks, blk_ptr)."""
    blk, ptr = hessian_blocks(model, z, pos, cell, batch, replicas)
    if blocks:
        return blk, ptr
    return blocks_to_dense(blk, ptr, batch, pos.shape[0])
