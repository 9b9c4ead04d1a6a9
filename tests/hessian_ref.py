"""fp64 statement of the Hessian for the tests: H = d^2E/dpos^2 (cell fixed) of the pinned CPU oracle (oracle/newtonnet_ref.py),
by double backward -- the math of the reference's HessianOutput (newtonnet/models/output.py:134-152: grad(-gradient_force, pos))."""
import torch

from oracle import newtonnet_ref as ref


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


def oracle_hessian_columns(sd, z, pos, cell, batch, cols, envelope='polynomial'):
    """Columns H[:, :, cols // 3, cols % 3] as [len(cols), N, 3] (fp64)."""
    ref.set_envelope(envelope)
    try:
        p = pos.detach().to(torch.float64).clone().requires_grad_(True)
        sd64 = {k: v.to(torch.float64) for k, v in sd.items()}
        e = oracle_energy(sd64, z, p, cell.to(torch.float64), batch).sum()
        (g,) = torch.autograd.grad(e, p, create_graph=True)
        g = g.reshape(-1)
        out = []
        for k in cols:
            (h,) = torch.autograd.grad(g[int(k)], p, retain_graph=True, allow_unused=True)
            out.append(torch.zeros_like(p) if h is None else h.detach())
        return torch.stack(out) if out else torch.zeros(0, p.shape[0], 3, dtype=torch.float64)
    finally:
        ref.set_envelope('polynomial')


def oracle_hessian(sd, z, pos, cell, batch, envelope='polynomial'):
    """Dense [N,3,N,3] fp64."""
    n = pos.shape[0]
    cols = oracle_hessian_columns(sd, z, pos, cell, batch, range(3 * n), envelope)
    return cols.reshape(n, 3, n, 3).permute(2, 3, 0, 1).contiguous()   # H[i,a,j,b] = d/dpos_jb (dE/dpos_ia)
