"""The cases of tests/test_hip_node_q.py, run as a script in a child process: results to the .npz named on the command line.
NNHIP_NODE_BWD_Q (and NNHIP_NODE_TURN) are read once per process, so each route is a process of its own; every route runs exactly
this code and the test compares the arrays bit for bit.

Every case is one newtonnet_amd.hip.energy_forces call on a workspace filled with 0xff bytes beforehand.  Recorded: energy, forces,
atom energies, atom_node, force_node, and per layer whether the call wrote the q slot of the workspace (q = f W_u^T: stored by
node_fwd for node_bwd to read, or formed again by node_bwd and never stored) -- which route ran is read from that, not assumed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import util  # noqa: E402

ORDERS = 13      # decades between the first and the last feature of the 'wide' model's force_node rows


def _model(n_layers=3, layer_norm=False, wide=False):
    from newtonnet_amd.models import NewtonNet
    torch.manual_seed(11)
    model = NewtonNet(output_properties=['energy', 'gradient_force'], layer_norm=layer_norm, n_interactions=n_layers)
    sd = {k: v for k, v in util.load_state('rand', torch.float32).items()
          if not k.startswith('interaction_layers.') or int(k.split('.')[1]) < n_layers}
    if wide:
        # force_node[i][c][k] = sum_j phi1_ij[k] u_ij[c] + ...: scaling output feature k of equiv_message{1,2}'s last linear by
        # 10^(-ORDERS k / 127) spreads the 128 values of every f row -- one row of the kernels' 32 x 128 tile -- over ORDERS decades
        s = torch.pow(10.0, -ORDERS * torch.arange(128, dtype=torch.float64) / 127).float()[:, None]
        for l in range(n_layers):
            for m in ('equiv_message1', 'equiv_message2'):
                sd[f'interaction_layers.{l}.{m}.2.weight'] = sd[f'interaction_layers.{l}.{m}.2.weight'] * s
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    if layer_norm:
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for il in model.interaction_layers:
                il.layer_norm.weight.add_(0.1 * torch.randn(128, generator=g))
                il.layer_norm.bias.add_(0.1 * torch.randn(128, generator=g))
    model = model.to('cuda')
    model.eval()
    return model


def _batch(sizes, seed):
    """Molecules of the given sizes cut from perturbed aspirin conformers: the first n atoms of one, and beyond 21 the first n - 21
    again, 3 A away."""
    a = util.load_npz('aspirin_frames.npz')
    g = torch.Generator().manual_seed(seed)
    p0, z0 = torch.from_numpy(a['test0_pos']).float(), torch.from_numpy(a['z']).long()
    zs, ps = [], []
    for n in sizes:
        p = p0 + 0.05 * torch.randn(21, 3, generator=g)
        z, p = torch.cat([z0, z0]), torch.cat([p, p + torch.tensor([3.0, 0.5, -0.5])])
        zs.append(z[:n])
        ps.append(p[:n])
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return torch.cat(zs).cuda(), torch.cat(ps).cuda(), torch.zeros(len(sizes), 3, 3, device='cuda'), batch.cuda()


def _run(out, tag, model, inputs, want_forces=True):
    from newtonnet_amd import hip
    z, pos, cell, batch = inputs
    g = hip.build_graph(pos, cell, batch, 5.0, model.embedding_layers.edge_embedding.embedding.frequencies)
    m = model._hip_model(0)
    N, L = g.n_atoms, m.n_layers
    need = hip.lib().nnhip_workspace_bytes(N, g.n_edges, g.n_mol, L)
    ws = torch.full((max(need, 256),), 255, dtype=torch.uint8, device='cuda')
    res = hip.energy_forces(m, z, pos, cell, g, want_forces=want_forces, workspace=ws)
    torch.cuda.synchronize()
    for k in ('energy', 'forces', 'atom_energy', 'atom_node', 'force_node'):
        if res.get(k) is not None:
            out[f'{tag}.{k}'] = res[k].cpu().numpy()
    lay = hip.workspace_layout(N, g.n_edges, g.n_mol, L)
    out[tag + '.q_written'] = np.array([int((ws[lay.q[l]:lay.q[l] + 12 * N * 128] != 255).any().item()) for l in range(L)])
    out[tag + '.mol_kernels'] = np.array(int(g.n_mol >= hip.config()['molecule_forms']['edge_kernels_from_molecules']))


def run_all(which='all'):
    from newtonnet_amd import hip
    out = {}
    cfg = hip.config()
    out['config.node_bwd_recomputes_q'] = np.array(cfg['node_bwd_recomputes_q'])
    out['config.node_turn_fused'] = np.array(cfg['node_turn_fused'])
    model = _model()
    n33, five = _batch([33], 2), _batch([9, 13, 21, 17, 11], 3)
    _run(out, 'n33', model, n33)
    _run(out, 'five', model, five)
    if which == 'few':
        return out
    _run(out, 'mol3', model, _batch([3], 1))
    _run(out, 'mol640', model, _batch([3] * 640, 4))
    _run(out, 'wide', _model(wide=True), five)
    _run(out, 'layer_norm', _model(layer_norm=True), five)
    _run(out, 'one_layer', _model(n_layers=1), five)
    _run(out, 'energy_only', model, five, want_forces=False)
    return out


if __name__ == '__main__':
    np.savez(sys.argv[1], **run_all(sys.argv[2] if len(sys.argv) > 2 else 'all'))
