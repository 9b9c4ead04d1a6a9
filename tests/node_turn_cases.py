"""The cases of tests/test_hip_node_turn.py, run in whichever process imports this (or as a script: results to the .npz named on the
command line).  NNHIP_NODE_TURN / NNHIP_MSG_BWD_FORCE are read once per process, so the three-launch route is a child process of the
test; both sides run exactly this code and the test compares the arrays bit for bit.

Every case goes through newtonnet_amd.hip.energy_forces (the ctypes entry points nnhip_energy_forces / nnhip_energy_forces_pp) or the
module's forward, records energy, forces, atom energies, atom_node, force_node, and how many launches the library's timers counted
in the node class ('lin128': the row-local node kernels) and in 'other' (head tail, molecule sums, geometry adjoint)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import util  # noqa: E402


def _model(props=('energy', 'gradient_force'), layer_norm=False, state='rand'):
    from newtonnet_amd.models import NewtonNet
    torch.manual_seed(11)      # (the parameters the state dict does not cover: layer_norm, the direct_force head)
    model = NewtonNet(output_properties=list(props), layer_norm=layer_norm)
    res = model.load_state_dict(util.load_state(state, torch.float32), strict=False)
    assert not res.unexpected_keys
    if layer_norm:             # (nn.LayerNorm starts as the identity affine map: make it a real one)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for il in model.interaction_layers:
                il.layer_norm.weight.add_(0.1 * torch.randn(128, generator=g))
                il.layer_norm.bias.add_(0.1 * torch.randn(128, generator=g))
    model = model.to('cuda')
    model.eval()
    return model


def _aspirin(B, seed, extra=None):
    """B perturbed aspirin conformers (21 atoms each); extra = k: one more molecule of 21 + k atoms (a conformer and k of its atoms
    again, 3 A away) in the middle of the batch."""
    a = util.load_npz('aspirin_frames.npz')
    n = 21
    g = torch.Generator().manual_seed(seed)
    p0, z0 = torch.from_numpy(a['test0_pos']).float(), torch.from_numpy(a['z']).long()
    mols = [(z0, p0 + 0.05 * torch.randn(n, 3, generator=g)) for _ in range(B)]
    if extra:
        zb, pb = mols[0]
        mols.insert(B // 2, (torch.cat([zb, zb[:extra]]), torch.cat([pb + 0.02, pb[:extra] + torch.tensor([3.0, 0.5, -0.5])])))
    z = torch.cat([m[0] for m in mols])
    pos = torch.cat([m[1] for m in mols])
    batch = torch.repeat_interleave(torch.arange(len(mols)), torch.tensor([m[0].shape[0] for m in mols]))
    return z.cuda(), pos.cuda(), torch.zeros(len(mols), 3, 3, device='cuda'), batch.cuda()


def _counts(fn):
    from newtonnet_amd import hip
    torch.cuda.synchronize()
    hip.timers_read(reset=True)
    hip.timers_enable(True, classes=('lin128', 'other'))
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        hip.timers_enable(False)
    t = hip.timers_read(reset=True)
    return res, np.array([t['lin128'][1], t['other'][1]], dtype=np.int64)


def _abi(out, tag, model, inputs, **kw):
    """One hip.energy_forces call (build_graph + the C entry point)."""
    from newtonnet_amd import hip
    z, pos, cell, batch = inputs
    g = hip.build_graph(pos, cell, batch, 5.0, model.embedding_layers.edge_embedding.embedding.frequencies)
    m = model._hip_model(0)
    res, cnt = _counts(lambda: hip.energy_forces(m, z, pos, cell, g, **kw))
    out[tag + '.launches'] = cnt
    out[tag + '.big_molecule'] = np.array(int(bool(g.status & hip.STATUS_BIG_MOLECULE)))
    for k in ('energy', 'forces', 'atom_energy', 'atom_node', 'force_node'):
        if res.get(k) is not None:
            out[f'{tag}.{k}'] = res[k].cpu().numpy()
    if not kw.get('want_nodes', True):   # the node states of the last layer stay in the workspace
        N, L = g.n_atoms, m.n_layers
        lay = hip.workspace_layout(N, g.n_edges, g.n_mol, L)
        ws = res['workspace']
        out[tag + '.atom_node'] = ws[lay.a_out[L - 1]:lay.a_out[L - 1] + 4 * N * 128].view(torch.float32).reshape(N, 128).cpu().numpy()
        out[tag + '.force_node'] = ws[lay.f_out[L - 1]:lay.f_out[L - 1] + 12 * N * 128].view(torch.float32).reshape(N, 3, 128).cpu().numpy()


def _module(out, tag, model, inputs, keys):
    """The module's forward twice: the second call is the deferred step (queued before the host knows the edge count)."""
    for rnd in ('first', 'again'):
        o, cnt = _counts(lambda: model(*inputs))
        for k in keys:
            out[f'{tag}.{rnd}.{k}'] = getattr(o, k).detach().cpu().numpy()
        out[f'{tag}.{rnd}.launches'] = cnt


def run_all(which='all'):
    """which = 'all', or 'mol' (the two batches of the molecule-resident / row regimes only: the child processes that force the
    molecule-resident edge kernels at 64 molecules)."""
    from newtonnet_amd import hip
    out = {}
    cfg = hip.config()
    out['config.node_turn_fused'] = np.array(cfg['node_turn_fused'])
    out['config.msg_bwd_force'] = np.array(cfg['molecule_forms']['msg_bwd_with_forces'])
    model = _model()
    full = ('energy', 'gradient_force', 'atom_node', 'force_node')
    asp64, mixed = _aspirin(64, 3), _aspirin(4, 4, extra=9)
    _abi(out, 'asp64', model, asp64)
    _module(out, 'asp64_module', model, asp64, full)
    _abi(out, 'mixed', model, mixed)
    _module(out, 'mixed_module', model, mixed, full)
    if which == 'mol':
        return out
    z, pos, cell, batch = _aspirin(1, 1)
    _abi(out, 'mol5', model, (z[:5], pos[:5], cell, batch[:5]))
    asp3 = _aspirin(3, 2)
    _abi(out, 'asp3', model, asp3)
    _abi(out, 'asp3_ws_nodes', model, asp3, want_nodes=False)          # atom_node / force_node in the workspace, not the caller's arrays
    _abi(out, 'energy_only', model, asp3, want_forces=False)
    _abi(out, 'layer_norm', _model(layer_norm=True), asp3)
    _module(out, 'direct_force', _model(props=('energy', 'direct_force')), asp3, ('energy', 'direct_force'))
    return out


if __name__ == '__main__':
    np.savez(sys.argv[1], **run_all(sys.argv[2] if len(sys.argv) > 2 else 'all'))
