"""The fused turn-around of the energy+force sweep (csrc/node128s.hip:node_turn_split_kernel) and layer 0's molecule-resident
message adjoint going on with the forces (csrc/edge.hip:msg_bwd_mol_kernel<false, true>) against the launches they replace.

Both keep every operand order of the kernels they replace, so every comparison is BITWISE: energy, forces, atom energies, atom_node,
force_node.  NNHIP_NODE_TURN / NNHIP_MSG_BWD_FORCE are read once per process: the fused route runs in this process, the three-launch
route in a fresh child process running the same code (tests/node_turn_cases.py).  Which route ran is read from the library's launch
counters (timer classes 'lin128' = the row-local node kernels, 'other' = head tail / molecule sums / geometry adjoint), never from
a timing."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util  # noqa: F401  (the golden fixtures' directory)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ('energy', 'forces', 'atom_energy', 'atom_node', 'force_node')


def _child(tmp, name, which, **env):
    path = os.path.join(tmp, name + '.npz')
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', 'node_turn_cases.py'), path, which], cwd=ROOT,
                         env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p, path


@pytest.fixture(scope='module')
def routes(tmp_path_factory):
    """'on': this process (defaults).  'off': NNHIP_NODE_TURN=0 NNHIP_MSG_BWD_FORCE=0.  'mol_on' / 'mol_off': the same pair with the
    molecule-resident edge kernels forced from one molecule up (they start at 640 molecules by default), two batches only."""
    from tests import node_turn_cases
    tmp = str(tmp_path_factory.mktemp('node_turn'))
    off = dict(NNHIP_NODE_TURN='0', NNHIP_MSG_BWD_FORCE='0')
    kids = {'off': _child(tmp, 'off', 'all', **off),
            'mol_on': _child(tmp, 'mol_on', 'mol', NNHIP_MOL_KERNELS_MIN='1'),
            'mol_off': _child(tmp, 'mol_off', 'mol', NNHIP_MOL_KERNELS_MIN='1', **off)}
    res = {'on': node_turn_cases.run_all('all')}
    for k, (p, path) in kids.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, f'[{k}] {log[-3000:]}'
        with np.load(path) as f:
            res[k] = {n: f[n] for n in f.files}
    assert int(res['on']['config.node_turn_fused']) == 1 and int(res['off']['config.node_turn_fused']) == 0
    assert int(res['mol_on']['config.msg_bwd_force']) == 1 and int(res['mol_off']['config.msg_bwd_force']) == 0
    return res


def _same(a, b, tag, keys=ARRAYS, need=ARRAYS):
    seen = []
    for k in keys:
        name = f'{tag}.{k}'
        if name in a or name in b:
            assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, name
            assert np.array_equal(a[name].view(np.uint32 if a[name].dtype == np.float32 else a[name].dtype),
                                  b[name].view(np.uint32 if b[name].dtype == np.float32 else b[name].dtype)), name
            seen.append(k)
    assert set(need) <= set(seen), (tag, seen)


# N = 5: one partial tile.  N = 63: a full tile and a 31-row tail, molecules across the tile boundary.  64 x 21 atoms: 42 tiles,
# the molecule-resident head / force forms.  mixed: a 30-atom molecule, the row regime.
@pytest.mark.parametrize('tag', ['mol5', 'asp3', 'asp64', 'mixed'])
def test_fused_turn_equals_three_launches(routes, tag):
    on, off = routes['on'], routes['off']
    _same(on, off, tag)
    # one node launch less (node_fwd + node_bwd of the last layer -> node_turn); head_out -> mol_energy keeps the 'other' count
    assert on[tag + '.launches'][0] == off[tag + '.launches'][0] - 1, (on[tag + '.launches'], off[tag + '.launches'])
    assert on[tag + '.launches'][1] == off[tag + '.launches'][1]
    assert int(on[tag + '.big_molecule']) == (1 if tag == 'mixed' else 0)


@pytest.mark.parametrize('tag', ['asp64_module', 'mixed_module'])
def test_fused_turn_in_the_deferred_step(routes, tag):
    """The module's forward: the first call is synchronous, the second is queued before the host knows the edge count."""
    keys = ('energy', 'gradient_force', 'atom_node', 'force_node')
    for rnd in ('first', 'again'):
        _same(routes['on'], routes['off'], f'{tag}.{rnd}', keys, keys)
        assert routes['on'][f'{tag}.{rnd}.launches'][0] == routes['off'][f'{tag}.{rnd}.launches'][0] - 1
    for k in keys:
        assert np.array_equal(routes['on'][f'{tag}.first.{k}'], routes['on'][f'{tag}.again.{k}']), k


def test_caller_arrays_and_workspace_nodes_agree(routes):
    """atom_node / force_node written into the caller's arrays (want_nodes) or left in the workspace: the same bits, on both routes."""
    on, off = routes['on'], routes['off']
    _same(on, off, 'asp3_ws_nodes')
    for k in ARRAYS:
        assert np.array_equal(on[f'asp3.{k}'], on[f'asp3_ws_nodes.{k}']), k
    assert on['asp3_ws_nodes.launches'][0] == off['asp3_ws_nodes.launches'][0] - 1


def test_cases_outside_the_fused_route_keep_their_launches(routes):
    on, off = routes['on'], routes['off']
    # energy only: nothing to turn around -- the old forward launches, the same count on both sides
    _same(on, off, 'energy_only', need=('energy', 'atom_energy', 'atom_node', 'force_node'))
    assert 'energy_only.forces' not in on
    assert np.array_equal(on['energy_only.launches'], off['energy_only.launches'])
    assert on['energy_only.launches'][0] == off['asp3.launches'][0] - 3      # (the three node_bwd launches of the reverse sweep)
    assert np.array_equal(on['energy_only.energy'], on['asp3.energy']) and np.array_equal(on['energy_only.atom_energy'], on['asp3.atom_energy'])
    # LayerNorm after the last layer sits between the pieces the fused launch joins
    _same(on, off, 'layer_norm')
    assert np.array_equal(on['layer_norm.launches'], off['layer_norm.launches'])
    assert not np.array_equal(on['layer_norm.energy'], on['asp3.energy'])
    # direct_force: an energy-only sweep, the force head reads atom_node / force_node
    for rnd in ('first', 'again'):
        _same(on, off, f'direct_force.{rnd}', ('energy', 'direct_force'), ('energy', 'direct_force'))
        assert np.array_equal(on[f'direct_force.{rnd}.launches'], off[f'direct_force.{rnd}.launches'])


def test_msg_bwd_with_forces_equals_two_launches(routes):
    """Molecule-resident edge kernels forced on at 64 molecules: layer 0's message adjoint goes on with the geometry adjoint and the
    forces (one 'other' launch less); the batch with a 30-atom molecule must stay on the row kernels and their launches."""
    on, off = routes['mol_on'], routes['mol_off']
    for tag in ('asp64', 'mixed'):
        _same(on, off, tag)
        assert on[tag + '.launches'][0] == off[tag + '.launches'][0] - 1
    assert on['asp64.launches'][1] == off['asp64.launches'][1] - 1, (on['asp64.launches'], off['asp64.launches'])
    assert on['mixed.launches'][1] == off['mixed.launches'][1]
    for tag in ('asp64_module', 'mixed_module'):
        for rnd in ('first', 'again'):
            _same(on, off, f'{tag}.{rnd}', ('energy', 'gradient_force', 'atom_node', 'force_node'), ('energy', 'gradient_force'))
    assert on['asp64_module.again.launches'][1] == off['asp64_module.again.launches'][1] - 1
    assert on['mixed_module.again.launches'][1] == off['mixed_module.again.launches'][1]
    # the default process (row-regime message adjoint at 64 molecules) does not take the tail
    assert routes['on']['asp64.launches'][1] == routes['off']['asp64.launches'][1]


def test_golden_cases_on_the_fused_route():
    """The golden fixtures at tests/test_hip_parity.py's own tolerances with the fused route on (this process): pins the new kernel
    to the fp64 reference, not only to the launches it replaces."""
    from newtonnet_amd import hip
    from tests import test_hip_parity as parity
    assert hip.config()['node_turn_fused'] == 1
    for case in parity.CASES:
        parity.test_golden_case(case)
