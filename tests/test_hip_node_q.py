"""q = f W_u^T formed again in the update adjoint (csrc/node128s.hip:node_bwd_split_kernel<true>, NNHIP_NODE_BWD_Q=1, the default)
against the stored route (NNHIP_NODE_BWD_Q=0: node_fwd_split_kernel writes q, node_bwd_split_kernel<false> reads it back).

The recompute is the forward's commit and GEMM on the same f tile and the same weight image, so every comparison is BITWISE: energy,
forces, atom energies, atom_node, force_node.  A switch is read once per process: every route is a child process of its own running
tests/node_q_cases.py, one after the other, each under its own time limit, and nothing is started after one that failed.  Which
route a call took is read from the workspace (was the q slot of a layer written?), never assumed.

Shapes: one 3-atom molecule (one ragged tile); 33 atoms (a second tile with one live row); five molecules of 9-21 atoms (71 rows,
molecules across the tile boundaries); 640 molecules of 3 atoms (the molecule-resident edge kernels); a model whose force_node rows
span 12 decades inside one row of the tile (the row scaling of the split-f16 products)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util  # noqa: F401  (the golden fixtures' directory)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ('energy', 'forces', 'atom_energy', 'atom_node', 'force_node')
CHILD_SECONDS = 240      # (a child imports torch, builds three models and runs eight small calls: seconds; the limit is for a hang)


@pytest.fixture(scope='module')
def routes(tmp_path_factory):
    """'q1' / 'q0': NNHIP_NODE_BWD_Q=1 / 0, every case.  'turn0_q1' / 'turn0_q0': the same pair under NNHIP_NODE_TURN=0 (the last
    layer's update adjoint is then a node_bwd launch too), two batches."""
    tmp = str(tmp_path_factory.mktemp('node_q'))
    res = {}
    for name, which, env in (('q1', 'all', {'NNHIP_NODE_BWD_Q': '1'}), ('q0', 'all', {'NNHIP_NODE_BWD_Q': '0'}),
                             ('turn0_q1', 'few', {'NNHIP_NODE_BWD_Q': '1', 'NNHIP_NODE_TURN': '0'}),
                             ('turn0_q0', 'few', {'NNHIP_NODE_BWD_Q': '0', 'NNHIP_NODE_TURN': '0'})):
        path = os.path.join(tmp, name + '.npz')
        e = {k: v for k, v in os.environ.items() if not k.startswith('NNHIP_') or k in ('NNHIP_LIB_NAME', 'NNHIP_ALLOW_TOOLING_LIB')}
        e.update(env)
        # (a failure raises here: the fixture is not run again, so no further child is started after it)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'node_q_cases.py'), path, which], cwd=ROOT, env=e,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_SECONDS)
        assert r.returncode == 0, f'[{name}] exit {r.returncode}: {r.stdout[-3000:]}'
        with np.load(path) as f:
            res[name] = {n: f[n] for n in f.files}
    for name, want_q, want_turn in (('q1', 1, 1), ('q0', 0, 1), ('turn0_q1', 1, 0), ('turn0_q0', 0, 0)):
        assert int(res[name]['config.node_bwd_recomputes_q']) == want_q, name
        assert int(res[name]['config.node_turn_fused']) == want_turn, name
    return res


def _bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _same(a, b, tag, need=ARRAYS):
    for k in need:
        x, y = a[f'{tag}.{k}'], b[f'{tag}.{k}']
        assert x.dtype == y.dtype and x.shape == y.shape, (tag, k)
        assert np.isfinite(x).all(), (tag, k)
        assert np.array_equal(_bits(x), _bits(y)), (tag, k)


@pytest.mark.parametrize('tag', ['mol3', 'n33', 'five', 'mol640'])
def test_recomputed_q_equals_stored_q(routes, tag):
    q1, q0 = routes['q1'], routes['q0']
    _same(q1, q0, tag)
    # three layers, the last one's adjoint inside node_turn_split_kernel on both routes: q[2] is never written, q[0] and q[1] only
    # by the stored route
    assert q1[tag + '.q_written'].tolist() == [0, 0, 0] and q0[tag + '.q_written'].tolist() == [1, 1, 0]
    assert int(q1[tag + '.mol_kernels']) == (1 if tag == 'mol640' else 0)


def test_rows_spanning_twelve_decades(routes):
    """force_node rows whose 128 values span more than 12 decades: the row maximum sets the scale of the f16 pieces, the small
    entries lose their low piece -- on both routes in the same way."""
    q1, q0 = routes['q1'], routes['q0']
    _same(q1, q0, 'wide')
    f = np.abs(q1['wide.force_node'].astype(np.float64))        # [N][3][128]: the f tile of the last layer
    spread = f.max(axis=2) / np.where(f > 0, f, np.inf).min(axis=2)
    print('decades per row: min %.1f max %.1f' % (np.log10(spread.min()), np.log10(spread.max())))
    assert (spread >= 1e12).any(), spread.max()
    assert q1['wide.q_written'].tolist() == [0, 0, 0] and q0['wide.q_written'].tolist() == [1, 1, 0]
    assert not np.array_equal(q1['wide.forces'], q1['five.forces'])


@pytest.mark.parametrize('tag', ['n33', 'five'])
def test_with_the_turn_around_as_three_launches(routes, tag):
    """NNHIP_NODE_TURN=0: the head adjoint + the last layer's update adjoint is a node_bwd launch and recomputes q as well; the
    results are those of the fused turn-around."""
    q1, q0 = routes['turn0_q1'], routes['turn0_q0']
    _same(q1, q0, tag)
    _same(q1, routes['q1'], tag)
    assert q1[tag + '.q_written'].tolist() == [0, 0, 0] and q0[tag + '.q_written'].tolist() == [1, 1, 1]


def test_routes_that_keep_the_stored_q(routes):
    q1, q0 = routes['q1'], routes['q0']
    # LayerNorm after every layer: its adjoint sits between the two halves of node_bwd -- the stored route under both settings
    _same(q1, q0, 'layer_norm')
    assert q1['layer_norm.q_written'].tolist() == [1, 1, 1] and q0['layer_norm.q_written'].tolist() == [1, 1, 1]
    assert not np.array_equal(q1['layer_norm.energy'], q1['five.energy'])
    # one layer: no inter-layer adjoint; the only update adjoint is inside the fused turn-around
    _same(q1, q0, 'one_layer')
    assert q1['one_layer.q_written'].tolist() == [0] and q0['one_layer.q_written'].tolist() == [0]


def test_energy_only_call_stores_no_q(routes):
    q1, q0 = routes['q1'], routes['q0']
    need = ('energy', 'atom_energy', 'atom_node', 'force_node')
    _same(q1, q0, 'energy_only', need)
    assert 'energy_only.forces' not in q1 and 'energy_only.forces' not in q0
    for r in (q1, q0):       # nobody reads q without forces: not written under either setting
        assert r['energy_only.q_written'].tolist() == [0, 0, 0]
    for k in need:           # and the energies are those of the call with forces
        assert np.array_equal(_bits(q1[f'energy_only.{k}']), _bits(q1[f'five.{k}'])), k
