"""NNHIP_NODE_BWD_Q (q = f W_u^T formed again in the update adjoint instead of read back), without a GPU: the switch is in the table
and in the documents, nnhip_config reports it and follows it, and the built node_bwd_split_kernel -- both forms -- uses no scratch
memory and leaves room for two workgroups per CU (read from the metadata of the code object inside the built library: tests/codeobj.py)."""
import json
import os
import re
import subprocess
import sys

from tests import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(**env):
    code = ("import sys, json; sys.path.insert(0, %r)\n"
            "from newtonnet_amd import hip\n"
            "print(json.dumps(hip.config()))\n" % ROOT)
    e = {k: v for k, v in os.environ.items() if not k.startswith('NNHIP_')}
    e.update(env)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=e, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_switch_is_in_the_table_and_documented():
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'switches.h')) as f:
        table = f.read()
    assert re.search(r'X\(int, flag, node_bwd_q, "NNHIP_NODE_BWD_Q", 1\)', table)
    for doc in ('README.md', 'INTEGRATION.md', os.path.join('tools', 'README.md')):
        with open(os.path.join(ROOT, doc)) as f:
            assert 'NNHIP_NODE_BWD_Q' in f.read(), doc


def test_config_key_follows_the_switch():
    cfg = _config()
    assert cfg['node_bwd_recomputes_q'] == 1 and cfg['node_turn_fused'] == 1 and cfg['env'] == {} and cfg['version'] == 113
    cfg = _config(NNHIP_NODE_BWD_Q='0')
    assert cfg['node_bwd_recomputes_q'] == 0 and cfg['node_turn_fused'] == 1 and cfg['env'] == {'NNHIP_NODE_BWD_Q': '0'}
    assert _config(NNHIP_NODE_BWD_Q='1')['node_bwd_recomputes_q'] == 1
    assert _config(NNHIP_NODE_BWD_Q='abc')['node_bwd_recomputes_q'] == 0        # a flag: garbage means off
    # the form exists for the split-f16 node kernels only; the turn-around's switch does not touch it
    assert _config(NNHIP_MLP_SPLIT='0')['node_bwd_recomputes_q'] == 0
    cfg = _config(NNHIP_NODE_TURN='0')
    assert cfg['node_bwd_recomputes_q'] == 1 and cfg['node_turn_fused'] == 0
    # a top-level key: the pinned groups keep their keys
    assert 'node_bwd_recomputes_q' not in json.dumps([cfg[k] for k in ('edge_mlp', 'molecule_forms', 'edge_rows', 'neighbor_list')])


def test_built_node_bwd_kernel_uses_no_scratch():
    from newtonnet_amd import hip
    assert os.path.isfile(hip.LIB_PATH), 'the library is not built'
    kernels = codeobj.kernel_metadata(hip.LIB_PATH)
    forms = {n: k for n, k in kernels.items() if n.startswith('_Z21node_bwd_split_kernelILb')}
    assert sorted(forms) == ['_Z21node_bwd_split_kernelILb0EEv11NodeBwdArgs10NodeImages',
                             '_Z21node_bwd_split_kernelILb1EEv11NodeBwdArgs10NodeImages'], sorted(forms)
    for name, k in forms.items():
        print(name, {f: k[f] for f in ('.vgpr_count', '.agpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')})
        assert k['.private_segment_fixed_size'] == 0 and k.get('.vgpr_spill_count', 0) == 0, (name, k)
        # two workgroups of four waves per CU = two waves per SIMD: at most 256 of the 512 registers of a lane, and two LDS
        # allocations within the CU's 160 KiB
        assert k['.vgpr_count'] + k.get('.agpr_count', 0) <= 256, (name, k)
        assert 2 * k['.group_segment_fixed_size'] <= 160 * 1024, (name, k)
    # the recompute form holds a second LDS tile (the f_k tile beside the g_a f_k tile)
    one = forms['_Z21node_bwd_split_kernelILb0EEv11NodeBwdArgs10NodeImages']['.group_segment_fixed_size']
    assert forms['_Z21node_bwd_split_kernelILb1EEv11NodeBwdArgs10NodeImages']['.group_segment_fixed_size'] == 2 * one
