"""NNHIP_NODE_TURN / NNHIP_MSG_BWD_FORCE and their nnhip_config fields (no GPU needed: the call only formats text).  That the
switches are documented where the others are: tests/test_switches_host.py::test_one_source_of_truth."""
import json
import os
import subprocess
import sys

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


def test_defaults_and_switches():
    cfg = _config()
    assert cfg['node_turn_fused'] == 1 and cfg['molecule_forms']['msg_bwd_with_forces'] == 1 and cfg['env'] == {}
    cfg = _config(NNHIP_NODE_TURN='0')
    assert cfg['node_turn_fused'] == 0 and cfg['molecule_forms']['msg_bwd_with_forces'] == 1
    assert cfg['env'] == {'NNHIP_NODE_TURN': '0'}
    cfg = _config(NNHIP_MSG_BWD_FORCE='0')
    assert cfg['node_turn_fused'] == 1 and cfg['molecule_forms']['msg_bwd_with_forces'] == 0
    assert cfg['env'] == {'NNHIP_MSG_BWD_FORCE': '0'}
    # the fused turn-around exists for the split-f16 node kernels only; the tail needs both kernels it joins
    assert _config(NNHIP_MLP_SPLIT='0')['node_turn_fused'] == 0
    assert _config(NNHIP_FORCE_DIRECT_MOL='0')['molecule_forms']['msg_bwd_with_forces'] == 0
    assert _config(NNHIP_MSG_BWD_MOL='0')['molecule_forms']['msg_bwd_with_forces'] == 0
    assert _config(NNHIP_NODE_TURN='1')['node_turn_fused'] == 1

