"""The library's NNHIP_* switches (csrc/switches.h: one table, read once per process) as nnhip_config reports them, one child process
per environment (no GPU needed: the call only formats text), and that the table, the code and the documents name the same switches."""
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'newtonnet_amd', 'csrc')
ONE_PASS = ('one_pass_adjoint', 'one_pass_forward', 'one_pass_single_adjoint', 'one_pass_single_forward')

# (the variables set, a function of the config that gives what must hold)
CASES = [
    ({'NNHIP_MLP_SPLIT': '0'}, lambda c: (c['split_f16_products'], c['edge_mlp']['row_local_up_to_tiles'],
                                          [c['edge_mlp'][k] for k in ONE_PASS], c['node_turn_fused']) == (0, 1536, [0, 0, 0, 0], 0)),
    ({'NNHIP_MLP_WIDE_TILES': '7'}, lambda c: c['edge_mlp']['row_local_up_to_tiles'] == 7),
    ({'NNHIP_MLP_WIDE_TILES': '0'}, lambda c: c['edge_mlp']['row_local_up_to_tiles'] == 0),
    ({'NNHIP_MLP_WIDE_TILES': '-3'}, lambda c: c['edge_mlp']['row_local_up_to_tiles'] == 832),
    ({'NNHIP_MLP_REGW': '0'}, lambda c: [c['edge_mlp'][k] for k in ONE_PASS] == [0, 0, 0, 0]),
    ({'NNHIP_MLP_REGW': '2'}, lambda c: c['edge_mlp']['one_pass_forward'] == 1),
    ({'NNHIP_MLP_REGW_SINGLE': '0'}, lambda c: [c['edge_mlp'][k] for k in ONE_PASS[2:]] == [0, 0]),
    ({'NNHIP_MLP_REGW_SINGLE': '2'}, lambda c: [c['edge_mlp'][k] for k in ONE_PASS[2:]] == [1, 1]),
    ({'NNHIP_EDGE_SMALL_ATOMS': '0'}, lambda c: c['edge_rows']['four_waves_per_row_up_to_atoms'] == 0),
    ({'NNHIP_MOL_KERNELS_MIN': '700'}, lambda c: c['molecule_forms']['edge_kernels_from_molecules'] == 700),
    ({'NNHIP_FORCE_FWD_MOL': '0'}, lambda c: _forms(c) == dict(_FORMS_ON, force_fwd=0)),
    ({'NNHIP_MSG_BWD_MOL': '0'}, lambda c: _forms(c) == dict(_FORMS_ON, msg_bwd=0, msg_bwd_with_forces=0)),
    ({'NNHIP_FORCE_DIRECT_MOL': '0'}, lambda c: _forms(c) == dict(_FORMS_ON, force_direct=0, msg_bwd_with_forces=0)),
    ({'NNHIP_HEAD_OUT_MOL': '0'}, lambda c: _forms(c) == dict(_FORMS_ON, head_out=0)),
    ({'NNHIP_GRAPH_MOL': '0'}, lambda c: c['neighbor_list']['per_molecule_kernels'] == 0),
    ({'NNHIP_GRAPH_SMALL_ATOMS': '5000'}, lambda c: c['neighbor_list']['single_launch_max_atoms'] == 1024),
    ({'NNHIP_GRAPH_SMALL_ATOMS': '-1'}, lambda c: c['neighbor_list']['single_launch_max_atoms'] == 0),
    ({'NNHIP_FORCE_FWD_MOL': 'abc'}, lambda c: c['molecule_forms']['force_fwd'] == 0),   # atoi('abc') == 0: garbage means off
    ({'NNHIP_FORCE_FWD_MOL': '1'}, lambda c: c['molecule_forms']['force_fwd'] == 1),
]
ECHO = {'NNHIP_FORCE_BWD_OWNER_GU': '0', 'NNHIP_MLP_REGW_TRAIN': '0', 'NNHIP_LIN_BLOCKS': '256', 'NNHIP_TRAIN_BF16': '1'}
_FORMS_ON = dict(force_fwd=1, msg_bwd=1, force_direct=1, head_out=1, msg_bwd_with_forces=1)


def _forms(cfg):
    return {k: cfg['molecule_forms'][k] for k in _FORMS_ON}


def _config(env):
    code = ("import sys, json; sys.path.insert(0, %r)\n"
            "from newtonnet_amd import hip\n"
            "print(json.dumps(hip.config()))\n" % ROOT)
    e = {k: v for k, v in os.environ.items() if not k.startswith('NNHIP_')}
    e.update(env)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=e, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope='module')
def configs():
    """Every environment of this module in a child process of its own (a switch is read once per process), a few at a time."""
    envs = [{}, ECHO] + [env for env, _ in CASES]
    with ThreadPoolExecutor(8) as pool:
        return list(zip(envs, pool.map(_config, envs)))


def test_defaults(configs):
    cfg = configs[0][1]
    assert cfg['edge_rows'] == {'waves_per_row': {'msg_fwd': 2, 'force_fwd': 2, 'force_bwd': 1, 'msg_bwd': 2},
                                'four_waves_per_row_up_to_atoms': 2048}
    assert cfg['molecule_forms'] == dict(_FORMS_ON, max_atoms=24, edge_kernels_from_molecules=640)
    assert cfg['neighbor_list']['single_launch_max_atoms'] == 128 and cfg['neighbor_list']['per_molecule_kernels'] == 1
    assert cfg['edge_mlp'] == {'row_local_up_to_tiles': 832, 'one_pass_adjoint': 1, 'one_pass_forward': 0,
                               'one_pass_single_adjoint': 1, 'one_pass_single_forward': 0}
    assert cfg['split_f16_products'] == 1 and cfg['node_turn_fused'] == 1 and cfg['env'] == {}
    assert cfg['version'] == 113


@pytest.mark.parametrize('k', range(len(CASES)), ids=['%s=%s' % kv for env, _ in CASES for kv in env.items()])
def test_one_switch(configs, k):
    env, holds = CASES[k]
    got_env, cfg = configs[2 + k]
    assert got_env == env and cfg['env'] == env     # "env" echoes what is set, whatever it says
    assert holds(cfg), cfg


def test_echo_is_complete(configs):
    """Switches that change no key of nnhip_config, and one that only the Python package reads, are echoed too."""
    assert configs[1][1]['env'] == ECHO
    assert list(configs[1][1]['env']) == sorted(ECHO)     # keys come out sorted by name


def _table_names():
    with open(os.path.join(CSRC, 'switches.h')) as f:
        return set(re.findall(r'"(NNHIP_[A-Z0-9_]+)"', f.read()))


def test_one_source_of_truth():
    names = _table_names()
    assert {'NNHIP_NODE_TURN', 'NNHIP_MSG_BWD_FORCE', 'NNHIP_TRAIN_BF16'} <= names and len(names) >= 22
    with open(os.path.join(ROOT, 'tools', 'README.md')) as f:
        readme = f.read()
    assert [n for n in sorted(names) if n not in readme] == []
    # the two switches of the fused turn-around stay documented where the others are
    for doc in ('README.md', 'INTEGRATION.md', os.path.join('tools', 'README.md')):
        with open(os.path.join(ROOT, doc)) as f:
            text = f.read()
        for name in ('NNHIP_NODE_TURN', 'NNHIP_MSG_BWD_FORCE'):
            assert name in text, (doc, name)
    # nothing else under csrc/ reads the environment or spells a switch of its own
    for fn in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, fn)
        if fn == 'switches.h' or not os.path.isfile(path):
            continue
        with open(path, errors='replace') as f:
            text = f.read()
        assert 'getenv(' not in text, fn
        assert set(re.findall(r'"(NNHIP_[A-Z0-9_]+)"', text)) <= names, fn
