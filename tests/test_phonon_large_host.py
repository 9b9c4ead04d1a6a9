"""CPU-side checks of the blocked phonon solver (csrc/phonon_large.hip): the C ABI exports it next to the unchanged one-workgroup
form, the workspace size behaves, the `solver` keyword is validated before anything touches a device, the q-chunk planner covers
every wave vector once, and the fp64 model of the blocked complex iteration (tests/phonon_large_ref.py) reaches the outer stopping
rule -- the CPU-checkable statement of the convergence argument in DESIGN.md 23a."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import phonon_large_ref as plr
from tests import phonon_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('nnhip_phonon_large_max_dim', 'nnhip_phonon_large_ws_bytes', 'nnhip_phonon_bands_large')


def library():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip, ctypes.CDLL(hip.LIB_PATH)


def test_blocked_phonon_symbols_are_declared_listed_and_exported():
    hip, lib = library()
    from newtonnet_amd import abi
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for sym in NEW_SYMBOLS:
        assert sym in declared, f'{sym} is not declared in the header'
        assert sym in abi.FUNCTIONS and sym in hip.EXPORTED_SYMBOLS, f'{sym} is not listed by abi.FUNCTIONS'
        assert hasattr(lib, sym), f'{sym} is not exported'


def test_bounds_of_the_two_forms():
    from newtonnet_amd import elastic, phonons, vibrations
    assert phonons.max_dim_large() == 768 > phonons.max_dim() == 96
    assert elastic.max_dim() == 96 and elastic.max_dim_large() == min(768, vibrations.max_dim_large())


def ws(counts, n_q, modes, select=None):
    hip, _ = library()
    cry = torch.zeros(len(counts) + 1, dtype=torch.int32)
    cry[1:] = torch.cumsum(torch.tensor(counts, dtype=torch.int32), 0)
    sel = None if select is None else torch.tensor(select, dtype=torch.uint8)
    return int(hip.lib().nnhip_phonon_large_ws_bytes(cry.data_ptr(), len(counts), n_q, modes, None if sel is None else sel.data_ptr()))


def test_workspace_size():
    assert ws([33, 43], 4, 1, select=[0, 0]) == 0 and ws([33], 0, 1) == 0 and ws([0], 3, 1) == 0
    one = ws([33], 1, 1)
    # d = 99 pads to 128: A takes 8 x 128^2 bytes, the modes the same again
    assert one >= 16 * 128 * 128 and ws([33], 1, 0) >= 8 * 128 * 128
    assert ws([33], 1, 0) < one <= 4 * ws([33], 1, 0)                     # larger with modes
    sizes = [ws([33], n_q, 1) for n_q in (1, 2, 3, 8)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))                   # monotone in n_q ...
    by_n = [ws([n], 2, 1) for n in (1, 22, 33, 43, 84, 256)]
    assert all(b >= a for a, b in zip(by_n, by_n[1:])) and by_n[-1] > by_n[0]   # ... and in the size
    # a region (one more q of one crystal) is a multiple of 256 bytes, with and without modes
    for n in (1, 33, 43, 256):
        for modes in (0, 1):
            region = ws([n], 9, modes) - ws([n], 8, modes)
            assert region > 0 and region % 256 == 0                        # (the header is rounded to 256 too)
            mp = (3 * n + 63) // 64 * 64
            assert region >= (8 + 8 * modes) * mp * mp
    # blind to what is not selected: the size of the selected crystals alone
    assert ws([33, 10, 43], 3, 1, select=[1, 0, 1]) == ws([33, 43], 3, 1)
    assert ws([33, 300, 43], 3, 1, select=[1, 0, 1]) == ws([33, 43], 3, 1)     # (even one above the bound)
    assert ws([33, 0], 3, 1) == ws([33], 3, 1)
    # one above the bound has no size; 768 coordinates with modes take about 16 Mp^2 bytes
    assert ws([257], 1, 1) == 0
    assert 16 * 768 * 768 <= ws([256], 1, 1) <= 17 * 768 * 768


def test_unknown_solver_is_refused_before_the_device_check():
    from newtonnet_amd import elastic, phonons
    from newtonnet_amd.models import NewtonNet
    fc, pos, cell, S, m = plr.planted_case(2, 3)
    z = np.ones(2, dtype=np.int64)
    msg = "'lds', 'auto', 'blocked'"
    with pytest.raises(ValueError, match=msg):
        phonons.Phonons.from_force_constants(fc, z, pos, cell, S, masses=m, device='cpu', solver='nope')
    for ok in ('lds', 'auto', 'blocked'):          # a known value is kept on the object and gets as far as the device check
        p = phonons.Phonons.from_force_constants(fc, z, pos, cell, S, masses=m, device='cpu', solver=ok)
        assert p.solver == ok
        with pytest.raises(RuntimeError, match='cuda'):
            p.frequencies(np.zeros((1, 3)))
        with pytest.raises(ValueError, match=msg):
            p.frequencies(np.zeros((1, 3)), solver='nope')
        with pytest.raises(ValueError, match=msg):
            p.mesh(1, 1, 1, solver='nope')
        with pytest.raises(ValueError, match=msg):
            p.band_structure([[0, 0, 0], [0.5, 0, 0]], 2, solver='nope')
    model = NewtonNet(output_properties=['energy', 'gradient_force'])
    model.eval()
    z1, pos1, cell1, batch1 = torch.ones(1, dtype=torch.long), torch.zeros(1, 3), 9.0 * torch.eye(3)[None], torch.zeros(1, dtype=torch.long)
    with pytest.raises(ValueError, match=msg):
        model.elastic_constants(z1, pos1, cell1, batch1, solver='nope')
    with pytest.raises(ValueError, match=msg):
        elastic.elastic_constants(model, z1, pos1, cell1, batch1, solver='nope')
    with pytest.raises(ValueError, match=msg):
        model.phonons(z1, pos1, cell1, batch1, (1, 1, 1), solver='nope')
    with pytest.raises(ValueError, match=msg):
        elastic.relaxation_term(torch.zeros(9), torch.zeros(1, dtype=torch.long), [1], torch.zeros(3, 6), solver='nope')


def test_bounds_are_checked_on_the_host():
    """'lds' keeps its refusal and its message above max_dim(); every solver refuses above max_dim_large(), before the device check"""
    from newtonnet_amd import phonons

    def make(n, solver):
        fc = np.zeros((n, 3, n, 3), dtype=np.float32)
        pos = np.random.default_rng(n).uniform(0.0, 9.0, (n, 3))
        return phonons.Phonons.from_force_constants(fc, np.ones(n, dtype=np.int64), pos, 9.0 * np.eye(3), (1, 1, 1), device='cpu',
                                                    solver=solver)
    with pytest.raises(NotImplementedError, match=r'above the 96 of phonons\.max_dim\(\) \(nnhip_phonon_max_dim\)'):
        make(33, 'lds')
    p = make(33, 'auto')
    with pytest.raises(NotImplementedError, match=r'phonons\.max_dim\(\)'):
        p.frequencies(np.zeros((1, 3)), solver='lds')
    for solver in ('lds', 'auto', 'blocked'):
        with pytest.raises(NotImplementedError, match=r'768 of phonons\.max_dim_large\(\)'):
            make(257, solver)


def test_image_table_does_not_depend_on_its_chunking():
    from newtonnet_amd import phonons
    fc, pos, cell, S, m = pr.stage_case(33, 8)
    whole = phonons.image_table(pos, cell, S)
    saved = phonons.IMAGE_TABLE_BYTES
    try:
        phonons.IMAGE_TABLE_BYTES = 1          # one home atom per chunk
        parts = phonons.image_table(pos, cell, S)
    finally:
        phonons.IMAGE_TABLE_BYTES = saved
    assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1])
    table = pr.image_table_fast(pos, cell, S)
    n, N = len(pos), len(pos) * 8
    assert all(np.array_equal(np.array(table[(i, J)]), whole[1][whole[0][i * N + J]:whole[0][i * N + J + 1]])
               for i in range(n) for J in range(N))


@pytest.mark.parametrize('n_q, per_q, budget', [(1, 100, 1), (7, 100, 1), (7, 100, 250), (7, 100, 700), (7, 100, 10 ** 9), (0, 100, 50),
                                                (64, 9437184, 1 << 30)])
def test_q_chunk_planner(n_q, per_q, budget):
    from newtonnet_amd import phonons
    chunks = phonons.plan_q_chunks(n_q, per_q, budget)
    covered = [q for a, b in chunks for q in range(a, b)]
    assert covered == list(range(n_q))                                  # every q once, in order
    assert all(b > a for a, b in chunks)                                # a chunk holds one q at least
    assert all((b - a) * per_q <= budget or b - a == 1 for a, b in chunks)
    if budget >= n_q * per_q and n_q:
        assert len(chunks) == 1


@pytest.mark.parametrize('d', [99, 129])
def test_fp64_model_of_the_blocked_iteration_reaches_the_outer_rule(d):
    fc, pos, cell, S, m = plr.planted_case(d // 3, 100 + d)
    D = pr.dynamical_matrix(fc.astype(np.float64), pos, cell, S, m.astype(np.float64), np.array([0.31, -0.17, 0.44]),
                            pr.image_table_fast(pos, cell, S))
    assert np.abs(D.imag).max() > 1e-3 * np.abs(D).max()                # a genuinely complex problem
    r = plr.block_jacobi(D)
    print(f'd = {d}: {r["sweeps"]} outer sweeps, inner solves of up to {r["inner_max"]} sweeps')
    assert r['converged'] and 1 <= r['sweeps'] <= plr.MAX_SWEEPS
    assert r['inner_max'] < plr.INNER_SWEEPS                            # the inner cap is never what ends a solve
    assert r['padding_zero'] and r['identity_on_padding']               # padding rows and columns stay exactly zero, W = I there
    want = np.linalg.eigvalsh(D)
    scale = np.abs(want).max()
    assert np.abs(r['evals'] - want).max() <= 2.0 ** -24 * d * scale     # the outer rule: off <= 2^-24 ||A||_F (Weyl, loosely)
    V = r['modes']
    assert np.abs(V @ V.conj().T - np.eye(d)).max() <= 1e-9
    assert np.linalg.norm(D @ V.T - V.T * r['evals'][None, :], axis=0).max() <= 2.0 ** -24 * d * scale
