"""CPU-side checks of the workgroup-per-system L-BFGS form (nnhip_lbfgs_step_wg, nnhip_cell_lbfgs_step_wg; form= of the
relaxation drivers): the C ABI exports both entry points and the header's thread count is the Python one; `form` and `wg_min_atoms`
are refused before any device work by all six callables; and the batches the GPU tests launch (tests/relax_wg_ref.py) reach every
branch at every size with NO ambiguous decision, a float32 emulation of the workgroup's reduction order staying inside the fp64
reference's bound at the workgroup's depth -- so the GPU tests can demand every case."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import cellrelax_ref as cr
from tests import relax_ref as rr
from tests import relax_wg_ref as wg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_the_thread_count_are_declared_listed_and_exported():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for name in ('nnhip_lbfgs_step_wg', 'nnhip_cell_lbfgs_step_wg'):
        assert name in declared and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    threads = int(re.search(r'#define NNHIP_LBFGS_WG_THREADS (\S+)', header).group(1))
    assert threads == hip.LBFGS_WG_THREADS == wg.WG_THREADS == 1024
    from newtonnet_amd import relax
    assert relax.FORMS == ('wave', 'workgroup', 'auto') and relax.WG_AUTO_MIN_ATOMS >= 1


def test_the_depth_of_the_workgroup_reduction():
    assert [wg.wg_dot_depth(n) for n in (1, 1024, 1025, 2049, 5127)] == [14, 14, 15, 16, 19]
    # more roundings than the wave form below 193 rows (hence the swap), fewer from 321 on
    assert all(wg.wg_dot_depth(n) > rr.dot_depth(n) for n in range(1, 193))
    assert all(wg.wg_dot_depth(n) < rr.dot_depth(n) for n in range(321, 6000))
    keep = rr.dot_depth
    with wg.workgroup_depth():
        assert rr.dot_depth is wg.wg_dot_depth
    assert rr.dot_depth is keep
    # the emulated reduction: exact on integers, and its order is the workgroup's, not the wave's
    t = np.arange(3000, dtype=np.float32)
    assert wg._block_sum32(t) == t.sum(dtype=np.float64)
    r = np.random.default_rng(3).normal(0, 1, 5000).astype(np.float32)
    assert abs(float(wg._block_sum32(r)) - float(r.astype(np.float64).sum())) <= 19 * rr.EPS32 * float(np.abs(r).sum())
    assert wg._block_sum32(r) != rr._wave_sum32(r)


# ---- form and wg_min_atoms are refused where the other arguments are -------------------------------------------------------------------

class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force', 'virial']


def _inputs(n=3, b=1):
    return (torch.ones(n, dtype=torch.long), torch.zeros(n, 3), torch.eye(3).repeat(b, 1, 1), torch.zeros(n, dtype=torch.long))


BAD_FORMS = ('block', 'WAVE', '', None, 1)
BAD_MIN_ATOMS = (0, -5, 2.5, '64', True, 2 ** 31)


def _drivers():
    from newtonnet_amd.cellrelax import CellRelaxation
    from newtonnet_amd.models.newtonnet import NewtonNet
    from newtonnet_amd.relax import Relaxation
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    model = _FakeModel()
    z, pos, cell, batch = _inputs()
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype = torch.device('cpu'), torch.float32
    calc.model = model
    atoms = FakeAtoms([8, 1, 1], np.zeros((3, 3)))
    return {
        'Relaxation': lambda **kw: Relaxation(model, z, pos, cell, batch, **kw),
        'CellRelaxation': lambda **kw: CellRelaxation(model, z, pos, cell, batch, **kw),
        'model.relaxation': lambda **kw: NewtonNet.relaxation(model, z, pos, cell, batch, **kw),
        'model.cell_relaxation': lambda **kw: NewtonNet.cell_relaxation(model, z, pos, cell, batch, **kw),
        'calc.relax': lambda **kw: calc.relax(atoms, **kw),
        'calc.relax_cell': lambda **kw: calc.relax_cell(atoms, **kw),
    }


@pytest.mark.parametrize('name', ['Relaxation', 'CellRelaxation', 'model.relaxation', 'model.cell_relaxation', 'calc.relax',
                                  'calc.relax_cell'])
def test_form_and_wg_min_atoms_are_refused_before_any_device_work(name):
    make = _drivers()[name]
    for bad in BAD_FORMS:
        with pytest.raises(ValueError, match='form'):
            make(form=bad)
    for bad in BAD_MIN_ATOMS:
        for form in ('auto', 'wave'):
            with pytest.raises(ValueError, match='wg_min_atoms'):
                make(form=form, wg_min_atoms=bad)
    # good values pass every check and reach the refusal of CPU tensors: there is no CPU path, in either form
    for kw in (dict(form='workgroup'), dict(form='auto'), dict(form='auto', wg_min_atoms=22), dict(form='wave', wg_min_atoms=None),
               dict(form='workgroup', wg_min_atoms=np.int64(7))):
        with pytest.raises(RuntimeError, match='MI355X'):
            make(**kw)


def test_check_form_returns_what_the_wrappers_take():
    from newtonnet_amd import relax
    assert relax.check_form('wave', None) is None and relax.check_form('wave', 5) is None
    assert relax.check_form('workgroup', None) == 0 and relax.check_form('workgroup', 300) == 0
    assert relax.check_form('auto', None) == relax.WG_AUTO_MIN_ATOMS and relax.check_form('auto', 22) == 22


def test_the_wrappers_refuse_a_bad_threshold_in_python():
    from newtonnet_amd import hip
    d = wg.relax_batch([(3, 0, 'first', False, False)])
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])) for k in ('x', 'F', 'f_prev', 'S', 'Y', 'rho', 'ptr', 'free') + wg.INTS}
    for bad in (2.5, 'all', 2 ** 31, True):
        with pytest.raises(ValueError, match='wg_min_atoms'):
            hip.lbfgs_step(t['x'], t['F'], t['free'], t['ptr'], 4, d['tol2'], d['alpha'], d['maxstep'], 0, t['converged'],
                           t['n_steps'], t['n_pairs'], t['head'], t['S'], t['Y'], t['rho'], t['f_prev'], None, torch.zeros(3, 3),
                           torch.zeros(1), wg_min_atoms=bad)


# ---- the batches of the GPU tests: every branch, no ambiguous decision, the emulation inside the bound ----------------------------------

def _relax_check(d, flags=0):
    with wg.workgroup_depth():
        worst, seen, ambiguous = wg.check_relax_launch(d, wg.emulate_relax_launch(d, flags), flags)
    assert not ambiguous, ambiguous
    assert max(worst.values()) <= 0.5, worst              # a correct chain shows err / bound <= 0.5 against C_RX = 2
    return worst, seen


BRANCHES = ([('accept', False, True, c) for c in (False, True)] + [('first', False, None, c) for c in (False, True)]
            + [(k, False, False, c) for k in ('reject_neg', 'reject_cos') for c in (False, True)]
            + [('converged', True, None, False), ('converging', True, None, False)])


@pytest.mark.parametrize('flags', [0, rr.CHECK_ONLY])
def test_small_relax_batch_reaches_every_branch_without_an_ambiguous_decision(flags):
    d = wg.relax_small_batch()
    worst, seen = _relax_check(d, flags)
    sizes = np.diff(d['ptr'])
    assert set(sizes.tolist()) == set(wg.SMALL_SIZES) and len(sizes) == len(wg.SMALL_SIZES) * len(rr.SYN_VARIANTS) * 4
    if flags == 0:
        for want in BRANCHES:
            assert want in seen, want
        # every branch at EVERY size: molecule by molecule
        per_size = {}
        with wg.workgroup_depth():
            for b, kind in enumerate(d['kinds']):
                ref = rr.batch_step(d, b, 0)
                per_size.setdefault(int(sizes[b]), set()).add((kind, ref['frozen'], ref['accepted'], ref['clamped']))
        for n in wg.SMALL_SIZES[1:]:
            for want in BRANCHES:
                assert want in per_size[n], (n, want)
    print(f'small relax batch, flags {flags}: emulation worst err / bound {worst}')


@pytest.mark.parametrize('v', range(len(wg.EDGE_VARIANTS)))
@pytest.mark.parametrize('n', wg.EDGE_SIZES)
def test_edge_relax_cases_have_no_ambiguous_decision(n, v):
    d = wg.relax_edge_case(n, v)
    _, seen = _relax_check(d, 0)
    kind = wg.EDGE_VARIANTS[v][1]
    frozen, accepted, _ = next((f, a, c) for k, f, a, c in seen)
    assert frozen == (kind == 'converging') and accepted == {'first': None, 'accept': True, 'reject_neg': False, 'converging': None}[kind]


@pytest.mark.parametrize('n', wg.LARGE_SIZES)
def test_large_relax_batches_have_no_ambiguous_decision(n):
    for flags in (0, rr.CHECK_ONLY):
        _, seen = _relax_check(wg.relax_large_batch(n), flags)
        assert {k for k, _, _, _ in seen} == {k for _, k in wg.NO_PAIR_VARIANTS}
    d = wg.relax_history_batch(n)
    out = wg.emulate_relax_launch(d, 0)
    for b in range(2):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        ref = wg.plain_step(d['x'][a0:a1], d['F'][a0:a1], d['free'][a0:a1], rr.batch_state(d, b), d['tol2'], d['alpha'], d['maxstep'])
        assert ref['accepted'] is True and ref['clamped'] == bool(d['big'][b]) and ref['n_pairs'] == wg.MEMORY
        assert [int(out[k][b]) for k in wg.INTS] == [0, ref['n_steps'], ref['n_pairs'], ref['head']]
        err = float(np.abs(out['pos_out'][a0:a1].astype(np.float64) - ref['x_out']).max())
        assert err <= 4 * float(np.spacing(np.float32(8.0))), err


def test_many_small_systems_have_no_ambiguous_decision():
    d = wg.relax_many_batch()
    assert len(d['kinds']) == 2100 > 2048 and set(np.diff(d['ptr']).tolist()) == {1, 2, 3}
    _relax_check(d)


def test_many_small_cells_have_no_ambiguous_decision():
    c = wg.cell_many_batch()
    assert len(c['kinds']) == 2100
    _cell_check(c)


def test_the_plain_step_is_the_reference_without_its_bounds():
    d = wg.relax_small_batch()
    for b in range(len(d['kinds'])):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        if a1 - a0 > 65:
            continue
        ref = rr.batch_step(d, b, 0, eps=0.0)
        got = wg.plain_step(d['x'][a0:a1], d['F'][a0:a1], d['free'][a0:a1], rr.batch_state(d, b), d['tol2'], d['alpha'], d['maxstep'])
        assert got['frozen'] == ref['frozen'] and got['accepted'] == ref['accepted'] and got['clamped'] == ref['clamped']
        assert [got[k] for k in wg.INTS] == [ref['state'][k] for k in wg.INTS]
        assert np.allclose(got['x_out'], ref['x_out'], rtol=0, atol=1e-12)


def _cell_check(d, bits=cr.MASK_ALL, flags=0):
    with wg.workgroup_depth(), wg.block_emulation():
        worst, seen, ambiguous = cr.check_launch(d, cr.emulate_launch(d, bits, flags), bits, flags)
    assert not ambiguous, ambiguous
    assert max(worst.values()) <= 0.5, worst
    return worst, seen


@pytest.mark.parametrize('bits,flags', list(cr.SYN_OPTIONS) + [(cr.MASK_ALL, cr.CHECK_ONLY)])
def test_small_cell_batch_reaches_every_branch_without_an_ambiguous_decision(bits, flags):
    d = wg.cell_small_batch()
    worst, seen = _cell_check(d, bits, flags)
    if (bits, flags) == (cr.MASK_ALL, 0):
        outcomes = {(k, o, a) for k, o, a, _, _ in seen}
        for want in (('first', 'step', None), ('accept', 'step', True), ('reject_neg', 'step', False), ('reject_cos', 'step', False),
                     ('converged', 'frozen', None), ('converging', 'frozen', None), ('det_neg', 'skip', None)):
            assert want in outcomes, want
        assert any(c and by_cell for _, o, _, c, by_cell in seen if o == 'step'), 'no clamp was decided by a cell row'
        assert any(c and not by_cell for _, o, _, c, by_cell in seen if o == 'step'), 'no clamp was decided by an atom row'
        assert any(not c for _, o, _, c, _ in seen if o == 'step')
    print(f'small cell batch, strain_mask {bits}, flags {flags}: emulation worst err / bound {worst}')


@pytest.mark.parametrize('v', range(len(wg.EDGE_VARIANTS)))
@pytest.mark.parametrize('rows', wg.CELL_EDGE_ROWS)
def test_edge_cell_cases_have_no_ambiguous_decision(rows, v):
    d = wg.cell_edge_case(rows, v)
    assert d['X'].shape[0] == rows
    _cell_check(d)


@pytest.mark.parametrize('n', wg.LARGE_SIZES)
def test_large_cell_batches_have_no_ambiguous_decision(n):
    _cell_check(wg.cell_large_batch(n))
