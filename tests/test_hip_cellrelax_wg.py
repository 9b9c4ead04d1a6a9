"""The workgroup-per-system form of the variable-cell L-BFGS step on the GPU (nnhip_cell_lbfgs_step_wg, csrc/cellrelax.hip;
form='workgroup' / 'auto' of newtonnet_amd/cellrelax.py).

Kernel alone, on the batches of tests/relax_wg_ref.py (tests/test_relax_wg_host.py shows on the CPU that none of their decisions is
ambiguous), memory 4, wg_min_atoms = 0 unless said otherwise, held to cellrelax_ref.check_launch with the workgroup's depth:
  tier A  every variant and load at 0 .. 200 atoms under every option of cellrelax_ref.SYN_OPTIONS and check-only; four variants at
          1023, 1024 and 1025 ROWS (atoms = rows - 3), one system per test item
  tier B  2049 and 5127 atoms, the variants that leave no stored pair
  tier C  the same sizes with accepted pairs on a full history: the prologue has no reduction, so G is the wave form's bit for bit;
          from it, max |x_out - fp64 plain step| of the workgroup form <= max(2 x that of the wave form, one fp32 ulp of 8)
Then routing (wg_min_atoms counts ATOMS), the bitwise properties of a launch, refusals, and the drivers: the acceptance tests of
tests/test_hip_cellrelax.py, verbatim, with every relaxation made under form='workgroup' (the analytic crystal: with every launch
through the new entry point)."""
import math

import numpy as np
import pytest
import torch

from tests import cellrelax_ref as cr
from tests import relax_ref as rr
from tests import relax_wg_ref as wg
from tests import test_hip_cellrelax as base

pytestmark = pytest.mark.gpu

SENT = cr.SENT
INTS = cr.INTS
STATE = base.STATE
ROW_OUT, ATOM_OUT, SYS_OUT = ('x_out', 'G', 'g_prev'), ('pos_out',), ('cell_out', 'fmax', 'rho') + INTS
ULP8 = float(np.spacing(np.float32(8.0)))


def _np(t):
    return t.detach().cpu().numpy()


_same_bits = wg._same_bits


def _call(d, t, bits=cr.MASK_ALL, flags=0, wg_min_atoms=0, **over):
    from newtonnet_amd import hip
    kw = dict(memory=d['memory'], tol2=d['tol2'], alpha=d['alpha'], maxstep=d['maxstep'])
    kw.update(over)
    hip.cell_lbfgs_step(t['X'], t['pos'], t['f'], t['W'], t['cell'], t['h0'], t['free'], t['ptr'], t['p'], t['c'], kw['memory'],
                        kw['tol2'], kw['alpha'], kw['maxstep'], bits, flags, t['converged'], t['n_steps'], t['n_pairs'], t['head'],
                        t['S'], t['Y'], t['rho'], t['g_prev'], t['work'], t['G'], t['x_out'], t['pos_out'], t['cell_out'], t['fmax'],
                        wg_min_atoms=wg_min_atoms)


def _launch(d, bits=cr.MASK_ALL, flags=0, wg_min_atoms=0):
    t = base._tensors(d)
    _call(d, t, bits, flags, wg_min_atoms)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in t.items()}


def _check(d, bits=cr.MASK_ALL, flags=0, label=''):
    out = _launch(d, bits, flags)
    for k in ('X', 'pos', 'f', 'W', 'cell', 'h0', 'ptr', 'p', 'c'):
        assert _same_bits(out[k], d[k]), f'input {k} was modified'
    with wg.workgroup_depth():
        worst, seen, ambiguous = cr.check_launch(d, out, bits, flags)
    print(f'cell_lbfgs_step_wg {label} strain_mask = {bits}, flags = {flags}, {len(d["kinds"])} systems, {d["X"].shape[0]} rows: worst '
          f'err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f' (C_RX = {cr.C_RX}); ambiguous {ambiguous}')
    assert not ambiguous
    return out, seen


@pytest.fixture(scope='module')
def small():
    return wg.cell_small_batch()


# ---- tier A ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('bits,flags', list(cr.SYN_OPTIONS) + [(cr.MASK_ALL, cr.CHECK_ONLY)])
def test_tier_a_every_variant_up_to_200_atoms_against_fp64(small, bits, flags):
    out, seen = _check(small, bits, flags, 'tier A')
    if bits == cr.MASK_ALL and flags == 0:
        for want in ([('accept', 'step', True, False, False), ('accept', 'step', True, True, False), ('accept', 'step', True, True, True),
                      ('first', 'step', None, False, False), ('first', 'step', None, True, False), ('first', 'step', None, True, True),
                      ('converged', 'frozen', None, False, False), ('converging', 'frozen', None, False, False),
                      ('det_neg', 'skip', None, False, False)]
                     + [(k, 'step', False, cl, False) for k in ('reject_neg', 'reject_cos') for cl in (False, True)]):
            assert want in seen, want
    if flags & cr.CHECK_ONLY:
        assert all(s[1] in ('frozen', 'skip') for s in seen)
    assert bool(np.all(out['work'] == np.float32(SENT)))              # up to 1024 rows the work vector is in registers


@pytest.mark.parametrize('v', range(len(wg.EDGE_VARIANTS)))
@pytest.mark.parametrize('rows', wg.CELL_EDGE_ROWS)
def test_tier_a_around_one_row_per_thread_against_fp64(rows, v):
    d = wg.cell_edge_case(rows, v)
    assert d['X'].shape[0] == rows
    out, seen = _check(d, label=f'tier A {wg.EDGE_VARIANTS[v][1]}')
    stepped = any(s[1] == 'step' for s in seen)
    assert stepped == (wg.EDGE_VARIANTS[v][1] != 'converging')
    assert bool(np.all(out['work'] == np.float32(SENT))) == (not stepped or rows <= 1024)


# ---- tier B ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('flags', [0, cr.CHECK_ONLY])
@pytest.mark.parametrize('n', wg.LARGE_SIZES)
def test_tier_b_several_rows_per_thread_against_fp64(n, flags):
    out, seen = _check(wg.cell_large_batch(n), cr.MASK_ALL, flags, 'tier B')
    if flags == 0:
        assert {(k, o, a) for k, o, a, _, _ in seen} == {('first', 'step', None), ('reject_neg', 'step', False),
                                                         ('converged', 'frozen', None), ('converging', 'frozen', None)}


# ---- tier C ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', wg.LARGE_SIZES)
def test_tier_c_full_history_is_no_worse_than_the_wave_form(n):
    d = wg.cell_history_batch(n)
    wave, block = _launch(d, wg_min_atoms=None), _launch(d, wg_min_atoms=0)
    assert _same_bits(wave['G'], block['G']) and _same_bits(wave['g_prev'], block['g_prev'])
    clamps = set()
    for b in range(len(d['kinds'])):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        r0, rc, r1 = cr.rows_of(d, b)
        G32 = block['G'][r0:r1]
        ref = wg.plain_step(d['X'][r0:r1], G32, cr.row_free(d['free'][a0:a1], a1 - a0), cr.batch_state(d, b), 0.0, d['alpha'],
                            d['maxstep'])
        assert ref['accepted'] is True and ref['n_pairs'] == d['memory'] and not ref['frozen']
        clamps.add(ref['clamped'])
        # over all rows, and over the atom rows alone: a cell row is c = n times an entry of F, and half its own fp32 ulp (1.2e-4 at
        # 2049) would hide the atoms
        for rows, sl in (('all rows', slice(r0, r1)), ('atom rows', slice(r0, rc))):
            x64 = ref['x_out'][sl.start - r0:sl.stop - r0]
            e_wave = float(np.abs(wave['x_out'][sl].astype(np.float64) - x64).max())
            e_block = float(np.abs(block['x_out'][sl].astype(np.float64) - x64).max())
            print(f'tier C, {n} atoms, load {d["loads"][b]} ({"clamped" if ref["clamped"] else "free"}), {rows}: max |x_out - fp64| '
                  f'wave {e_wave:.3e}, workgroup {e_block:.3e} (one fp32 ulp of 8: {ULP8:.3e})')
            assert e_block <= max(2.0 * e_wave, ULP8), (rows, e_block, e_wave)
        for k in INTS:
            assert int(block[k][b]) == int(wave[k][b]) == [0, ref['n_steps'], ref['n_pairs'], ref['head']][INTS.index(k)], k
        h0 = int(d['head'][b])
        assert _same_bits(block['Y'][h0, r0:r1], wave['Y'][h0, r0:r1])
        assert _same_bits(block['S'][ref['head'], r0:r1], rr.stored_s(block['x_out'][r0:r1], d['X'][r0:r1]).astype(np.float32))
        # the epilogue from the stored x_out, by the reference's bound
        cell, pos = cr.epilogue(block['x_out'][r0:r1], d['h0'][b], d['c'][b])
        for got, val in ((block['cell_out'][b], cell), (block['pos_out'][a0:a1], pos)):
            assert np.all(np.abs(got.astype(np.float64) - val.v) <= cr.out_bound(val))
    assert clamps == {False, True}


# ---- routing and bitwise properties of a launch -----------------------------------------------------------------------------------------

def _assert_system(one, whole, d, b, what, sliced):
    """system b of `whole` has the bits of `one` (sliced: `one` is a launch of system b alone, else a launch of the whole batch)"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    r0, _, r1 = cr.rows_of(d, b)
    pick_r = (lambda a: a) if sliced else (lambda a: a[r0:r1])
    pick_a = (lambda a: a) if sliced else (lambda a: a[a0:a1])
    pick_b = (lambda a: a) if sliced else (lambda a: a[b:b + 1])
    for k in ROW_OUT:
        assert _same_bits(pick_r(one[k]), whole[k][r0:r1]), f'{what}: {k}'
    for k in ('S', 'Y'):
        assert _same_bits(one[k] if sliced else one[k][:, r0:r1], whole[k][:, r0:r1]), f'{what}: {k}'
    for k in ATOM_OUT:
        assert _same_bits(pick_a(one[k]), whole[k][a0:a1]), f'{what}: {k}'
    for k in SYS_OUT:
        assert _same_bits(pick_b(one[k]), whole[k][b:b + 1]), f'{what}: {k}'


def test_each_system_alone_gives_the_bits_it_gave_in_the_batch_and_a_launch_repeats(small):
    d = small
    bits, flags = 0b111011, cr.CONSTANT_VOLUME
    whole, again = _launch(d, bits, flags), _launch(d, bits, flags)
    for k in ROW_OUT + ATOM_OUT + SYS_OUT + ('S', 'Y'):
        assert _same_bits(whole[k], again[k]), f'the same launch twice: {k}'
    for b in range(len(d['kinds'])):
        _assert_system(_launch(cr.slice_batch(d, b), bits, flags), whole, d, b, f'system {b} ({d["kinds"][b]})', True)


def test_more_systems_than_workgroups():
    d = wg.cell_many_batch()
    assert len(d['kinds']) > 2048
    _check(d, label='many systems')


def test_the_threshold_routes_each_system_by_its_atom_count(small):
    d = small
    wave, block, mixed = _launch(d, wg_min_atoms=None), _launch(d, wg_min_atoms=0), _launch(d, wg_min_atoms=62)
    sizes = np.diff(d['ptr'])
    assert (sizes == 61).any() and (sizes == 62).any()
    differ = 0
    for b, n in enumerate(sizes):
        _assert_system(wave if n < 62 else block, mixed, d, b, f'system {b} ({n} atoms)', False)
        r0, _, r1 = cr.rows_of(d, b)
        differ += not _same_bits(wave['x_out'][r0:r1], block['x_out'][r0:r1])
    assert differ > 0, 'the two forms agree bit for bit everywhere: the routing was not tested'
    none = _launch(d, wg_min_atoms=10 ** 6)
    for k in ROW_OUT + ATOM_OUT + SYS_OUT + ('S', 'Y'):
        assert _same_bits(none[k], wave[k]), k


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def test_cell_lbfgs_step_wg_refuses_what_its_twin_refuses(small):
    from newtonnet_amd import hip
    b = next(i for i, (k, n) in enumerate(zip(small['kinds'], np.diff(small['ptr']))) if k == 'accept' and n == 61)
    d = cr.slice_batch(small, b)
    n, m = d['pos'].shape[0], d['memory']
    t = base._tensors(d)
    keep = {k: v.clone() for k, v in t.items()}
    for alias in (dict(x_out=t['X']), dict(pos_out=t['pos']), dict(cell_out=t['cell'])):
        with pytest.raises(hip.HipLibraryError, match='alias'):
            _call(d, dict(t, **alias))
    with pytest.raises(hip.HipLibraryError, match='memory'):
        _call(d, dict(t, S=t['S'][:0], Y=t['Y'][:0], rho=t['rho'][:, :0]), memory=0)
    with pytest.raises(hip.HipLibraryError, match='flags'):
        _call(d, t, flags=8)
    with pytest.raises(hip.HipLibraryError, match='strain_mask'):
        _call(d, t, bits=64)
    for kw, match in ((dict(alpha=0.0), 'alpha'), (dict(alpha=float('inf')), 'alpha'), (dict(maxstep=float('nan')), 'maxstep'),
                      (dict(maxstep=-0.2), 'maxstep'), (dict(tol2=-1.0), 'tol2')):
        with pytest.raises(hip.HipLibraryError, match=match):
            _call(d, t, **kw)
    L = hip.lib()
    order = ('X', 'pos', 'f', 'W', 'cell', 'h0', 'free', 'ptr', 'p', 'c', 'converged', 'n_steps', 'n_pairs', 'head', 'S', 'Y', 'rho',
             'g_prev', 'work', 'G', 'x_out', 'pos_out', 'cell_out', 'fmax')

    def raw(t, null=(), n_mol=1, n_atoms=n, wg_min_atoms=0):
        p = [None if k in null else hip._ptr(t[k]) for k in order]
        return L.nnhip_cell_lbfgs_step_wg(*p[:10], n_mol, n_atoms, m, d['tol2'], d['alpha'], d['maxstep'], cr.MASK_ALL, wg_min_atoms, 0,
                                          *p[10:], hip._stream(t['X'].device))
    for mode in (0, 62):
        for name in order:
            if name in ('free', 'work'):
                continue                                              # optional (work: only needed above 64 rows)
            assert raw(t, null=(name,), wg_min_atoms=mode) != 0, f'a null {name} was accepted'
            assert b'nnhip_cell_lbfgs_step_wg' in L.nnhip_last_error()
    big = cr.slice_batch(small, next(i for i, (k, s) in enumerate(zip(small['kinds'], np.diff(small['ptr']))) if k == 'accept' and s == 62))
    tb = base._tensors(big)
    assert raw(tb, null=('work',), n_atoms=62) != 0, 'no scratch above 64 rows was accepted'        # (as the twin: work is mandatory)
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(t[k], v), f'{k} was written by a refused call'
    assert all(bool(torch.all(tb[k] == SENT)) for k in ('G', 'x_out', 'pos_out', 'cell_out', 'fmax'))
    assert raw(t, n_mol=0) == 0 and raw(t, null=order, n_mol=0, n_atoms=0) == 0
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(t[k], v), f'{k} was written by an empty launch'
    # a per-system cell_factor or pressure that is not finite (or c <= 0) skips its system and nothing else
    for name, value in (('c', 0.0), ('c', float('nan')), ('p', float('inf'))):
        t2 = base._tensors(d)
        t2[name][0] = value
        _call(d, t2)
        assert math.isnan(float(t2['fmax'][0])) and all(bool(torch.all(t2[k] == SENT)) for k in ('G', 'x_out', 'pos_out', 'cell_out'))
        assert all(torch.equal(t2[k], keep[k]) for k in STATE)


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def workgroup_relaxations(monkeypatch):
    """every model.cell_relaxation(...) and model.relaxation(...) of the test is made with form='workgroup' unless it names a form;
    yields the list of the objects made, for the test to see that they were"""
    from newtonnet_amd.models.newtonnet import NewtonNet
    made = []

    def patched(plain):
        def method(self, *args, **kw):
            kw.setdefault('form', 'workgroup')
            made.append(plain(self, *args, **kw))
            return made[-1]
        return method
    monkeypatch.setattr(NewtonNet, 'cell_relaxation', patched(NewtonNet.cell_relaxation))
    monkeypatch.setattr(NewtonNet, 'relaxation', patched(NewtonNet.relaxation))
    yield made
    assert made and all(r.form == 'workgroup' and r._wg_min_atoms == 0 for r in made)


def test_analytic_crystal_reaches_its_known_minimum_through_the_new_entry(monkeypatch):
    """tests/test_hip_cellrelax.py's analytic crystal with the same acceptance, every launch through nnhip_cell_lbfgs_step_wg"""
    launches = []

    class WorkgroupLoop(base._DeviceLoop):
        def step(self, flags=0):
            from newtonnet_amd import hip
            cur, other = self.cur, 1 - self.cur
            _, f, W = self.efv(self.pos[cur], self.cell[cur])
            self.f, self.W = f, W
            hip.cell_lbfgs_step(self.X[cur], self.pos[cur], f, W, self.cell[cur], self.h0, None, self.ptr, self.p, self.c, *self.num,
                                cr.MASK_ALL, flags, *self.ints, self.S, self.Y, self.rho, self.g_prev, self.work, self.G, self.X[other],
                                self.pos[other], self.cell[other], self.fmax, wg_min_atoms=0)
            self.cur = other
            launches.append(flags)
    monkeypatch.setattr(base, '_DeviceLoop', WorkgroupLoop)
    base.test_analytic_crystal_reaches_its_known_minimum()
    assert len(launches) > 10 and launches[-1] == cr.CHECK_ONLY


def test_every_recorded_step_of_the_boxes_follows_from_the_state_before(workgroup_relaxations):
    """pbc_batch2_rand: 20 recorded steps, each launch held to cellrelax_ref.check_launch with the workgroup's depth"""
    with wg.workgroup_depth():
        base.test_every_recorded_step_follows_from_the_state_before('pbc_batch2_rand', 'virial', dict(pressure=[0.0, 5000.0]))


def test_boxes_converge_like_the_host_fp64_loop(workgroup_relaxations):
    """the existing yardstick: both boxes within 1.5 x the slowest box of the host fp64 loop cellrelax_ref.minimise"""
    base.test_boxes_converge_like_the_host_fp64_loop()


def test_bitwise_properties_of_the_driver(workgroup_relaxations):
    base.test_bitwise_properties()


def test_calculator_relax_cell_in_the_workgroup_form_equals_the_model_path():
    from newtonnet_amd.utils import MLAseCalculator
    from tests import util
    from tests.test_hip_hessian import make_model
    z, pos, cell, batch = base._periodic_case('pbc_batch2_rand')
    model = make_model(util.load_state('rand'), props=('energy', 'gradient_force', 'stress'))
    calc = MLAseCalculator(model, properties=['energy', 'forces', 'stress'], device='cuda')
    n = int((batch == 1).sum())
    sl = batch == 1
    atoms = base.PeriodicAtoms(_np(z[sl]), _np(pos[sl]), _np(cell[1]))
    out = calc.relax_cell(atoms, fmax=0.2, max_steps=15, hydrostatic=True, form='workgroup')
    res = model.cell_relaxation(z[sl], pos[sl], cell[1:2], torch.zeros(n, dtype=torch.long, device='cuda'), fmax=0.2, hydrostatic=True,
                                form='workgroup').run(15, check_every=10)
    assert np.array_equal(out['positions'], _np(res.pos)) and np.array_equal(out['cell'], _np(res.cell)[0])
    assert out['energy'] == _np(res.energy)[0] and out['fmax'] == _np(res.fmax)[0] and out['n_steps'] == _np(res.n_steps)[0]
    wave = calc.relax_cell(atoms, fmax=0.2, max_steps=15, hydrostatic=True)
    auto = calc.relax_cell(atoms, fmax=0.2, max_steps=15, hydrostatic=True, form='auto', wg_min_atoms=n + 1)
    assert all(np.array_equal(auto[k], wave[k]) for k in wave)
    with pytest.raises(ValueError, match='form'):
        calc.relax_cell(atoms, form='block')
