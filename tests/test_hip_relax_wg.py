"""The workgroup-per-system form of the L-BFGS step on the GPU (nnhip_lbfgs_step_wg, csrc/relax.hip; form='workgroup' / 'auto' of
newtonnet_amd/relax.py).

Kernel alone, on the batches of tests/relax_wg_ref.py (tests/test_relax_wg_host.py shows on the CPU that none of their decisions is
ambiguous), memory 4, wg_min_atoms = 0 unless said otherwise:
  tier A  against the fp64 restatement with the workgroup's depth, by the yardstick of tests/test_hip_relax.py (every output within
          bound + half an fp32 ulp, integers and flags exact, y and S[head] bitwise, everything a step must not touch bitwise
          untouched): every variant at 0 .. 200 atoms, four variants at 1023, 1024, 1025 atoms (one molecule per test item: the
          reference of a stored pair builds dense 3n x 3n maps)
  tier B  2049 and 5127 atoms (3 and 6 rows per thread, the last pass partial), the variants that leave no stored pair, where the
          reference needs no dense map: the multi-row sums, the max, the clamp, all stores
  tier C  the same sizes with accepted pairs on a full history against a plain fp64 step; the yardstick is the WAVE kernel on the
          same inputs:  max |x_out - fp64| of the workgroup form <= max(2 x that of the wave form, one fp32 ulp of 8).  The workgroup
          form's sums are shallower there (16 roundings against 42 at 2049 atoms), so a correct kernel is expected to be no worse;
          the factor 2 only allows for a different realisation of the roundings.
Then routing (wg_min_atoms), the bitwise properties of a launch, refusals, and the drivers: the acceptance tests of
tests/test_hip_relax.py, verbatim, with every relaxation made under form='workgroup'."""
import numpy as np
import pytest
import torch

from tests import relax_ref as rr
from tests import relax_wg_ref as wg
from tests import test_hip_relax as base

pytestmark = pytest.mark.gpu

SENT = wg.SENT
INTS = wg.INTS
OUT = ('pos_out', 'fmax', 'S', 'Y', 'rho', 'f_prev') + INTS
ULP8 = float(np.spacing(np.float32(8.0)))


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return wg._same_bits(a, b)


def _tensors(d):
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ('x', 'F', 'f_prev', 'S', 'Y', 'rho', 'ptr', 'free') + INTS}
    N, B = d['x'].shape[0], len(d['ptr']) - 1
    t.update(pos_out=torch.full((N, 3), SENT, device='cuda'), fmax=torch.full((B,), SENT, device='cuda'),
             work=torch.full((N, 3), SENT, device='cuda'))
    return t


def _call(d, t, flags=0, wg_min_atoms=0, **over):
    from newtonnet_amd import hip
    kw = dict(memory=d['memory'], tol2=d['tol2'], alpha=d['alpha'], maxstep=d['maxstep'])
    kw.update(over)
    hip.lbfgs_step(t['x'], t['F'], t['free'], t['ptr'], kw['memory'], kw['tol2'], kw['alpha'], kw['maxstep'], flags, t['converged'],
                   t['n_steps'], t['n_pairs'], t['head'], t['S'], t['Y'], t['rho'], t['f_prev'], t['work'], t['pos_out'], t['fmax'],
                   wg_min_atoms=wg_min_atoms)


def _launch(d, flags=0, wg_min_atoms=0):
    """one launch on a batch in the kernel's layout (wg_min_atoms None: the wave entry point); returns the inputs as they are
    afterwards and the sentinel-filled outputs, as numpy arrays"""
    t = _tensors(d)
    _call(d, t, flags, wg_min_atoms)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in t.items()}


def _check(d, flags=0, label=''):
    out = _launch(d, flags)
    for k in ('x', 'F', 'ptr', 'free'):
        assert _same_bits(out[k], d[k]), f'input {k} was modified'
    with wg.workgroup_depth():
        worst, seen, ambiguous = wg.check_relax_launch(d, out, flags)
    print(f'lbfgs_step_wg {label} flags = {flags}, {len(d["kinds"])} molecules, {d["x"].shape[0]} atoms: worst err / bound '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f' (C_RX = {rr.C_RX}); ambiguous {ambiguous}')
    assert not ambiguous
    return out, seen


@pytest.fixture(scope='module')
def small():
    return wg.relax_small_batch()


# ---- tier A ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('flags', [0, rr.CHECK_ONLY])
def test_tier_a_every_variant_up_to_200_atoms_against_fp64(small, flags):
    out, seen = _check(small, flags, 'tier A')
    if flags == 0:
        for want in ([('accept', False, True, c) for c in (False, True)] + [('first', False, None, c) for c in (False, True)]
                     + [(k, False, False, c) for k in ('reject_neg', 'reject_cos') for c in (False, True)]
                     + [('converged', True, None, False), ('converging', True, None, False)]):
            assert want in seen, want
    else:
        assert all(frozen for _, frozen, _, _ in seen)
    # the scratch vector belongs to molecules above 1024 atoms alone: here no word of it is written
    assert bool(np.all(out['work'] == np.float32(SENT)))


@pytest.mark.parametrize('v', range(len(wg.EDGE_VARIANTS)))
@pytest.mark.parametrize('n', wg.EDGE_SIZES)
def test_tier_a_around_one_row_per_thread_against_fp64(n, v):
    d = wg.relax_edge_case(n, v)
    for flags in (0, rr.CHECK_ONLY) if wg.EDGE_VARIANTS[v][0] == 0 else (0,):      # (check-only needs no dense map; once per size)
        out, seen = _check(d, flags, f'tier A {wg.EDGE_VARIANTS[v][1]}')
        stepped = any(not frozen for _, frozen, _, _ in seen)
        # the work vector: registers up to 1024 atoms, the thread's own rows of `work` above
        assert bool(np.all(out['work'] == np.float32(SENT))) == (not stepped or n <= 1024)


# ---- tier B ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('flags', [0, rr.CHECK_ONLY])
@pytest.mark.parametrize('n', wg.LARGE_SIZES)
def test_tier_b_several_rows_per_thread_against_fp64(n, flags):
    d = wg.relax_large_batch(n)
    out, seen = _check(d, flags, 'tier B')
    if flags == 0:
        assert {(k, f, a) for k, f, a, _ in seen} == {('first', False, None), ('reject_neg', False, False), ('converged', True, None),
                                                      ('converging', True, None)}
        assert {c for k, _, _, c in seen if k == 'first'} == {False, True}           # the clamp taken and not taken


# ---- tier C ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', wg.LARGE_SIZES)
def test_tier_c_full_history_is_no_worse_than_the_wave_form(n):
    d = wg.relax_history_batch(n)
    wave, block = _launch(d, 0, wg_min_atoms=None), _launch(d, 0, wg_min_atoms=0)
    for b in range(len(d['kinds'])):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        ref = wg.plain_step(d['x'][a0:a1], d['F'][a0:a1], d['free'][a0:a1], rr.batch_state(d, b), d['tol2'], d['alpha'], d['maxstep'])
        assert ref['accepted'] is True and ref['n_pairs'] == d['memory'] and ref['clamped'] == bool(d['big'][b])
        e_wave = float(np.abs(wave['pos_out'][a0:a1].astype(np.float64) - ref['x_out']).max())
        e_block = float(np.abs(block['pos_out'][a0:a1].astype(np.float64) - ref['x_out']).max())
        print(f'tier C, {n} atoms, {"clamped" if ref["clamped"] else "free"}: max |x_out - fp64| wave {e_wave:.3e}, workgroup {e_block:.3e} '
              f'(one fp32 ulp of 8: {ULP8:.3e})')
        assert e_block <= max(2.0 * e_wave, ULP8), (e_block, e_wave)
        for k in INTS:                                                         # integers and decisions: the wave form's
            assert int(block[k][b]) == int(wave[k][b]) == [0, ref['n_steps'], ref['n_pairs'], ref['head']][INTS.index(k)], k
        # single correctly rounded operations are the same function of their inputs in both forms
        h0 = int(d['head'][b])
        assert _same_bits(block['Y'][h0, a0:a1], wave['Y'][h0, a0:a1]) and _same_bits(block['f_prev'][a0:a1], wave['f_prev'][a0:a1])
        assert _same_bits(block['S'][ref['head'], a0:a1], rr.stored_s(block['pos_out'][a0:a1], d['x'][a0:a1]).astype(np.float32))
        free = d['free'][a0:a1]
        assert _same_bits(block['pos_out'][a0:a1][~free], d['x'][a0:a1][~free])


# ---- routing and bitwise properties of a launch -----------------------------------------------------------------------------------------

def test_each_molecule_alone_gives_the_bits_it_gave_in_the_batch_and_a_launch_repeats(small):
    d = small
    whole, again = _launch(d), _launch(d)
    for k in OUT:
        assert _same_bits(whole[k], again[k]), f'the same launch twice: {k}'
    for b in range(0, len(d['kinds'])):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        one = _launch(wg.slice_relax(d, b))
        what = f'molecule {b} ({d["kinds"][b]}, {a1 - a0} atoms)'
        assert _same_bits(one['pos_out'], whole['pos_out'][a0:a1]) and _same_bits(one['fmax'], whole['fmax'][b:b + 1]), what
        assert _same_bits(one['S'], whole['S'][:, a0:a1]) and _same_bits(one['Y'], whole['Y'][:, a0:a1]), what
        assert _same_bits(one['rho'], whole['rho'][b:b + 1]) and _same_bits(one['f_prev'], whole['f_prev'][a0:a1]), what
        for k in INTS:
            assert _same_bits(one[k], whole[k][b:b + 1]), f'{what}: {k}'


def test_more_systems_than_workgroups():
    d = wg.relax_many_batch()
    assert len(d['kinds']) > 2048
    _check(d, 0, 'many systems')


def test_the_threshold_routes_each_system_to_one_kernel(small):
    d = small
    wave, block, mixed = _launch(d, wg_min_atoms=None), _launch(d, wg_min_atoms=0), _launch(d, wg_min_atoms=64)
    sizes = np.diff(d['ptr'])
    assert (sizes < 64).any() and (sizes == 64).any() and (sizes > 64).any()
    differ = 0
    for b, n in enumerate(sizes):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        want = wave if n < 64 else block
        for k in ('pos_out', 'f_prev'):
            assert _same_bits(mixed[k][a0:a1], want[k][a0:a1]), (b, n, k)
        for k in ('S', 'Y'):
            assert _same_bits(mixed[k][:, a0:a1], want[k][:, a0:a1]), (b, n, k)
        for k in ('fmax', 'rho') + INTS:
            assert _same_bits(mixed[k][b], want[k][b]), (b, n, k)
        differ += not _same_bits(wave['pos_out'][a0:a1], block['pos_out'][a0:a1])
    assert differ > 0, 'the two forms agree bit for bit everywhere: the routing was not tested'
    # a threshold nothing reaches is the wave entry point; one everything reaches is the workgroup kernel alone
    none, all_ = _launch(d, wg_min_atoms=10 ** 6), _launch(d, wg_min_atoms=1)
    for k in OUT:
        assert _same_bits(none[k], wave[k]), k
    nonempty = np.repeat(sizes > 0, sizes)
    assert _same_bits(all_['pos_out'][nonempty], block['pos_out'][nonempty]) and _same_bits(all_['S'], block['S'])
    # a system whose offsets leave the arrays is marked by exactly one kernel in every mode
    bad = wg.relax_batch([(5, 0, 'first', False, False), (70, 0, 'first', False, False)])
    bad['ptr'] = np.array([0, 80, 75], dtype=np.int32)
    for mode in (None, 0, 64):
        out = _launch(bad, wg_min_atoms=mode)
        assert np.isnan(out['fmax']).all() and bool(np.all(out['pos_out'] == np.float32(SENT))), mode
        assert all(_same_bits(out[k], bad[k]) for k in ('S', 'Y', 'rho', 'f_prev') + INTS), mode


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def test_lbfgs_step_wg_refuses_what_its_twin_refuses(small):
    from newtonnet_amd import hip
    b = next(i for i, (k, n) in enumerate(zip(small['kinds'], np.diff(small['ptr']))) if k == 'accept' and n == 63)
    d = wg.slice_relax(small, b)
    n, m = d['x'].shape[0], d['memory']
    t = _tensors(d)
    keep = {k: v.clone() for k, v in t.items()}
    with pytest.raises(hip.HipLibraryError, match='alias'):
        _call(d, dict(t, pos_out=t['x']))
    flat = torch.zeros(3 * n + 3, device='cuda')
    with pytest.raises(hip.HipLibraryError, match='alias'):          # an overlapping view is an alias too
        _call(d, dict(t, x=flat[:3 * n].view(n, 3), pos_out=flat[3:].view(n, 3)))
    with pytest.raises(hip.HipLibraryError, match='memory'):
        _call(d, dict(t, S=t['S'][:0], Y=t['Y'][:0], rho=t['rho'][:, :0]), memory=0)
    with pytest.raises(hip.HipLibraryError, match='flags'):
        _call(d, t, flags=2)
    for kw, match in ((dict(alpha=0.0), 'alpha'), (dict(maxstep=float('nan')), 'maxstep'), (dict(tol2=-1.0), 'tol2')):
        with pytest.raises(hip.HipLibraryError, match=match):
            _call(d, t, **kw)
    L = hip.lib()
    order = ('x', 'F', 'free', 'ptr', 'converged', 'n_steps', 'n_pairs', 'head', 'S', 'Y', 'rho', 'f_prev', 'work', 'pos_out', 'fmax')

    def raw(t, null=(), n_mol=1, n_atoms=n, wg_min_atoms=0):
        p = {k: (None if k in null else hip._ptr(t[k])) for k in order}
        return L.nnhip_lbfgs_step_wg(p['x'], p['F'], p['free'], p['ptr'], n_mol, n_atoms, m, d['tol2'], d['alpha'], d['maxstep'],
                                     wg_min_atoms, 0, p['converged'], p['n_steps'], p['n_pairs'], p['head'], p['S'], p['Y'], p['rho'],
                                     p['f_prev'], p['work'], p['pos_out'], p['fmax'], hip._stream(t['x'].device))
    for mode in (0, 64):
        for name in order:
            if name in ('free', 'work'):
                continue                                              # optional (work: only needed above 64 atoms)
            assert raw(t, null=(name,), wg_min_atoms=mode) != 0, f'a null {name} was accepted'
            assert b'nnhip_lbfgs_step_wg' in L.nnhip_last_error()
    big = wg.slice_relax(small, next(i for i, n_b in enumerate(np.diff(small['ptr'])) if n_b == 65))
    tb = _tensors(big)
    assert raw(tb, null=('work',), n_atoms=65) != 0, 'no scratch above 64 atoms was accepted'       # (as the twin: work is mandatory)
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(t[k], v), f'{k} was written by a refused call'
    assert bool(torch.all(tb['pos_out'] == SENT)) and bool(torch.all(tb['fmax'] == SENT))
    # empty batches are no-ops that succeed; systems without atoms are converged from the start, by the workgroup kernel too
    assert raw(t, n_mol=0) == 0 and raw(t, null=order, n_mol=0, n_atoms=0) == 0
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(t[k], v), f'{k} was written by an empty launch'
    for mode in (0, 64):
        e3 = torch.zeros(0, 3, device='cuda')
        ints = [torch.zeros(2, dtype=torch.int32, device='cuda') for _ in range(4)]
        fm = torch.full((2,), SENT, device='cuda')
        hip.lbfgs_step(e3, e3.clone(), None, torch.zeros(3, dtype=torch.int32, device='cuda'), m, d['tol2'], d['alpha'], d['maxstep'], 0,
                       *ints, torch.zeros(m, 0, 3, device='cuda'), torch.zeros(m, 0, 3, device='cuda'), torch.zeros(2, m, device='cuda'),
                       e3.clone(), None, e3.clone(), fm, wg_min_atoms=mode)
        assert ints[0].tolist() == [1, 1] and ints[1].tolist() == [0, 0] and fm.tolist() == [0.0, 0.0]


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def workgroup_relaxations(monkeypatch):
    """every model.relaxation(...) of the test is made with form='workgroup' unless it names a form; yields the list of the
    Relaxation objects made, for the test to see that they were"""
    from newtonnet_amd.models.newtonnet import NewtonNet
    made, plain = [], NewtonNet.relaxation

    def relaxation(self, *args, **kw):
        kw.setdefault('form', 'workgroup')
        made.append(plain(self, *args, **kw))
        return made[-1]
    monkeypatch.setattr(NewtonNet, 'relaxation', relaxation)
    yield made
    assert made and all(r.form == 'workgroup' and r._wg_min_atoms == 0 for r in made)


def test_every_recorded_step_of_the_aspirins_follows_from_the_frames_before(workgroup_relaxations):
    """tests/test_hip_relax.py's stepwise check of 40 recorded steps, against the reference with the workgroup's depth"""
    with wg.workgroup_depth():
        base.test_every_recorded_step_follows_from_the_frames_before('aspirin8_ckpt', 'ckpt')


def test_aspirins_converge_like_the_host_fp64_loop(workgroup_relaxations):
    """the existing yardstick: all 8 within 1.5 x the slowest molecule of the host fp64 loop relax_ref.minimise"""
    base.test_aspirins_converge_like_the_host_fp64_loop()


def test_bitwise_properties_of_the_driver(workgroup_relaxations):
    """check_every 0 / 1 / 7, run(a); run(b) against run(a + b), the same run twice, frozen molecules, inputs unmodified"""
    base.test_bitwise_properties()


def _auto_against_both_forms(model, z, pos, cell, batch, thresholds, steps):
    """run `steps` steps under 'wave', 'workgroup' and 'auto' with each threshold: every molecule of an 'auto' run has, bit for bit,
    its result under 'wave' if it is smaller than the threshold and under 'workgroup' otherwise.  Returns the atom counts and how
    many molecules the two forms themselves differ on."""
    def run(**kw):
        rel = model.relaxation(z, pos, cell, batch, **kw)
        return rel, rel.run(steps, check_every=0, record_every=5)
    rel, wave = run(form='wave')
    block = run(form='workgroup')[1]
    ptr = _np(rel._mol_ptr)
    sizes = np.diff(ptr)
    slices = [slice(int(ptr[b]), int(ptr[b + 1])) for b in range(len(sizes))]
    for threshold in thresholds:
        auto = run(form='auto', wg_min_atoms=threshold)[1]
        for b, (n, sl) in enumerate(zip(sizes, slices)):
            want = wave if n < threshold else block
            assert torch.equal(auto.pos[sl], want.pos[sl]) and torch.equal(auto.traj_pos[:, sl], want.traj_pos[:, sl]), (threshold, b)
            for name in ('energy', 'fmax', 'converged', 'n_steps'):
                assert torch.equal(getattr(auto, name)[b], getattr(want, name)[b]), (threshold, b, name)
            assert torch.equal(auto.traj_n_pairs[:, b], want.traj_n_pairs[:, b])
    return sizes, sum(not torch.equal(wave.pos[sl], block.pos[sl]) for sl in slices)


def test_auto_gives_each_molecule_the_bits_of_the_form_it_is_routed_to():
    """mixed_rand (21, 9, 1 and 2 atoms) under form='auto' with wg_min_atoms = 22 (every molecule below it) and 21 (the largest one
    not).  Up to 64 atoms the routing cannot be seen in the bits -- 15 of the workgroup's 16 wave sums are exact zeros, and what is
    left is the wave form's butterfly -- so the boxes of pbc_batch2_rand (216 and 125 atoms, at their fixed cells) follow with a
    threshold between them, where the two forms differ."""
    model, z, pos, cell, batch = base._setup('mixed_rand', 'rand')
    sizes, differ = _auto_against_both_forms(model, z, pos, cell, batch, (22, 21), 25)
    assert sizes.max() == 21 and differ == 0
    model, z, pos, cell, batch = base._setup('pbc_batch2_rand', 'rand')
    sizes, differ = _auto_against_both_forms(model, z, pos, cell, batch, (200,), 10)
    assert sorted(sizes.tolist()) == [125, 216] and differ == 2, (sizes, differ)


def test_calculator_relax_in_the_workgroup_form_equals_the_model_path(monkeypatch):
    from newtonnet_amd import hip
    from newtonnet_amd.utils import MLAseCalculator
    seen, plain = [], hip.lbfgs_step

    def spy(*args, **kw):
        seen.append(kw.get('wg_min_atoms'))
        return plain(*args, **kw)
    monkeypatch.setattr(hip, 'lbfgs_step', spy)
    from tests.test_hip_md import FakeAtoms
    model, z, pos, cell, batch = base._setup('aspirin8_ckpt', 'ckpt')
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda')
    zc, pc = _np(z), _np(pos)
    frames = [FakeAtoms(zc[21 * k:21 * (k + 1)], pc[21 * k:21 * (k + 1)]) for k in range(3)]
    out = calc.relax(frames, fmax=0.05, max_steps=60, form='workgroup')
    assert seen and set(seen) == {0}                                    # every launch went through nnhip_lbfgs_step_wg, all systems
    res = model.relaxation(z[:63], pos[:63], cell[:3], batch[:63], fmax=0.05, form='workgroup').run(60, check_every=10)
    assert np.array_equal(out['positions'].reshape(63, 3), _np(res.pos)) and np.array_equal(out['energy'], _np(res.energy))
    assert np.array_equal(out['fmax'], _np(res.fmax)) and np.array_equal(out['n_steps'], _np(res.n_steps))
    del seen[:]
    auto = calc.relax(frames, fmax=0.05, max_steps=60, form='auto', wg_min_atoms=22)       # 21 atoms each: the wave kernel
    assert set(seen) == {22}
    del seen[:]
    wave = calc.relax(frames, fmax=0.05, max_steps=60)
    assert set(seen) == {None}
    # (up to 64 atoms the two forms agree bit for bit: 15 of the workgroup's 16 wave sums are exact zeros)
    assert all(np.array_equal(auto[k], wave[k]) and np.array_equal(out[k], wave[k]) for k in wave)
    with pytest.raises(ValueError, match='form'):
        calc.relax(frames, form='block')
