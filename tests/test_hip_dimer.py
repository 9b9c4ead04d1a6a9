"""GPU checks of the batched dimer-method saddle search (newtonnet_amd/dimer.py, csrc/dimer.hip): one launch against the fp64
restatement tests/dimer_ref.py on synthetic inputs that reach every branch at every size, bitwise independence of the batch,
refused calls and impossible state, every launch of two real searches against the reference from the device's own state, the
refinement of a band's climbing image (the point of the feature), a single-ended search, the bitwise properties of the driver and
the calculator's interface."""
import math

import numpy as np
import pytest
import torch

from tests import dimer_ref as dr
from tests import neb_ref as nr
from tests import relax_ref as rr
from tests import util
from tests.test_hip_hessian import cuda, make_model

pytestmark = pytest.mark.gpu

SENT = 777.0
STATE = ('istate', 'fstate', 'vstate', 'S', 'Y', 'rho')
INPUTS = ('x', 'F', 'ptr', 'free')
NI, NF, NV = len(dr.INTS), len(dr.FLOATS), len(dr.VECS)


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _slice(d, b):
    """molecule b of a batch (the kernel's layout) as a batch of its own"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    out = dict(d, ptr=np.array([0, a1 - a0], dtype=np.int32), cases=[d['cases'][b]])
    for k in ('x', 'F', 'free'):
        out[k] = d[k][a0:a1]
    for k in ('vstate', 'S', 'Y'):
        out[k] = np.ascontiguousarray(d[k][:, a0:a1])
    for k in ('istate', 'fstate'):
        out[k] = np.ascontiguousarray(d[k][:, b:b + 1])
    out['rho'] = d['rho'][b:b + 1]
    return out


def _reversed(d):
    B = len(d['ptr']) - 1
    parts = [_slice(d, b) for b in range(B - 1, -1, -1)]
    out = dict(d, ptr=np.concatenate([[0], np.cumsum([len(p['x']) for p in parts])]).astype(np.int32), cases=d['cases'][::-1])
    for k in ('x', 'F', 'free', 'rho'):
        out[k] = np.concatenate([p[k] for p in parts])
    for k in ('vstate', 'S', 'Y', 'istate', 'fstate'):
        out[k] = np.ascontiguousarray(np.concatenate([p[k] for p in parts], axis=1))
    return out


def _launch(d, flags=0, use_mask=None, energy=True, **over):
    """one launch on a batch in the kernel's layout; returns the inputs as they are afterwards and the outputs, as numpy arrays"""
    from newtonnet_amd import hip
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in INPUTS + STATE}
    N, B = d['x'].shape[0], len(d['ptr']) - 1
    t.update(pos_out=torch.full((N, 3), SENT, device='cuda'), fmax=torch.full((B,), SENT, device='cuda'),
             e_out=torch.full((B,), SENT, device='cuda'), energy=torch.arange(B, device='cuda', dtype=torch.float32) + 0.5,
             work=torch.full((N, 3), SENT, device='cuda'))
    p = dict(d['par'], memory=d['memory'], **over)
    use_mask = d['masked'] if use_mask is None else use_mask
    hip.dimer_step(t['x'], t['F'], t['energy'] if energy else None, t['free'] if use_mask else None, t['ptr'], p['memory'], p['delta'],
                   p['rot_tol'], p['max_rotations'], p['tol2'], p['alpha'], p['maxstep'], flags, t['istate'], t['fstate'],
                   t['vstate'], t['S'], t['Y'], t['rho'], t['work'], t['pos_out'], t['fmax'], t['e_out'] if energy else None)
    return {k: _np(v) for k, v in t.items()}


def _device_state(out, b, a0, a1):
    st = {name: int(out['istate'][k, b]) for k, name in enumerate(dr.INTS)}
    st.update({name: float(out['fstate'][k, b]) for k, name in enumerate(dr.FLOATS)})
    st.update({name: out['vstate'][k, a0:a1].astype(np.float64) for k, name in enumerate(dr.VECS)})
    st.update(S=out['S'][:, a0:a1].astype(np.float64), Y=out['Y'][:, a0:a1].astype(np.float64), rho=out['rho'][b].astype(np.float64))
    return st


def check_launch(ref_of, st, got, x, xo, fmax, e_out, e_in, free, what, worst):
    """one molecule of one launch against the reference.  ref_of(ft_stored) -> dimer_ref.dimer_step's result; st: the state before,
    got: the device's state after; x, xo: the probe and the next one; free: bool [n].  Returns False when the launch held an
    ambiguous decision (nothing is compared then)."""
    ref = ref_of(None)
    if any(ref['ambiguous'].values()):
        return False
    tr = ref['translate']
    if tr is not None:                                       # the step is taken from the F+ the kernel stored (dimer_ref's head)
        ref = ref_of(got['f_prev'])
        tr = ref['translate']
        if any(ref['ambiguous'].values()):
            return False
    new = ref['state']
    for k in dr.INTS:
        assert got[k] == new[k], f'{what}: {k} {got[k]} != {new[k]} ({ref["path"]})'
    if ref['fmax'] is None:
        assert fmax == SENT and e_out == SENT, f'{what}: fmax_out / energy_out written though the probe is no centre'
    else:
        assert abs(fmax - ref['fmax']) <= ref['b_fmax'] + float(rr.half_ulp32(ref['fmax'])), f'{what}: fmax {fmax} != {ref["fmax"]}'
        assert e_out == e_in, f'{what}: energy_out {e_out} != {e_in}'
    assert _same_bits(xo[~free], got['center'].astype(np.float32)[~free]), f'{what}: a fixed atom moved'
    if ref['frozen']:
        assert _same_bits(xo, x), f'{what}: a frozen molecule moved'
        for k in dr.FLOATS + dr.VECS + ('S', 'Y', 'rho'):
            assert np.array_equal(np.asarray(got[k]), np.asarray(st[k])), f'{what}: {k} touched'
        return True
    top = dr.compare(ref, xo.astype(np.float64), got, worst)
    assert top <= 1.0, f'{what} ({ref["path"]}): err / (bound + half an ulp) = {top:.3f}'
    # what the launch copies or leaves alone is exact: F0 / F1 = the masked force, x_prev = the centre left, every untouched row
    skip = set(ref['bounds']) | ({'center', 'f_prev'} if tr is not None else set())
    for k in dr.FLOATS + dr.VECS:
        if k not in skip:
            assert np.array_equal(np.asarray(got[k]), np.asarray(new[k])), f'{what} ({ref["path"]}): {k} is not the exact value'
    for k in dr.VECS:                                        # a fixed atom's rows keep their bits, in every vector but F0 / F1 (0)
        if k not in ('F0', 'F1', 'f_prev', 'x_prev', 'center'):
            assert np.array_equal(got[k][~free], st[k][~free]), f'{what}: {k} of a fixed atom was written'
    if tr is None:
        for k in ('S', 'Y', 'rho'):
            assert np.array_equal(got[k], st[k]), f'{what}: {k} touched without a translation'
    else:
        m, head = st['S'].shape[0], st['head']
        assert np.array_equal(got['S'][new['head']], rr.stored_s(got['center'], st['center'])), f'{what}: S[head] is not x_out - x'
        if tr['accepted']:
            assert np.array_equal(got['Y'][head], rr.pair_y(st['f_prev'], got['f_prev'])), f'{what}: Y[head] is not f_prev - f'
            assert abs(got['rho'][head] - new['rho'][head]) <= tr['b_rho_new'] + float(rr.half_ulp32(new['rho'][head])), what
        untouched = [k for k in range(m) if k != new['head'] and not (tr['accepted'] and k == head)]
        for k in untouched:
            assert np.array_equal(got['S'][k], st['S'][k]) and np.array_equal(got['Y'][k], st['Y'][k]), f'{what}: slot {k} touched'
            assert got['rho'][k] == st['rho'][k], f'{what}: rho[{k}] touched'
    return True


# ---- 1. the kernel against fp64 on the same inputs ---------------------------------------------------------------------------------

@pytest.mark.parametrize('masked,flags', [(False, 0), (True, 0), (False, dr.CHECK_ONLY), (True, dr.CHECK_ONLY)])
def test_dimer_step_against_fp64_on_the_same_inputs(masked, flags):
    d = dr.synthetic_batch(masked)
    out = _launch(d, flags)
    for k in INPUTS:
        assert _same_bits(out[k], d[k]), f'{k}: an input was written'
    worst, earned, moved = {}, {n: set() for n in dr.SYN_SIZES}, 0
    for b, c in enumerate(d['cases']):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        what = f'mask {masked}, flags {flags}: molecule {b} ({a1 - a0} atoms)'
        if c is None:                                        # an empty molecule: frozen, nothing but fmax_out = 0 and its energy
            assert out['fmax'][b] == 0.0 and out['e_out'][b] == out['energy'][b], what
            assert _same_bits(out['istate'][:, b], d['istate'][:, b]) and _same_bits(out['fstate'][:, b], d['fstate'][:, b]), what
            continue
        st = dr.batch_state(d, b)
        free = d['free'][a0:a1] if masked else np.ones(a1 - a0, dtype=bool)
        ok = check_launch(lambda ft: dr.batch_step(d, b, flags, ft_stored=ft), st, _device_state(out, b, a0, a1), d['x'][a0:a1],
                          out['pos_out'][a0:a1], float(out['fmax'][b]), float(out['e_out'][b]), float(out['energy'][b]), free, what, worst)
        assert ok, f'{what}: an ambiguous decision among the synthetic inputs'
        if not flags:
            ref = dr.batch_step(d, b)
            earned[c['n']] |= dr._labels(ref, st)
            moved += not ref['frozen']
    if flags:
        assert _same_bits(out['vstate'], d['vstate']) and _same_bits(out['istate'], d['istate']) and _same_bits(out['S'], d['S'])
        assert _same_bits(out['pos_out'], d['x'])
    else:
        for n in dr.SYN_SIZES:                               # every branch was run at every size
            assert earned[n] == set(dr.SYN_WANTED), f'size {n}: {sorted(set(dr.SYN_WANTED) - earned[n])} not run'
    print(f'dimer_step mask {masked}, flags {flags}: {len(d["cases"])} molecules, {moved} moved, worst err / (bound + half an ulp) '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f' (C_DM = {dr.C_DM})')


# ---- 2. bitwise: the batch around a molecule, the mask ---------------------------------------------------------------------------------

OUTPUTS = ('pos_out', 'fmax', 'e_out') + STATE


def test_each_molecule_alone_and_the_batch_reversed_give_the_bits_of_the_batch():
    d = dr.synthetic_batch(True)
    whole = _launch(d)
    again = _launch(d)
    for k in OUTPUTS:
        assert _same_bits(whole[k], again[k]), f'{k}: two launches differ'
    B = len(d['ptr']) - 1
    back = _launch(_reversed(d))
    for b in range(B):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        alone = _launch(_slice(d, b))
        r = B - 1 - b
        r0 = int(d['ptr'][-1]) - a1
        for k in ('pos_out',):
            assert _same_bits(alone[k], whole[k][a0:a1]) and _same_bits(back[k][r0:r0 + a1 - a0], whole[k][a0:a1]), (b, k)
        for k in ('vstate', 'S', 'Y'):
            assert _same_bits(alone[k], whole[k][:, a0:a1]) and _same_bits(back[k][:, r0:r0 + a1 - a0], whole[k][:, a0:a1]), (b, k)
        for k in ('istate', 'fstate'):
            assert _same_bits(alone[k][:, 0], whole[k][:, b]) and _same_bits(back[k][:, r], whole[k][:, b]), (b, k)
        assert _same_bits(alone['rho'][0], whole['rho'][b]) and _same_bits(back['rho'][r], whole['rho'][b]), b
        assert _same_bits(alone['fmax'][0], whole['fmax'][b]) and _same_bits(back['fmax'][r], whole['fmax'][b]), b


def test_a_null_mask_means_all_atoms_free():
    d = dr.synthetic_batch(False)
    ones = dict(d, free=np.ones_like(d['free']))
    a, b = _launch(ones, use_mask=True), _launch(d, use_mask=False)
    for k in OUTPUTS:
        assert _same_bits(a[k], b[k]), k
    c = _launch(d, energy=False)                             # and without energies nothing else changes
    for k in OUTPUTS:
        assert _same_bits(c[k], b[k]) or k == 'e_out', k


# ---- 3. refused calls and impossible state -----------------------------------------------------------------------------------------------

def _small():
    d = dr.synthetic_batch(True)
    b = next(b for b, c in enumerate(d['cases']) if c is not None and c['n'] == 21 and c['path'].startswith('p2') and c['path'].endswith('trial'))
    return _slice(d, b)


def test_dimer_step_refuses_bad_arguments_and_writes_nothing():
    from newtonnet_amd import hip
    from newtonnet_amd.abi import HipLibraryError
    d = _small()
    good = _launch(d)
    assert (good['pos_out'] != SENT).all()
    nan = float('nan')
    for over in (dict(memory=0), dict(memory=hip.LBFGS_MAX_MEMORY + 1), dict(delta=0.0), dict(delta=-0.01), dict(delta=nan),
                 dict(rot_tol=0.0), dict(rot_tol=nan), dict(alpha=0.0), dict(alpha=nan), dict(maxstep=-0.2), dict(maxstep=nan),
                 dict(tol2=-1e-6), dict(tol2=nan), dict(max_rotations=-1)):
        t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in INPUTS + STATE}
        keep = {k: v.clone() for k, v in t.items()}
        pos_out, fmax = torch.full((21, 3), SENT, device='cuda'), torch.full((1,), SENT, device='cuda')
        p = dict(d['par'], memory=d['memory'])
        p.update(over)
        S, Y = (torch.zeros(p['memory'], 21, 3, device='cuda') for _ in range(2))
        rho = torch.zeros(1, p['memory'], device='cuda')
        with pytest.raises(HipLibraryError, match='nnhip_dimer_step'):
            hip.dimer_step(t['x'], t['F'], None, t['free'], t['ptr'], p['memory'], p['delta'], p['rot_tol'], p['max_rotations'],
                           p['tol2'], p['alpha'], p['maxstep'], 0, t['istate'], t['fstate'], t['vstate'], S, Y, rho, None, pos_out, fmax)
        assert (pos_out == SENT).all() and (fmax == SENT).all(), over
        for k in ('istate', 'fstate', 'vstate'):
            assert _same_bits(_np(t[k]), _np(keep[k])), (over, k)

    def call(t, flags=0, pos_out=None, **kw):
        p = dict(d['par'])
        a = dict(t, **kw)
        hip.dimer_step(a['x'], a['F'], None, a['free'], a['ptr'], d['memory'], p['delta'], p['rot_tol'], p['max_rotations'], p['tol2'],
                       p['alpha'], p['maxstep'], flags, a['istate'], a['fstate'], a['vstate'], a['S'], a['Y'], a['rho'], None,
                       a['x'] if pos_out is None else pos_out, torch.full((1,), SENT, device='cuda'))
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in INPUTS + STATE}
    keep = {k: v.clone() for k, v in t.items()}
    with pytest.raises(HipLibraryError, match='alias'):      # pos_out overlapping pos_in
        call(t)
    with pytest.raises(HipLibraryError, match='flags'):      # an unknown flag
        call(t, flags=2, pos_out=torch.empty(21, 3, device='cuda'))
    for k, v in keep.items():
        assert _same_bits(_np(t[k]), _np(v)), k                # (bits: the force rows of fixed atoms hold NaN)
    # the wrapper's own checks (shared with the other wrappers): types, sizes, contiguity
    out = torch.empty(21, 3, device='cuda')
    with pytest.raises(ValueError):
        call(t, pos_out=out, istate=t['istate'].long())
    with pytest.raises(ValueError):
        call(t, pos_out=out, vstate=t['vstate'][:-1])
    with pytest.raises(ValueError):
        call(t, pos_out=out, free=t['free'][:-1])
    with pytest.raises(ValueError):
        call(t, pos_out=torch.empty(21, 3, device='cuda', dtype=torch.float64))
    # an empty batch succeeds without a launch
    e = torch.zeros(0, device='cuda')
    hip.dimer_step(e.reshape(0, 3), e.reshape(0, 3), None, None, torch.zeros(1, dtype=torch.int32, device='cuda'), 4, 0.01, 0.17, 3,
                   1e-4, 70.0, 0.2, 0, torch.zeros(NI, 0, dtype=torch.int32, device='cuda'), e.reshape(NF, 0), e.reshape(NV, 0, 3),
                   e.reshape(4, 0, 3), e.reshape(4, 0, 3), e.reshape(0, 4), None, e.reshape(0, 3), e)


def test_a_molecule_with_impossible_state_is_left_alone_and_gets_nan():
    d = _small()
    I, F = {n: k for k, n in enumerate(dr.INTS)}, {n: k for k, n in enumerate(dr.FLOATS)}
    bad_ints = [('phase', 3), ('phase', -1), ('status', 2), ('head', d['memory']), ('head', -1), ('n_pairs', d['memory'] + 1),
                ('n_steps', -1), ('n_evals', -2), ('n_rot', -1), ('n_evals', 0), ('pending', 2), ('pending', -1)]
    for name, v in bad_ints:
        e = dict(d, istate=d['istate'].copy())
        e['istate'][I[name], 0] = v
        out = _launch(e)
        assert np.isnan(out['fmax'][0]) and np.all(out['pos_out'] == SENT), (name, v)
        for k in STATE:
            assert _same_bits(out[k], e[k]), (name, v, k)
    for v in (np.nan, np.inf):                               # a curvature that is not finite in a trial launch
        e = dict(d, fstate=d['fstate'].copy())
        e['fstate'][F['curvature'], 0] = v
        out = _launch(e)
        assert np.isnan(out['fmax'][0]) and np.all(out['pos_out'] == SENT), v
        for k in STATE:
            assert _same_bits(out[k], e[k]), (v, k)
    for ptr in ([0, 22], [-1, 21], [5, 3]):                  # atom offsets outside the arrays
        e = dict(d, ptr=np.array(ptr, dtype=np.int32))
        from newtonnet_amd import hip
        t = {k: torch.from_numpy(np.ascontiguousarray(e[k])).cuda() for k in INPUTS + STATE}
        pos_out, fmax = torch.full((21, 3), SENT, device='cuda'), torch.full((1,), SENT, device='cuda')
        p = d['par']
        hip.dimer_step(t['x'], t['F'], None, t['free'], t['ptr'], d['memory'], p['delta'], p['rot_tol'], p['max_rotations'], p['tol2'],
                       p['alpha'], p['maxstep'], 0, t['istate'], t['fstate'], t['vstate'], t['S'], t['Y'], t['rho'], None, pos_out, fmax)
        assert bool(torch.isnan(fmax).all()) and bool((pos_out == SENT).all()), ptr
        for k in STATE:
            assert _same_bits(_np(t[k]), e[k]), (ptr, k)


# ---- 4. the driver ---------------------------------------------------------------------------------------------------------------------------

def _setup(case, weights):
    z, pos, cell, batch, _ = util.case_inputs(case, torch.float32)
    z, pos, cell, batch = cuda(z, pos, cell, batch)
    return make_model(util.load_state(weights)), z, pos, cell, batch


@pytest.fixture(scope='module')
def band_top():
    """the shipped model and the climbing image of aspirin's methyl rotation as a band LEAVES it: aspirin8_ckpt molecule 0 relaxed
    on the device, then the 7-image band of tests/test_hip_neb.py (spring 0.1 eV/A^2, climbing below 0.05 eV/A) stopped at the
    band's usual fmax = 0.01 eV/A -- not tightened"""
    model, z, pos, cell, batch = _setup('aspirin8_ckpt', 'ckpt')
    z1, c1, b1 = z[:21].contiguous(), cell[:1].contiguous(), batch[:21].contiguous()
    res = model.relaxation(z1, pos[:21], c1, b1).run(600, check_every=10)
    assert bool(res.converged.all())
    A = _np(res.pos).astype(np.float64)
    zA = _np(z1)
    x0 = nr.methyl_rotation_band(zA, A, 7).astype(np.float32)
    bb = torch.arange(7, device='cuda').repeat_interleave(21)
    band = model.band(z1.repeat(7), torch.from_numpy(x0.reshape(-1, 3)).cuda(), torch.zeros(7, 3, 3, device='cuda'), bb, 7, spring=0.1,
                      fmax=0.01, climb_below=0.05)
    out = band.run(1000, check_every=10)
    assert bool(out.converged[0])
    top = int(out.saddle_image[0])
    S = out.pos[21 * top:21 * (top + 1)].clone()
    tangent = out.tangent[21 * top:21 * (top + 1)].clone()
    f_top = float(model(z1, S.clone(), c1, b1).gradient_force.norm(dim=1).max())
    print(f'band stopped at 0.01 eV/A after {int(out.n_steps[0])} steps ({7 * int(out.n_steps[0])} force evaluations), true |f| on the '
          f'climbing image {f_top:.2e} eV/A')
    return dict(model=model, z=z1, cell=c1, batch=b1, zA=zA, A=A, pos=S, tangent=tangent, f_top=f_top, all=(z, pos, cell, batch),
                band_steps=int(out.n_steps[0]))


@pytest.fixture(scope='module')
def refined(band_top):
    """saddle_search from the climbing image along its tangent, fmax = 0.0005, and dimer_ref.search on the same model() forces"""
    model, z1, c1, b1 = band_top['model'], band_top['z'], band_top['cell'], band_top['batch']

    def energy_forces(x):
        out = model(z1, torch.from_numpy(x).float().cuda(), c1, b1)
        return _np(out.energy).astype(np.float64), _np(out.gradient_force).astype(np.float64)
    host = dr.search(energy_forces, _np(band_top['pos']).astype(np.float64), _np(band_top['tangent']).astype(np.float64), fmax=0.0005,
                     max_evaluations=1500)
    limit = int(math.floor(1.5 * host['n_evaluations']))
    search = model.saddle_search(z1, band_top['pos'], c1, b1, direction=band_top['tangent'], fmax=0.0005)
    res = search.run(limit, check_every=10)
    print(f'refinement: device {int(res.n_evaluations[0])} evaluations ({int(res.n_steps[0])} translations, {int(res.n_rotations[0])} '
          f'rotations), converged {bool(res.converged[0])}, fmax {float(res.fmax[0]):.2e}, curvature {float(res.curvature[0]):.4f}; host '
          f'fp64 loop on model() forces {host["n_evaluations"]} evaluations ({host["n_steps"]} translations, {host["n_rotations"]} '
          f'rotations), converged {host["converged"]}, curvature {host["curvature"]:.4f} (limit {limit})')
    return dict(res=res, host=host, limit=limit)


def _start_state(search):
    """the reference state of every molecule of a SaddleSearch before its first launch"""
    ptr = _np(search._mol_ptr)
    out = dict(ptr=ptr, masked=search._free is not None, memory=search.memory,
               par=dict(tol2=search._tol2, delta=search._delta, rot_tol=search._rot_tol, max_rotations=search.max_rotations,
                        maxstep=search._maxstep, alpha=search._alpha))
    return out


def _snapshot(search):
    d = dict(istate=_np(search._istate).copy(), fstate=_np(search._fstate).copy(), vstate=_np(search._vstate).copy(),
             S=_np(search._S).copy(), Y=_np(search._Y).copy(), rho=_np(search._rho).copy())
    return d


@pytest.mark.parametrize('case', ['aspirin', 'mixed_rand'])
def test_every_evaluation_follows_from_the_state_before(case, band_top):
    """60 evaluations, one run(1, record_every=1) each (run(a); run(b) leaves the bits of run(a + b): the driver test): before
    every launch the device's own state is read, and the launch must land within the bound of dimer_ref.dimer_step from exactly
    that state, the recorded probe and the recorded force -- integers and phases exactly.  The recorded forces and energies are
    model(recorded probe) bit for bit.  A molecule-step with an ambiguous decision is skipped and counted; more than 5 % fail."""
    model = band_top['model']
    if case == 'aspirin':
        z, cell, batch, pos, direction = band_top['z'], band_top['cell'], band_top['batch'], band_top['pos'], band_top['tangent']
    else:
        _, z, pos, cell, batch = _setup('mixed_rand', 'ckpt')
        direction = torch.randn(pos.shape, generator=torch.Generator().manual_seed(5)).cuda()
    search = model.saddle_search(z, pos, cell, batch, direction=direction, fmax=0.0005)
    info = _start_state(search)
    ptr, B = info['ptr'], len(info['ptr']) - 1
    first = model(z, pos, cell, batch)
    probe, force, energy = _np(pos), _np(first.gradient_force), _np(first.energy).reshape(-1)
    worst, steps, ambiguous, paths = {}, 0, 0, {}
    for k in range(60):
        before = _snapshot(search)
        res = search.run(1, 0, record_every=1)
        assert res.traj_step.tolist() == [k + 1]
        after = _snapshot(search)
        xo = _np(res.traj_pos[0])
        out = model(z, res.traj_pos[0].clone(), cell, batch)
        assert torch.equal(out.gradient_force, res.traj_force[0]) and torch.equal(out.energy.reshape(-1), res.traj_energy[0]), k
        assert torch.equal(res.traj_center[0], search.positions) and torch.equal(res.traj_mode[0], search.mode)
        for b in range(B):
            a0, a1 = int(ptr[b]), int(ptr[b + 1])
            d = dict(before, ptr=ptr)
            st, got = dr.batch_state(d, b), _device_state(after, b, a0, a1)
            assert int(res.traj_phase[0, b]) == got['phase'] and float(res.traj_curvature[0, b]) == np.float32(got['curvature'])
            free = np.ones(a1 - a0, dtype=bool)
            fm = SENT if st['phase'] != 0 else float(res.fmax[b])
            eo = SENT if st['phase'] != 0 else float(energy[b])
            ok = check_launch(lambda ft: dr.dimer_step(probe[a0:a1], force[a0:a1], None, st, info['par'], ft_stored=ft), st, got,
                              probe[a0:a1], xo[a0:a1], fm, eo, float(energy[b]), free, f'{case}: evaluation {k + 1}, molecule {b}', worst)
            steps += 1
            ambiguous += not ok
            path = dr.dimer_step(probe[a0:a1], force[a0:a1], None, st, info['par'], eps=0.0)['path'].split(':')[0]
            paths[path] = paths.get(path, 0) + 1
        probe, force, energy = xo, _np(res.traj_force[0]), _np(res.traj_energy[0])
    print(f'{case}: {steps} molecule-steps, {ambiguous} ambiguous; launches by kind {paths}; worst err / (bound + half an ulp) '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert ambiguous <= 0.05 * steps


# ---- 5. refinement: the point of the feature ------------------------------------------------------------------------------------------------

def test_refinement_of_a_band_image_reaches_a_saddle_a_reaction_path_can_leave(band_top, refined):
    """Methyl rotation of aspirin (110i cm^-1), shipped weights.  A band stopped at its usual 0.01 eV/A leaves a climbing image from
    which one IRC branch starts uphill; the IRC tests tighten the band to 0.0005 eV/A over thousands of band
    steps of 7 force evaluations each.  Here the dimer starts from the image the band left, along its tangent, with fmax = 0.0005.
    The yardstick of the evaluation count is dimer_ref.search (fp64 positions and arithmetic) on the same model() forces from the
    same start: the device must converge within 1.5 x its evaluations (the margin DESIGN section 12 uses for the same kind of
    comparison).  On the CPU oracle the prototype took 386 evaluations (fp64) from a band image with a true force of 0.0043 eV/A."""
    model, z1, c1, b1 = band_top['model'], band_top['z'], band_top['cell'], band_top['batch']
    res, host = refined['res'], refined['host']
    assert host['converged'], f'the host loop did not converge in {host["n_evaluations"]} evaluations'
    assert bool(res.converged[0]), f'not converged within {refined["limit"]} evaluations (host {host["n_evaluations"]})'
    assert int(res.n_evaluations[0]) <= 1.5 * host['n_evaluations']
    out = model(z1, res.pos.clone(), c1, b1)
    f_true = float(out.gradient_force.norm(dim=1).max())
    from newtonnet_amd.vibrations import table_masses
    nm = model.normal_modes(z1, res.pos, c1, b1)
    freq = _np(model.frequencies(z1, res.pos, c1, b1))
    n_imaginary = int(nm.n_imaginary[0])
    m = _np(table_masses(z1)).astype(np.float64)
    o = int(nm.blk_ptr[0])
    low = _np(nm.modes.reshape(-1)[o:o + 63]).astype(np.float64).reshape(21, 3) / np.sqrt(m)[:, None]     # un-mass-weighted, as
    low /= np.linalg.norm(low)                                                                           # reaction_path does
    overlap = abs(float((low * _np(res.mode).astype(np.float64)).sum()))
    t_overlap = abs(float((low * _np(band_top['tangent']).astype(np.float64)).sum()) / float(band_top['tangent'].norm()))
    print(f'true fmax at the result {f_true:.2e} eV/A (band image: {band_top["f_top"]:.2e}), curvature {float(res.curvature[0]):.4f} '
          f'eV/A^2, imaginary modes {n_imaginary} (lowest {freq[:2].round(1).tolist()} cm^-1), |mode . lowest normal mode| '
          f'{overlap:.4f} (band tangent: {t_overlap:.4f}), centre moved {float((res.pos - band_top["pos"]).detach().norm(dim=1).max()):.4f} A')
    assert f_true < 0.0005
    assert float(res.curvature[0]) < 0
    assert int(nm.n_imaginary[0]) == 1
    assert overlap > 0.9
    # the reaction path leaves this saddle downhill on both sides
    sign = 1.0
    path = model.reaction_path(z1, res.pos, c1, b1, direction=res.mode * sign, initial_displacement=0.05)
    r = path.run(40, check_every=5, record_every=1)
    e_s = float(out.energy.reshape(-1)[0])
    n = r.n_steps.tolist()
    E = _np(r.traj_energy).astype(np.float64)
    print(f'reaction path from the refined saddle: steps {n}, status {r.status.tolist()}, saddle - end '
          f'{(e_s - _np(r.energy).astype(np.float64)).round(5).tolist()} eV')
    for p in range(2):
        assert n[p] > 10, f'branch {p} stopped after {n[p]} steps'
        assert float(np.diff(np.concatenate([[e_s], E[:n[p], p]])).max()) <= 2.0 * float(util.energy_tol(e_s)), f'branch {p} rises'
        assert float(r.energy[p]) < e_s, f'branch {p} ends above the saddle'


# ---- 6. single-ended search -----------------------------------------------------------------------------------------------------------------

def test_single_ended_search_finds_the_saddle_again_from_a_random_direction_and_its_negative(band_top, refined):
    """From the refined saddle displaced by 0.05 A along a seeded random unit vector, with a seeded random direction d and with -d
    (one batch of two molecules), fmax = 0.0005: both searches must find the saddle again to 0.01 A (largest atomic distance) and
    the same mode up to sign.  The start lies in a convex region of the dimer (its curvature along a random direction is positive
    for the first cycles), which is what the history rule of the translation is for: while C >= 0 the step is
    the plain F+ / alpha and no curvature pair is kept.  With pairs kept through that phase, as nnhip_lbfgs_step's recursion would
    by itself, d converged 1.12 A away at another stationary point (curvature -58.9 eV/A^2) after three steps at the maxstep cap.
    Measured on one MI355X: 729 and 743 evaluations (73 and 76 translations, 582 and 590 rotations), 0.0079 and 0.0079 A from the
    refined saddle, mode overlaps 0.981 and -0.983, curvatures -0.0651 and -0.0662 eV/A^2.  A converged centre is defined to about
    fmax / |curvature| = 0.0076 A along this soft mode."""
    model, z1, c1, b1 = band_top['model'], band_top['z'], band_top['cell'], band_top['batch']
    res = refined['res']
    assert bool(res.converged[0])
    g = torch.Generator().manual_seed(11)
    u = torch.randn(21, 3, generator=g)
    start = res.pos + (0.05 * u / u.norm()).cuda()
    d = torch.randn(21, 3, generator=g).cuda()
    z2, c2, b2 = z1.repeat(2), c1.repeat(2, 1, 1), torch.arange(2, device='cuda').repeat_interleave(21).to(b1.dtype)
    search = model.saddle_search(z2, start.repeat(2, 1), c2, b2, direction=torch.cat([d, -d]), fmax=0.0005)
    r = search.run(3000, check_every=10)
    dist = (r.pos.reshape(2, 21, 3) - res.pos[None]).norm(dim=2).max(dim=1).values
    ov = (r.mode.reshape(2, 63) * res.mode.reshape(1, 63)).sum(1)
    print(f'single-ended: evaluations {r.n_evaluations.tolist()}, translations {r.n_steps.tolist()}, rotations {r.n_rotations.tolist()}, '
          f'converged {r.converged.tolist()}, fmax {_np(r.fmax).tolist()}, curvature {_np(r.curvature).tolist()}, largest atomic '
          f'distance to the refined saddle {_np(dist).tolist()} A, mode overlaps {_np(ov).tolist()}')
    assert bool(r.converged.all())
    assert float(dist.max()) < 0.01
    assert float(ov.abs().min()) > 0.9
    assert float((r.pos[:21] - r.pos[21:]).norm(dim=1).max()) < 0.01
    assert abs(float((r.mode[:21] * r.mode[21:]).sum())) > 0.9


# ---- 7. bitwise properties of the driver ----------------------------------------------------------------------------------------------------

RESULT = ('pos', 'mode', 'energy', 'fmax', 'curvature', 'converged', 'n_steps', 'n_evaluations', 'n_rotations')


def test_bitwise_properties_of_the_driver(band_top, refined):
    model = band_top['model']
    z, pos, cell, batch = band_top['all']
    direction = torch.randn(pos.shape, generator=torch.Generator().manual_seed(2)).cuda()
    keep = [t.clone() for t in (z, pos, cell, batch, direction)]

    def make(**kw):
        return model.saddle_search(z, pos, cell, batch, direction=direction, **kw)
    a = make().run(40, 0, record_every=1)
    assert a.traj_step.tolist() == list(range(1, 41)) and a.n_evaluations.tolist() == [40] * 8
    b = make().run(40, 0, record_every=1)
    for name in RESULT + ('traj_pos', 'traj_force', 'traj_center', 'traj_mode', 'traj_phase', 'traj_curvature'):
        assert torch.equal(getattr(a, name), getattr(b, name)), f'the same run twice: {name}'
    # run(13); run(27) leaves the bits of run(40); record_every and check_every change no bit
    s = make()
    first = s.run(13, 0, record_every=0)
    assert s.step_count == 13 and first.traj_pos is None and first.n_evaluations.tolist() == [13] * 8
    second = s.run(27, 10, record_every=7)
    assert second.traj_step.tolist() == [20, 27, 34, 40]
    for name in RESULT:
        assert torch.equal(getattr(a, name), getattr(second, name)), name
    assert torch.equal(second.traj_pos, a.traj_pos[[19, 26, 33, 39]]) and torch.equal(second.traj_mode, a.traj_mode[[19, 26, 33, 39]])
    assert torch.equal(first.pos, a.traj_center[12])
    for record, check in ((0, 0), (7, 1), (0, 7)):
        c = make().run(40, check, record_every=record)
        for name in RESULT:
            assert torch.equal(getattr(a, name), getattr(c, name)), f'record_every {record}, check_every {check}: {name}'
    # a batch of 8 against each molecule alone
    for k in range(8):
        sl = slice(21 * k, 21 * (k + 1))
        one = model.saddle_search(z[sl].contiguous(), pos[sl].contiguous(), cell[k:k + 1].contiguous(),
                                  torch.zeros(21, dtype=batch.dtype, device='cuda'), direction=direction[sl].contiguous()).run(40, 0)
        assert torch.equal(one.pos, a.pos[sl]) and torch.equal(one.mode, a.mode[sl]) and torch.equal(one.energy, a.energy[k:k + 1]), k
        assert torch.equal(one.curvature, a.curvature[k:k + 1]) and torch.equal(one.n_steps, a.n_steps[k:k + 1]), k
    # fixed atoms never move, the others do
    fixed = torch.zeros(pos.shape[0], dtype=torch.bool, device='cuda')
    fixed[::5] = True
    h = make(fixed=fixed).run(40, 0, record_every=1)
    assert torch.equal(h.traj_pos[:, fixed], pos[fixed].expand(40, -1, -1)) and (h.pos[~fixed] != pos[~fixed]).any()
    assert bool((h.mode[fixed] == 0).all())
    # a converged molecule keeps every bit: from the refined saddle along its mode the search converges after its first translation
    res = refined['res']
    assert bool(res.converged[0])
    z1, c1, b1 = band_top['z'], band_top['cell'], band_top['batch']
    f = model.saddle_search(z1, res.pos, c1, b1, direction=res.mode, fmax=0.001).run(30, 0, record_every=1)
    n = int(f.n_evaluations[0])
    assert bool(f.converged[0]) and n < 30, (f.converged.tolist(), n)
    for name in ('traj_pos', 'traj_center', 'traj_mode', 'traj_curvature', 'traj_phase', 'traj_force', 'traj_energy'):
        t = getattr(f, name)
        assert torch.equal(t[n - 1:], t[n - 1].expand_as(t[n - 1:])), f'{name} changed after convergence at evaluation {n}'
    # the caller's tensors are never modified
    for t, k in zip((z, pos, cell, batch, direction), keep):
        assert torch.equal(t, k)
    # what only the device knows is refused at construction
    with pytest.raises(ValueError, match='vanishes'):
        model.saddle_search(z1, res.pos, c1, b1, direction=torch.zeros(21, 3, device='cuda'))
    with pytest.raises(ValueError, match='is on'):
        model.saddle_search(z1, res.pos, c1, b1, direction=torch.ones(21, 3))


def test_direction_none_takes_the_lowest_normal_mode(band_top, refined):
    model, z1, c1, b1 = band_top['model'], band_top['z'], band_top['cell'], band_top['batch']
    res = refined['res']
    s = model.saddle_search(z1, res.pos, c1, b1)
    assert abs(float((s.mode * res.mode).sum())) > 0.9 and abs(float(s.mode.norm()) - 1.0) < 1e-5
    # a minimum has no imaginary mode: None is served all the same
    A = torch.from_numpy(band_top['A']).float().cuda()
    s = model.saddle_search(z1, A, c1, b1)
    assert abs(float(s.mode.norm()) - 1.0) < 1e-5


# ---- 8. the calculator -----------------------------------------------------------------------------------------------------------------------

def test_calculator_find_saddle_equals_the_model_path(band_top):
    from newtonnet_amd.utils import MLAseCalculator
    from tests.test_hip_md import FakeAtoms
    model, zA = band_top['model'], band_top['zA']
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda')
    S, T = _np(band_top['pos']), _np(band_top['tangent'])
    other = S + np.array([0.5, -0.3, 0.2], dtype=np.float32)
    frames = [FakeAtoms(zA, S), FakeAtoms(zA, other)]
    keep = [f.positions.copy() for f in frames]
    out = calc.find_saddle(frames, direction=np.stack([T, T]), fmax=0.0005, max_evaluations=50)
    assert all(np.array_equal(f.positions, k) for f, k in zip(frames, keep))
    z = torch.from_numpy(np.tile(zA, 2)).long().cuda()
    pos = torch.from_numpy(np.concatenate([S, other])).cuda()
    batch = torch.arange(2, device='cuda').repeat_interleave(21)
    res = model.saddle_search(z, pos, torch.zeros(2, 3, 3, device='cuda'), batch, direction=torch.from_numpy(np.concatenate([T, T])).cuda(),
                              fmax=0.0005).run(50, check_every=10)
    assert out['positions'].shape == (2, 21, 3) and np.array_equal(out['positions'], _np(res.pos).reshape(2, 21, 3))
    assert np.array_equal(out['mode'], _np(res.mode).reshape(2, 21, 3))
    for k, name in (('energy', 'energy'), ('fmax', 'fmax'), ('curvature', 'curvature'), ('converged', 'converged'),
                    ('n_steps', 'n_steps'), ('n_evaluations', 'n_evaluations'), ('n_rotations', 'n_rotations')):
        assert out[k].shape == (2,) and np.array_equal(out[k], _np(getattr(res, name))), k
    one = calc.find_saddle(frames[0], direction=T, fmax=0.0005, max_evaluations=50)
    assert one['positions'].shape == (21, 3) and one['energy'].shape == ()
