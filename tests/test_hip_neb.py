"""Batched nudged elastic band on the HIP path (newtonnet_amd/neb.py, csrc/neb.hip).

Kernel alone: nnhip_neb_step on synthetic bands that reach every branch (tests/neb_ref.synthetic_bands; tests/test_neb_host.py
shows on the CPU that none of their decisions is ambiguous) against its fp64 restatement on the SAME fp32 inputs, every output
within the derived first-order bound (C_NEB = 2) plus half an fp32 ulp of the stored value, integers and flags exact, everything a
launch must not touch bitwise untouched under sentinel-filled outputs; the tests print err / bound.  Driver: every recorded step
is checked ONE step at a time from the recorded frames, and convergence is measured against a host fp64 loop of the same
reference driven by model() forces."""
import math

import numpy as np
import pytest
import torch

from tests import neb_ref as nr
from tests import util
from tests.test_hip_hessian import cuda, make_model

pytestmark = pytest.mark.gpu

SENT = 777.0
INTS = ('converged', 'climbing', 'n_steps', 'n_pos')
STATE = INTS + ('dt', 'a', 'vel')
OUT = ('pos_out', 'neb_force', 'tangent', 'fmax', 'saddle')
FLAG_SETS = (0, nr.CLIMB, nr.CLIMB | nr.CHECK_ONLY)
PRM = nr.params(nr.SYN_SPRING, nr.SYN_FMAX, nr.SYN_CLIMB_BELOW)


def _np(t):
    return t.detach().cpu().numpy()


def _fire(prm):
    return tuple(prm[k] for k in ('dt', 'dt_max', 'n_min', 'f_inc', 'f_dec', 'a_start', 'f_a', 'maxstep'))


@pytest.fixture(scope='module')
def syn():
    return nr.synthetic_bands()


def _tensors(d):
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ('x', 'F', 'E', 'free', 'ptr', 'band_ptr', 'vel', 'dt', 'a') + INTS}
    N, K = d['x'].shape[0], len(d['band_ptr']) - 1
    t['band_ptr_host'] = torch.from_numpy(np.ascontiguousarray(d['band_ptr']))
    t.update(pos_out=torch.full((N, 3), SENT, device='cuda'), neb_force=torch.full((N, 3), SENT, device='cuda'),
             tangent=torch.full((N, 3), SENT, device='cuda'), fmax=torch.full((K,), SENT, device='cuda'),
             saddle=torch.full((K,), -7, dtype=torch.int32, device='cuda'))
    return t


def _call(t, flags=0, prm=PRM, use_mask=True, **over):
    from newtonnet_amd import hip
    p = dict(prm, **over)
    hip.neb_step(t['x'], t['F'], t['E'], t['free'] if use_mask else None, t['ptr'], t['band_ptr'], t['band_ptr_host'], p['spring'],
                 p['tol2'], p['climb2'], _fire(p), flags, t['converged'], t['climbing'], t['n_steps'], t['n_pos'], t['dt'], t['a'],
                 t['vel'], t['pos_out'], t['neb_force'], t['tangent'], t['fmax'], t['saddle'])


def _launch(bands, flags=0, use_mask=True):
    """one launch on a list of bands; returns the inputs as they are afterwards and the outputs, as numpy arrays"""
    d = nr.flatten(bands)
    t = _tensors(d)
    _call(t, flags, use_mask=use_mask)
    out = {k: _np(v) for k, v in t.items()}
    out['flat'] = d
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rows(d, k):
    """atom rows and molecule rows of band k of a flattened batch"""
    m0, m1 = int(d['band_ptr'][k]), int(d['band_ptr'][k + 1])
    return slice(int(d['ptr'][m0]), int(d['ptr'][m1])), slice(m0, m1)


# ---- 1. the kernel against fp64 on the same inputs ---------------------------------------------------------------------------------

@pytest.mark.parametrize('flags', FLAG_SETS)
def test_neb_step_against_fp64_on_the_same_inputs(syn, flags):
    out = _launch(syn, flags)
    d = out['flat']
    for k in ('x', 'F', 'E', 'ptr', 'band_ptr'):
        assert _same_bits(out[k], d[k]), f'input {k} was modified'
    worst = dict(x=0.0, F=0.0, t=0.0, v=0.0, fmax=0.0, dt=0.0, a=0.0)
    seen = set()

    def within(key, val, ref, bound, what):
        err, lim = np.abs(np.asarray(val, dtype=np.float64) - ref), bound + nr.half_ulp32(ref)
        ratio = float(np.max(err / lim)) if np.size(err) else 0.0
        assert ratio <= 1.0, f'{what}: {key} err / bound {ratio:.3f}'
        worst[key] = max(worst[key], ratio)
    for k, b in enumerate(syn):
        rows, mols = _rows(d, k)
        what = f'band {k} ({b["kind"]}, {b["n_img"]} images of {b["n"]} atoms, {b["profile"]}, flags {flags})'
        if b['kind'] == 'unequal':
            assert math.isnan(float(out['fmax'][k])), f'{what}: fmax_out is not NaN'
            for name in ('pos_out', 'neb_force', 'tangent'):
                assert np.all(out[name][rows] == SENT), f'{what}: {name} written'
            assert out['saddle'][k] == -7 and all(out[n][k] == d[n][k] for n in INTS + ('dt', 'a')) and _same_bits(out['vel'][rows], d['vel'][rows])
            continue
        shape = b['x'].shape
        ref = nr.band_step(b, flags)
        new = ref['state']
        seen.add((b['kind'], ref['frozen'], ref['fire'], ref['clamped'], new['converged'], new['climbing']))
        seen.add((b['kind'], ref['fire'], ref['clamped']))
        for name in INTS:
            assert int(out[name][k]) == int(new[name]), f'{what}: {name} {out[name][k]} != {int(new[name])}'
        assert int(out['saddle'][k]) == mols.start + ref['saddle'], f'{what}: saddle image'
        within('fmax', out['fmax'][k], ref['fmax'], ref['b_fmax'], what)
        within('F', out['neb_force'][rows].reshape(shape), ref['neb_force'], ref['b_neb_force'], what)
        within('t', out['tangent'][rows].reshape(shape), ref['tangent'], ref['b_tangent'], what)
        xo, x = out['pos_out'][rows].reshape(shape), b['x']
        vo, v = out['vel'][rows].reshape(shape), b['vel']
        held = ~np.broadcast_to(b['free'][:, :, None], shape).copy()
        held[0], held[-1] = True, True
        for name in ('neb_force', 'tangent'):
            assert not out[name][rows].reshape(shape)[0].any() and not out[name][rows].reshape(shape)[-1].any(), f'{what}: endpoint {name}'
            assert not out[name][rows].reshape(shape)[~np.broadcast_to(b['free'][:, :, None], shape)].any(), f'{what}: fixed-atom {name}'
        if ref['frozen']:
            assert _same_bits(xo, x), f'{what}: a frozen band moved'
            assert _same_bits(vo, v) and out['dt'][k] == d['dt'][k] and out['a'][k] == d['a'][k], f'{what}: FIRE state touched'
            continue
        within('x', xo, ref['x_out'], ref['bx'], what)
        within('v', vo, new['vel'], ref['b_vel_out'], what)
        within('dt', out['dt'][k], new['dt'], ref['b_dt_out'], what)
        within('a', out['a'][k], new['a'], ref['b_a_out'], what)
        assert _same_bits(xo[held], x[held]) and _same_bits(vo[held], v[held]), f'{what}: an endpoint or a fixed atom moved'
        assert (xo[~held] != x[~held]).any(), f'{what}: nothing moved'
    if flags == nr.CLIMB:
        for want in ([(kind, fire, c) for kind, fire in (('first', 'first'), ('pos_low', 'mix'), ('pos_high', 'mix_inc'), ('cap', 'mix_inc'),
                                                         ('neg', 'reset')) for c in (False, True)]
                     + [('first', False, 'first', True, False, False), ('converged', True, None, False, True, False), ('converging', True, None, False, True, True),
                        ('pending', False, 'mix', False, False, True), ('switch', False, 'mix', False, False, True),
                        ('climbing', False, 'mix', False, False, True), ('climbing', False, 'mix', True, False, True),
                        ('coincident', False, 'mix', False, False, False), ('flat', False, 'mix', False, False, False)]):
            assert want in seen, want
    print(f'neb_step flags = {flags}, {len(syn)} bands, {d["E"].shape[0]} images, {d["x"].shape[0]} atoms: worst err / bound '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f' (C_NEB = {nr.C_NEB})')


def test_a_null_mask_means_all_atoms_free(syn):
    free = [dict(b, free=np.ones_like(b['free'])) for b in syn]
    a, b = _launch(free, nr.CLIMB, use_mask=True), _launch(free, nr.CLIMB, use_mask=False)
    for k in OUT + STATE:
        assert _same_bits(a[k], b[k]) or k == 'fmax' and np.array_equal(a[k], b[k], equal_nan=True), k
    assert not _same_bits(a['pos_out'], _launch(syn, nr.CLIMB)['pos_out'])          # and the mask of the other tests does something


# ---- 2. a band's result does not depend on the batch --------------------------------------------------------------------------------

def test_each_band_alone_and_the_reversed_batch_give_the_bits_of_the_batch(syn):
    whole = _launch(syn, nr.CLIMB)
    d = whole['flat']
    rev = _launch(syn[::-1], nr.CLIMB)
    K = len(syn)
    for k, b in enumerate(syn):
        rows, _ = _rows(d, k)
        rrows, rmols = _rows(rev['flat'], K - 1 - k)
        one = _launch([b], nr.CLIMB)
        what = f'band {k} ({b["kind"]}, {b["n_img"]} images of {b["n"]} atoms)'
        for name in ('pos_out', 'neb_force', 'tangent', 'vel'):
            assert _same_bits(one[name], whole[name][rows]), f'{what}: {name} alone'
            assert _same_bits(rev[name][rrows], whole[name][rows]), f'{what}: {name} reversed'
        for name in INTS + ('dt', 'a', 'fmax'):
            assert _same_bits(one[name], whole[name][k:k + 1]), f'{what}: {name} alone'
            assert _same_bits(rev[name][K - 1 - k:K - k], whole[name][k:k + 1]), f'{what}: {name} reversed'
        if b['kind'] != 'unequal':
            first = int(d['band_ptr'][k])
            assert int(one['saddle'][0]) == int(whole['saddle'][k]) - first == int(rev['saddle'][K - 1 - k]) - rmols.start, what


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------

def test_neb_step_refuses_bad_arguments_and_writes_nothing(syn):
    from newtonnet_amd import hip
    band = syn[16]
    assert band['n'] > 2 and band['kind'] == 'pos_high'
    t = _tensors(nr.flatten([band]))
    keep = {k: v.clone() for k, v in t.items()}
    N = t['x'].shape[0]
    with pytest.raises(hip.HipLibraryError, match='alias'):
        _call(dict(t, pos_out=t['x']))
    flat = torch.zeros(3 * N + 3, device='cuda')
    with pytest.raises(hip.HipLibraryError, match='alias'):          # an overlapping view is an alias too
        _call(dict(t, x=flat[:3 * N].view(N, 3), pos_out=flat[3:].view(N, 3)))
    with pytest.raises(hip.HipLibraryError, match='flags'):
        _call(t, flags=4)
    for name in ('spring', 'tol2', 'climb2', 'dt', 'dt_max', 'f_inc', 'f_dec', 'a_start', 'f_a', 'maxstep'):
        for bad in (0.0, -1.0, float('nan')):
            with pytest.raises(hip.HipLibraryError, match='must all be > 0'):
                _call(t, **{name: bad})
    with pytest.raises(hip.HipLibraryError, match='n_min'):
        _call(t, n_min=-1)
    # image counts outside 3 .. NNHIP_NEB_MAX_IMAGES: two images; 65 single-atom images
    two = dict(t, band_ptr=torch.tensor([0, 2], dtype=torch.int32, device='cuda'), band_ptr_host=torch.tensor([0, 2], dtype=torch.int32),
               ptr=t['ptr'][:3].clone(), E=t['E'][:2])
    n2 = int(two['ptr'][2])
    for k in ('x', 'F', 'vel', 'pos_out', 'neb_force', 'tangent'):
        two[k] = t[k][:n2]
    two['free'] = t['free'][:n2]
    with pytest.raises(hip.HipLibraryError, match='images'):
        _call(two)
    many = nr.MAX_IMAGES + 1
    big = dict(x=np.zeros((many, 3), np.float32), F=np.zeros((many, 3), np.float32), E=np.zeros(many, np.float32), free=np.ones(many, bool),
               ptr=np.arange(many + 1, dtype=np.int32), band_ptr=np.array([0, many], np.int32), vel=np.zeros((many, 3), np.float32),
               dt=np.zeros(1, np.float32), a=np.zeros(1, np.float32), **{k: np.zeros(1, np.int32) for k in INTS})
    tb = _tensors(big)
    with pytest.raises(hip.HipLibraryError, match='images'):
        _call(tb)
    with pytest.raises(hip.HipLibraryError, match='band_ptr'):       # the band list does not cover the molecules
        _call(dict(t, band_ptr_host=torch.tensor([0, 3], dtype=torch.int32)))
    # null mandatory pointers: straight at the C ABI (the Python wrapper would not let a None through)
    L = hip.lib()
    order = ('x', 'F', 'E', 'free', 'ptr', 'band_ptr', 'band_ptr_host', 'converged', 'climbing', 'n_steps', 'n_pos', 'dt', 'a', 'vel',
             'pos_out', 'neb_force', 'tangent', 'fmax', 'saddle')
    B = t['E'].shape[0]

    def raw(null=(), n_bands=1, n_mol=B, n_atoms=N):
        p = {k: (None if k in null else hip._ptr(t[k])) for k in order}
        return L.nnhip_neb_step(p['x'], p['F'], p['E'], p['free'], p['ptr'], p['band_ptr'], p['band_ptr_host'], n_bands, n_mol, n_atoms,
                                PRM['spring'], PRM['tol2'], PRM['climb2'], *_fire(PRM), 0, p['converged'], p['climbing'], p['n_steps'],
                                p['n_pos'], p['dt'], p['a'], p['vel'], p['pos_out'], p['neb_force'], p['tangent'], p['fmax'], p['saddle'],
                                hip._stream(t['x'].device))
    for name in order:
        if name != 'free':
            assert raw(null=(name,)) != 0, f'a null {name} was accepted'
    assert raw(n_bands=-1) != 0 and raw(n_atoms=-1) != 0
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(t[k], v), f'{k} was written by a refused call'
    assert torch.all(tb['pos_out'] == SENT) and torch.all(tb['fmax'] == SENT)
    # empty batches are no-ops that succeed
    assert raw(n_bands=0) == 0 and raw(null=order, n_bands=0, n_mol=0, n_atoms=0) == 0
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(t[k], v), f'{k} was written by an empty launch'
    # and the same tensors are accepted as they are
    _call(t)
    torch.cuda.synchronize()
    assert not torch.equal(t['pos_out'], keep['pos_out']) and int(t['n_steps'][0]) == int(keep['n_steps'][0]) + 1


# ---- the physical bands ---------------------------------------------------------------------------------------------------------------

def _setup(case, weights):
    z, pos, cell, batch, _ = util.case_inputs(case, torch.float32)
    z, pos, cell, batch = cuda(z, pos, cell, batch)
    return make_model(util.load_state(weights)), z, pos, cell, batch


def _stack(bands):
    """z, pos, cell, batch of a list of bands (each [I,n,3] numpy positions with its z [n])"""
    zs, ps, bs = [], [], []
    m = 0
    for z, x in bands:
        for img in x:
            zs.append(np.asarray(z))
            ps.append(np.asarray(img, dtype=np.float32))
            bs.append(np.full(len(z), m))
            m += 1
    return (torch.from_numpy(np.concatenate(zs)).long().cuda(), torch.from_numpy(np.concatenate(ps)).cuda(),
            torch.zeros(m, 3, 3, device='cuda'), torch.from_numpy(np.concatenate(bs)).long().cuda())


@pytest.fixture(scope='module')
def aspirin():
    """the shipped model, aspirin8_ckpt molecule 0 relaxed on the device (endpoint A) and the raw molecules"""
    model, z, pos, cell, batch = _setup('aspirin8_ckpt', 'ckpt')
    rel = model.relaxation(z[:21], pos[:21], cell[:1], batch[:21])
    res = rel.run(600, check_every=10)
    assert bool(res.converged.all())
    return dict(model=model, z=_np(z[:21]), A=_np(res.pos).astype(np.float64), raw=_np(pos).reshape(8, 21, 3).astype(np.float64))


# ---- 4. stepwise consistency of the driver ------------------------------------------------------------------------------------------

def check_stepwise(band, frames, label):
    """frames: per step k = 0 .. R the dict(pos, force, energy, dt) the recording holds (k = 0: the start).  One neb_ref.neb_step
    per band from the state the reference itself has carried from the frames <= k -- velocities and a with their first-order bounds,
    dt taken from the record -- must land on frame k + 1 within the bound.  A band-step with an ambiguous decision is skipped and
    counted, and the state then follows what the record shows the kernel decided (bits kept: converged; dt halved: P <= 0); the climb
    switch leaves no trace in a frame, so after an ambiguous one both states are tried on the next step.  Returns (band-steps,
    skipped, worst err / bound)."""
    ptr, bptr = _np(band._mol_ptr), _np(band._band_ptr)
    prm = dict(nr.FIRE, spring=band._spring, tol2=band._tol2, climb2=band._climb2)
    prm.update(dict(zip(('dt', 'dt_max', 'n_min', 'f_inc', 'f_dec', 'a_start', 'f_a', 'maxstep'), band._fire)))
    total = skipped = 0
    worst = 0.0
    for k in range(band.n_bands):
        m0, m1 = int(bptr[k]), int(bptr[k + 1])
        rows = slice(int(ptr[m0]), int(ptr[m1]))
        shape = (m1 - m0, int(ptr[m0 + 1] - ptr[m0]), 3)
        states = [nr.new_state(shape[0], shape[1])]
        for s in range(len(frames) - 1):
            f0, f1 = frames[s], frames[s + 1]
            x, F, E = f0['pos'][rows].reshape(shape), f0['force'][rows].reshape(shape), f0['energy'][m0:m1]
            x1 = f1['pos'][rows].reshape(shape)
            stayed = _same_bits(x1, x)
            total += 1
            best = None
            for st in states:
                ref = nr.neb_step(x, F, E, None, st, prm, band._flags)
                amb = ref['ambiguous']
                if any(amb.values()) and not st['converged']:
                    halved = float(f1['dt'][k]) == float(np.float32(np.float32(f0['dt'][k]) * np.float32(prm['f_dec'])))
                    ref = nr.neb_step(x, F, E, None, st, prm, band._flags,
                                      decide=dict(converge=stayed, **({'P': not halved} if st['n_steps'] else {})))
                if ref['frozen'] != stayed:
                    ratio = float('inf')
                else:
                    err, lim = np.abs(x1.astype(np.float64) - ref['x_out']), ref['bx'] + nr.half_ulp32(ref['x_out'])
                    ratio = float(np.max(err / lim))
                if best is None or ratio < best[0]:
                    best = (ratio, ref, any(amb.values()))
            ratio, ref, ambiguous = best
            what = f'{label}: step {s} -> {s + 1}, band {k}'
            if ambiguous or len(states) > 1:
                skipped += 1
            else:
                assert ratio <= 1.0, f'{what}: positions err / bound {ratio:.3f} (frozen {ref["frozen"]}, bits kept {stayed})'
                if not ref['frozen']:
                    worst = max(worst, ratio)
                    new = ref['state']
                    assert abs(float(f1['dt'][k]) - new['dt']) <= ref['b_dt_out'] + nr.half_ulp32(new['dt']), f'{what}: dt'
            new = ref['state']
            if not ref['frozen']:
                new.update(dt=float(f1['dt'][k]), b_dt=0.0)               # the recorded fp32 value
            states = [new]
            if ref['ambiguous']['climb']:
                states.append(dict(nr.copy_state(new), climbing=not new['climbing']))
    print(f'{label}: {total} band-steps, {skipped} skipped as ambiguous, worst err / bound {worst:.4f}')
    return total, skipped, worst


def _frames(start, res):
    out = [start]
    for r in range(res.traj_step.numel()):
        out.append(dict(pos=_np(res.traj_pos[r]), force=_np(res.traj_force[r]), energy=_np(res.traj_energy[r]), dt=_np(res.traj_dt[r])))
    return out


@pytest.mark.parametrize('case', ['aspirin', 'mixed_rand'])
def test_every_recorded_step_follows_from_the_frames_before(case, aspirin):
    if case == 'aspirin':
        model, zA = aspirin['model'], aspirin['z']
        bands = [(zA, nr.methyl_rotation_band(zA, aspirin['raw'][0], 5)), (zA, nr.methyl_rotation_band(zA, aspirin['raw'][1], 7))]
        counts = [5, 7]
    else:
        model, z, pos, cell, batch = _setup('mixed_rand', 'rand')
        rng = np.random.default_rng(11)
        x = _np(pos[:21]).astype(np.float64)
        a, b = x + rng.normal(0, 0.03, x.shape), x + rng.normal(0, 0.03, x.shape)
        w = np.linspace(0, 1, 5)[:, None, None]
        bands = [(_np(z[:21]), a[None] * (1 - w) + b[None] * w)]
        counts = [5]
    z, pos, cell, batch = _stack(bands)
    band = model.band(z, pos, cell, batch, counts, spring=0.1, fmax=0.01, climb_below=0.05)
    start = dict(pos=_np(band.positions), force=_np(band.forces), energy=_np(band.potential_energy),
                 dt=np.zeros(len(counts), np.float32))
    before = model.deferred_stats()
    res = band.run(40, check_every=0, record_every=1)
    assert model.deferred_stats()['repeats_needed'] == before['repeats_needed']
    assert res.traj_step.tolist() == list(range(1, 41)) and res.traj_pos.shape == (40,) + tuple(pos.shape)
    assert res.traj_force.shape == res.traj_pos.shape and res.traj_energy.shape == (40, sum(counts)) and res.traj_dt.shape == (40, len(counts))
    frames = _frames(start, res)
    # the recorded forces and energies are the model's at the recorded positions (a repeat from the wrong buffer would show here)
    worst = 0.0
    for f in frames:
        out = model(z, torch.from_numpy(f['pos']).cuda(), cell, batch)
        worst = max(worst, float((out.gradient_force - torch.from_numpy(f['force']).cuda()).abs().max()))
        assert np.all(np.abs(_np(out.energy).astype(np.float64) - f['energy']) <= util.energy_tol(f['energy']))
    print(f'{case}: recorded forces against model(recorded positions): max difference {worst:.3e} eV/A (allowed {util.FORCE_MAX_TOL})')
    assert worst <= util.FORCE_MAX_TOL
    total, skipped, _ = check_stepwise(band, frames, case)
    assert total == 40 * len(counts) and skipped <= 0.01 * total, f'{skipped} of {total} band-steps are ambiguous'
    assert torch.equal(res.pos, res.traj_pos[-1]) and torch.equal(res.energy, res.traj_energy[-1])
    assert res.n_steps.tolist() == [40] * len(counts)
    # endpoints never move
    bp = np.concatenate([[0], np.cumsum(counts)])
    for k in range(len(counts)):
        for m in (bp[k], bp[k + 1] - 1):
            sl = batch == int(m)
            assert torch.equal(res.pos[sl], pos[sl])


# ---- 5. convergence -----------------------------------------------------------------------------------------------------------------------

NU_STAR = 109.8      # cm^-1: |imaginary frequency| of the CPU oracle's projected, mass-weighted Hessian at the host loop's climbing image


def test_methyl_rotation_converges_like_the_host_fp64_loop(aspirin):
    """Methyl rotation of aspirin (aspirin8_ckpt molecule 0 relaxed on the device; shipped weights), 7 images, spring 0.1 eV/A^2,
    fmax 0.01 eV/A, climbing image below 0.05 eV/A.  The yardstick is neb_ref.minimise (fp64 positions and arithmetic) driven by
    model() from the same start.  The device must converge within 1.5 x the host loop's steps (relax's margin: FIRE's path is not
    monotone and fp32 rounding shifts step counts), pick the same saddle image, give barriers within 2 util.energy_tol(E) of the host
    loop's, leave a recomputed |f| on the climbing image below fmax + util.FORCE_MAX_TOL, and model.frequencies there must show
    exactly one frequency below -NU_STAR / 2 and none at endpoint A.
    On the CPU oracle (fp64 model, positions and outputs rounded to fp32; endpoint A from relax_ref.minimise) the host loop took 151
    steps with the climbing image on from step 24, image 3, both barriers 0.0371 eV, true |f| 0.0064 eV/A there, and the projected
    mass-weighted oracle Hessian at that image has ONE imaginary frequency, NU_STAR = 109.8i cm^-1 (the next three eigenvalues are
    projected zeros; the lowest eigenvalue of the plain Hessian is -0.055 eV/A^2, the next -2e-4), and none at A.
    Measured on an MI355X when the test was written: device 151 steps, saddle image 3, barriers 0.03711 / 0.03711 eV (19 fp32 ulps
    of the energy), NEB fmax 0.00996, true |f| on the climbing image 0.00641 eV/A; host fp64 loop on model() forces 151 steps
    (climbing from step 24), image 3, the same barriers; lowest frequencies at the climbing image -110.0, -1.6, -1.4 cm^-1 and at
    endpoint A -1.3, -1.2, -1.2 cm^-1."""
    model, zA, A = aspirin['model'], aspirin['z'], aspirin['A']
    x0 = nr.methyl_rotation_band(zA, A, 7).astype(np.float32)
    z, pos, cell, batch = _stack([(zA, x0)])
    assert _same_bits(_np(pos).reshape(7, 21, 3), x0)

    def energy_forces(x):
        out = model(z, torch.from_numpy(x.reshape(-1, 3)).float().cuda(), cell, batch)
        return _np(out.energy).astype(np.float64), _np(out.gradient_force).astype(np.float64).reshape(x.shape)
    host = nr.minimise(energy_forces, x0.astype(np.float64), spring=0.1, fmax=0.01, climb_below=0.05, max_steps=600)
    assert host['converged'], f'the host loop did not converge: fmax {host["fmax"]}'
    limit = int(math.floor(1.5 * host['n_steps']))
    band = model.band(z, pos, cell, batch, 7, spring=0.1, fmax=0.01, climb_below=0.05)
    res = band.run(limit, check_every=10)
    top = int(res.saddle_image[0])
    out = model(z, res.pos, cell, batch)
    f_top = float(out.gradient_force[21 * top:21 * (top + 1)].norm(dim=1).max())
    bf, br = float(res.barrier_forward[0]), float(res.barrier_reverse[0])
    print(f'device: {int(res.n_steps[0])} steps, saddle image {top}, barriers {bf:.5f} / {br:.5f} eV, NEB fmax {float(res.fmax[0]):.5f}, '
          f'true |f| on the climbing image {f_top:.5f} eV/A; host fp64 loop: {host["n_steps"]} steps (climbing from step '
          f'{host["climb_step"]}), image {host["saddle"]}, barriers {host["barrier_forward"]:.5f} / {host["barrier_reverse"]:.5f} eV '
          f'(limit {limit} steps)')
    assert bool(res.converged[0]) and bool(res.climbing[0]), f'not converged within {limit} steps: fmax {float(res.fmax[0])}'
    assert int(res.n_steps[0]) <= limit and float(res.fmax[0]) < 0.01
    assert top == host['saddle']
    tol = 2.0 * float(util.energy_tol(host['energy'][host['saddle']]))
    assert abs(bf - host['barrier_forward']) <= tol and abs(br - host['barrier_reverse']) <= tol
    assert bf > 0.02 and br > 0.02                                     # a barrier, resolved by more than ten ulps of the energy
    assert f_top < 0.01 + util.FORCE_MAX_TOL
    assert torch.equal(res.energy, out.energy)
    one = (z[:21], None, cell[:1], batch[:21])
    nu_top = _np(model.frequencies(one[0], res.pos[21 * top:21 * (top + 1)], one[2], one[3]))
    nu_A = _np(model.frequencies(one[0], pos[:21], one[2], one[3]))
    print(f'frequencies at the climbing image: lowest {nu_top[:3]} cm^-1; at endpoint A: lowest {nu_A[:3]} cm^-1 (NU_STAR {NU_STAR})')
    assert int((nu_top < -NU_STAR / 2).sum()) == 1 and int((nu_A < -NU_STAR / 2).sum()) == 0


# ---- 6. bitwise properties ----------------------------------------------------------------------------------------------------------------

RESULT = ('pos', 'energy', 'neb_force', 'tangent', 'fmax', 'converged', 'climbing', 'n_steps', 'saddle_image', 'barrier_forward',
          'barrier_reverse')


def test_bitwise_properties(aspirin):
    model, zA, A = aspirin['model'], aspirin['z'], aspirin['A']
    z, pos, cell, batch = _stack([(zA, nr.methyl_rotation_band(zA, A, 7)), (zA, nr.methyl_rotation_band(zA, A, 5))])
    keep = [t.clone() for t in (z, pos, cell, batch)]
    n_run = 80

    def make(**kw):
        return model.band(z, pos, cell, batch, [7, 5], spring=0.1, fmax=0.03, climb_below=0.1, **kw)
    # the same run twice; check_every = 0 (never reads, all launches), 1 and 7 (stop early)
    a = make().run(n_run, 0, record_every=1)
    n_steps = a.n_steps.tolist()
    print(f'two bands (7 and 5 images) to fmax 0.03 eV/A: {n_steps} steps, barriers {a.barrier_forward.tolist()}')
    assert bool(a.converged.all()) and a.traj_step.tolist() == list(range(1, n_run + 1))
    for every in (0, 1, 7):
        b = make().run(n_run, every)
        for name in RESULT:
            assert torch.equal(getattr(a, name), getattr(b, name)), f'check_every = {every}: {name}'
    # a converged band's frames are constant, bit for bit, from the step after its last one
    assert max(n_steps) < n_run and min(n_steps) > 23
    for k, (n, sl, ms) in enumerate(zip(n_steps, (slice(0, 147), slice(147, 252)), (slice(0, 7), slice(7, 12)))):
        assert torch.equal(a.traj_pos[n - 1:, sl], a.traj_pos[n - 1, sl].expand(n_run + 1 - n, -1, -1)), f'band {k} moved after step {n}'
        assert not torch.equal(a.traj_pos[n - 2, sl], a.traj_pos[n - 1, sl])
        assert torch.equal(a.traj_energy[n - 1:, ms], a.traj_energy[n - 1, ms].expand(n_run + 1 - n, -1))
        assert torch.equal(a.traj_dt[n - 1:, k], a.traj_dt[n - 1, k].expand(n_run + 1 - n))
    # run(a); run(b) leaves the bits of run(a + b); recording changes nothing
    band = make()
    first = band.run(23, 0)
    assert band.step_count == 23 and first.n_steps.tolist() == [23, 23]
    second = band.run(n_run - 23, 10, record_every=10)
    assert second.traj_step[0].item() == 33
    for name in RESULT:
        assert torch.equal(getattr(a, name), getattr(second, name)), name
    assert torch.equal(first.pos, a.traj_pos[22]) and torch.equal(first.energy, a.traj_energy[22])
    assert torch.equal(band.positions, a.pos)
    again = band.run(5, 0)                                              # everything has converged: nothing changes any more
    for name in RESULT:
        assert torch.equal(getattr(a, name), getattr(again, name)), name
    # fixed atoms never move, the others do
    fixed = torch.zeros(252, dtype=torch.bool, device='cuda')
    fixed[::5] = True
    h = make(fixed=fixed).run(60, 10, record_every=1)
    assert torch.equal(h.traj_pos[:, fixed], pos[fixed].expand(h.traj_pos.shape[0], -1, -1)) and torch.equal(h.pos[fixed], pos[fixed])
    assert (h.pos[~fixed] != pos[~fixed]).any() and not h.neb_force[fixed].any()
    # the caller's tensors are never modified
    for t, k in zip((z, pos, cell, batch), keep):
        assert torch.equal(t, k)


# ---- 7. interfaces ------------------------------------------------------------------------------------------------------------------------

def test_calculator_neb_equals_the_model_path(aspirin):
    from newtonnet_amd.neb import Band, BandResult, interpolate
    from newtonnet_amd.utils import MLAseCalculator
    from tests.test_hip_md import FakeAtoms
    model, zA, A = aspirin['model'], aspirin['z'], aspirin['A']
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda')
    x7, x5 = nr.methyl_rotation_band(zA, A, 7).astype(np.float32), nr.methyl_rotation_band(zA, A, 5).astype(np.float32)
    bands = [[FakeAtoms(zA, img) for img in x7], [FakeAtoms(zA, img) for img in x5]]
    out = calc.neb(bands, fmax=0.05, max_steps=30)
    z, pos, cell, batch = _stack([(zA, x7), (zA, x5)])
    band = model.band(z, pos, cell, batch, [7, 5], fmax=0.05)
    res = band.run(30, check_every=10)
    assert isinstance(band, Band) and isinstance(res, BandResult) and res.traj_pos is None
    assert np.array_equal(out['positions'][0].reshape(-1, 3), _np(res.pos[:147])) and np.array_equal(out['positions'][1].reshape(-1, 3), _np(res.pos[147:]))
    assert np.array_equal(out['energy'][1], _np(res.energy[7:])) and np.array_equal(out['fmax'], _np(res.fmax))
    assert np.array_equal(out['saddle_image'], _np(res.saddle_image) - np.array([0, 7])) and np.array_equal(out['n_steps'], _np(res.n_steps))
    assert np.array_equal(out['barrier_forward'], _np(res.barrier_forward)) and out['converged'].dtype == np.bool_
    assert all(np.array_equal(f.positions, img) for f, img in zip(bands[0], x7))
    one = calc.neb(bands[1], fmax=0.05, max_steps=4)                    # a single band drops the band axis
    assert one['positions'].shape == (5, 21, 3) and one['energy'].shape == (5,) and one['n_steps'] == 4 and not one['converged']
    # interpolate on the device: endpoints bitwise
    im = interpolate(pos[:21], pos[126:147], 4)
    assert im.is_cuda and torch.equal(im[0], pos[:21]) and torch.equal(im[-1], pos[126:147])
    for bad in (dict(max_steps=-1), dict(max_steps=3, check_every=-1), dict(max_steps=3, record_every=2.5)):
        with pytest.raises(ValueError):
            band.run(**bad)
    assert band.run(0).n_steps.tolist() == res.n_steps.tolist()
