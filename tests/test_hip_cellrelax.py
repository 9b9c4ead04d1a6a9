"""Batched variable-cell relaxation on the HIP path (newtonnet_amd/cellrelax.py, csrc/cellrelax.hip).

Kernel alone: nnhip_cell_lbfgs_step on synthetic inputs that reach every branch at every size class
(tests/cellrelax_ref.synthetic_batch; tests/test_cellrelax_host.py shows on the CPU that none of its decisions is ambiguous)
against its fp64 restatement on the SAME fp32 inputs, stage by stage (cellrelax_ref.check_launch): every float output within the
derived first-order bound (C_RX = 2) plus half an fp32 ulp of the stored value, integers and flags exact, y and S[head] bitwise,
everything a step must not touch bitwise untouched under sentinel-filled outputs; the tests print err / bound.  Driver: every
step of a model-driven run is held to the same check from the state the device holds before it, so no error compounds;
convergence is measured on an analytic crystal with a known minimum and against a host fp64 loop of the same reference."""
import math

import numpy as np
import pytest
import torch

from tests import cellrelax_ref as cr
from tests import relax_ref as rr
from tests import util
from tests.test_cellrelax_host import host_crystal, metric_bound
from tests.test_hip_hessian import cuda, make_model

pytestmark = pytest.mark.gpu

SENT = cr.SENT
INTS = cr.INTS
STATE = ('S', 'Y', 'rho', 'g_prev') + INTS
VIRIAL_TOL = 2e-5          # x max(1, |W|): the tolerance tests/test_hip_parity.py::test_virial_and_stress holds the virial head to


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def syn():
    return cr.synthetic_batch()


def _tensors(d):
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda()
         for k in ('X', 'pos', 'f', 'W', 'cell', 'h0', 'free', 'ptr', 'p', 'c') + STATE}
    R, N, B = d['X'].shape[0], d['pos'].shape[0], len(d['ptr']) - 1
    for name, shape in (('G', (R, 3)), ('x_out', (R, 3)), ('pos_out', (N, 3)), ('cell_out', (B, 3, 3)), ('fmax', (B,)),
                        ('work', (R, 3))):
        t[name] = torch.full(shape, SENT, device='cuda')
    return t


def _call(d, t, bits=cr.MASK_ALL, flags=0, use_mask=True, **over):
    from newtonnet_amd import hip
    kw = dict(memory=d['memory'], tol2=d['tol2'], alpha=d['alpha'], maxstep=d['maxstep'])
    kw.update(over)
    hip.cell_lbfgs_step(t['X'], t['pos'], t['f'], t['W'], t['cell'], t['h0'], t['free'] if use_mask else None, t['ptr'], t['p'], t['c'],
                        kw['memory'], kw['tol2'], kw['alpha'], kw['maxstep'], bits, flags, t['converged'], t['n_steps'], t['n_pairs'],
                        t['head'], t['S'], t['Y'], t['rho'], t['g_prev'], t['work'], t['G'], t['x_out'], t['pos_out'], t['cell_out'],
                        t['fmax'])


def _launch(d, bits=cr.MASK_ALL, flags=0, use_mask=True):
    """one launch on a batch in the kernel's layout; returns the inputs as they are afterwards and the sentinel-filled outputs"""
    t = _tensors(d)
    _call(d, t, bits, flags, use_mask)
    return {k: _np(v) for k, v in t.items()}


# ---- 1. the kernel against fp64 on the same inputs ---------------------------------------------------------------------------------

@pytest.mark.parametrize('bits,flags', list(cr.SYN_OPTIONS) + [(cr.MASK_ALL, cr.CHECK_ONLY)])
def test_cell_lbfgs_step_against_fp64_on_the_same_inputs(syn, bits, flags):
    d = syn
    out = _launch(d, bits, flags)
    for k in ('X', 'pos', 'f', 'W', 'cell', 'h0', 'ptr', 'p', 'c'):
        assert _same_bits(out[k], d[k]), f'input {k} was modified'
    worst, seen, ambiguous = cr.check_launch(d, out, bits, flags)
    print(f'cell_lbfgs_step strain_mask = {bits}, flags = {flags}, {len(d["kinds"])} systems, {d["X"].shape[0]} rows: worst err / '
          f'bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f' (C_RX = {cr.C_RX}); ambiguous {ambiguous}')
    assert not ambiguous
    if bits == cr.MASK_ALL and flags == 0:
        for want in ([('accept', 'step', True, False, False), ('accept', 'step', True, True, False), ('accept', 'step', True, True, True),
                      ('first', 'step', None, False, False), ('first', 'step', None, True, False), ('first', 'step', None, True, True),
                      ('converged', 'frozen', None, False, False), ('converging', 'frozen', None, False, False),
                      ('det_neg', 'skip', None, False, False)]
                     + [(k, 'step', False, cl, False) for k in ('reject_neg', 'reject_cos') for cl in (False, True)]):
            assert want in seen, want
    if flags & cr.CHECK_ONLY:
        assert all(s[1] in ('frozen', 'skip') for s in seen)


def test_a_null_mask_means_all_atoms_free(syn):
    d = dict(syn, free=np.ones_like(syn['free']))
    a, b = _launch(d, use_mask=True), _launch(d, use_mask=False)
    for k in ('x_out', 'pos_out', 'cell_out', 'G', 'fmax') + STATE:
        assert _same_bits(a[k], b[k]), k
    assert not _same_bits(a['x_out'], _launch(syn)['x_out'])          # and the mask of the other tests does something


# ---- 2. a system's result does not depend on the batch ------------------------------------------------------------------------------

def test_each_system_alone_gives_the_bits_it_gave_in_the_batch(syn):
    d = syn
    bits, flags = 0b111011, cr.CONSTANT_VOLUME
    whole = _launch(d, bits, flags)
    for b in range(len(d['kinds'])):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        r0, _, r1 = cr.rows_of(d, b)
        one = _launch(cr.slice_batch(d, b), bits, flags)
        what = f'system {b} ({d["kinds"][b]}, {a1 - a0} atoms)'
        for k in ('x_out', 'G', 'g_prev'):
            assert _same_bits(one[k], whole[k][r0:r1]), f'{what}: {k}'
        assert _same_bits(one['pos_out'], whole['pos_out'][a0:a1]) and _same_bits(one['cell_out'], whole['cell_out'][b:b + 1]), what
        assert _same_bits(one['S'], whole['S'][:, r0:r1]) and _same_bits(one['Y'], whole['Y'][:, r0:r1]), what
        for k in ('fmax', 'rho') + INTS:
            assert _same_bits(one[k], whole[k][b:b + 1]), f'{what}: {k}'


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------

def test_cell_lbfgs_step_refuses_aliases_null_pointers_and_bad_numbers(syn):
    from newtonnet_amd import hip
    b = next(i for i, (k, n) in enumerate(zip(syn['kinds'], np.diff(syn['ptr']))) if k == 'accept' and n == 21)
    d = cr.slice_batch(syn, b)
    n, m = d['pos'].shape[0], d['memory']
    t = _tensors(d)
    keep = {k: v.clone() for k, v in t.items()}
    with pytest.raises(hip.HipLibraryError, match='alias'):
        _call(d, dict(t, x_out=t['X']))
    with pytest.raises(hip.HipLibraryError, match='alias'):
        _call(d, dict(t, pos_out=t['pos']))
    with pytest.raises(hip.HipLibraryError, match='alias'):
        _call(d, dict(t, cell_out=t['cell']))
    flat = torch.zeros(3 * n + 3, device='cuda')
    with pytest.raises(hip.HipLibraryError, match='alias'):          # an overlapping view is an alias too
        _call(d, dict(t, pos=flat[:3 * n].view(n, 3), pos_out=flat[3:].view(n, 3)))
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
    # null mandatory pointers: straight at the C ABI (the Python wrapper would not let a None through)
    L = hip.lib()
    order = ('X', 'pos', 'f', 'W', 'cell', 'h0', 'free', 'ptr', 'p', 'c', 'converged', 'n_steps', 'n_pairs', 'head', 'S', 'Y', 'rho',
             'g_prev', 'work', 'G', 'x_out', 'pos_out', 'cell_out', 'fmax')

    def raw(t, null=(), n_mol=1, n_atoms=n):
        p = [None if k in null else hip._ptr(t[k]) for k in order]
        return L.nnhip_cell_lbfgs_step(*p[:10], n_mol, n_atoms, m, d['tol2'], d['alpha'], d['maxstep'], cr.MASK_ALL, 0, *p[10:],
                                       hip._stream(t['X'].device))
    for name in order:
        if name in ('free', 'work'):
            continue                                                  # optional (work: only needed above 64 rows)
        assert raw(t, null=(name,)) != 0, f'a null {name} was accepted'
        assert b'nnhip_cell_lbfgs_step' in L.nnhip_last_error()
    big = cr.slice_batch(syn, next(i for i, (k, s) in enumerate(zip(syn['kinds'], np.diff(syn['ptr']))) if k == 'accept' and s == 62))
    tb = _tensors(big)
    assert raw(tb, null=('work',), n_atoms=62) != 0, 'no scratch above 64 rows was accepted'
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(t[k], v), f'{k} was written by a refused call'
    assert all(bool(torch.all(tb[k] == SENT)) for k in ('G', 'x_out', 'pos_out', 'cell_out', 'fmax'))
    # empty batches are no-ops that succeed
    assert raw(t, n_mol=0) == 0 and raw(t, null=order, n_mol=0, n_atoms=0) == 0
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(t[k], v), f'{k} was written by an empty launch'
    # a per-system cell_factor or pressure that is not finite (or c <= 0) skips its system and nothing else
    for name, value in (('c', 0.0), ('c', float('nan')), ('p', float('inf'))):
        t2 = _tensors(d)
        t2[name][0] = value
        _call(d, t2)
        assert math.isnan(float(t2['fmax'][0])) and all(bool(torch.all(t2[k] == SENT)) for k in ('G', 'x_out', 'pos_out', 'cell_out'))
        assert all(torch.equal(t2[k], keep[k]) for k in STATE)


# ---- 4. the analytic crystal on the device -------------------------------------------------------------------------------------------

class _DeviceLoop:
    """hip.cell_lbfgs_step driven by a callback, with CellRelaxation's buffers (two of X, pos and cell) and nothing else"""

    def __init__(self, efv, x0, h0, ptr, p, fmax, memory=16, maxstep=0.2, alpha=70.0):
        dev, f32 = 'cuda', torch.float32
        self.efv, self.ptr = efv, torch.from_numpy(np.asarray(ptr, dtype=np.int32)).cuda()
        B, N = len(ptr) - 1, int(ptr[-1])
        R = N + 3 * B
        sizes = np.diff(ptr)
        self.c = torch.from_numpy(sizes.astype(np.float32)).cuda()
        self.p = torch.from_numpy(np.asarray(p, dtype=np.float32)).cuda()
        self.h0 = torch.from_numpy(np.asarray(h0, dtype=np.float32)).cuda()
        X = np.zeros((R, 3), dtype=np.float32)
        for b in range(B):
            r0 = int(ptr[b]) + 3 * b
            X[r0:r0 + sizes[b]] = x0[ptr[b]:ptr[b + 1]]
            X[r0 + sizes[b]:r0 + sizes[b] + 3] = np.float32(sizes[b]) * np.eye(3, dtype=np.float32)
        self.X = [torch.from_numpy(X).cuda(), torch.empty(R, 3, device=dev)]
        self.pos = [torch.from_numpy(np.asarray(x0, dtype=np.float32)).cuda(), torch.empty(N, 3, device=dev)]
        self.cell = [self.h0.clone(), torch.empty(B, 3, 3, device=dev)]
        self.ints = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4)]
        self.S, self.Y = torch.zeros(memory, R, 3, device=dev), torch.zeros(memory, R, 3, device=dev)
        self.rho, self.g_prev, self.G = torch.zeros(B, memory, device=dev), torch.zeros(R, 3, device=dev), torch.zeros(R, 3, device=dev)
        self.work, self.fmax = torch.empty(R, 3, device=dev), torch.zeros(B, device=dev)
        self.num = (memory, float(np.float32(fmax * fmax)), float(np.float32(alpha)), float(np.float32(maxstep)))
        self.cur = 0

    def step(self, flags=0):
        from newtonnet_amd import hip
        cur, other = self.cur, 1 - self.cur
        _, f, W = self.efv(self.pos[cur], self.cell[cur])
        self.f, self.W = f, W
        hip.cell_lbfgs_step(self.X[cur], self.pos[cur], f, W, self.cell[cur], self.h0, None, self.ptr, self.p, self.c, *self.num,
                            cr.MASK_ALL, flags, *self.ints, self.S, self.Y, self.rho, self.g_prev, self.work, self.G, self.X[other],
                            self.pos[other], self.cell[other], self.fmax)
        self.cur = other


def test_analytic_crystal_reaches_its_known_minimum():
    """Eight systems of 8 .. 40 atoms (cellrelax_ref.crystal): E = (V0 K / 2) |eps_G - eps0|^2 + (k / 2) sum |q_i - q_i0|^2, forces and
    virial in closed form, evaluated with torch on the device in fp64 from the fp32 positions and cell and rounded to fp32.  fmax =
    1e-3 eV/A.  All systems converge within 1.5 x the fp64 driver's own step count (test_hip_relax's margin for fp32 against fp64
    histories).

    fmax recomputed.  The last (check-only) launch saw  f32 = fl32(f), W32 = fl32(W)  of the result (x, h) and found every row of
    its G below fmax.  The fp64 G of the same (x, h) differs from that by: the kernel's own rounding (the reference's b_fmax, x
    C_RX); the rounding of f and W to fp32, |df| <= ulp(f) / 2 per component through |F| and |dW| <= ulp(W) / 2 through |F^-T| / c;
    and dF between the kernel's F = X[n:] / c and the F = (h0^-1 h)^T this test rebuilds from the stored cell, at most
    |h0^-1|_inf x (C_RX 4 2^-24 sum_k |h0_ik F_jk|) (three roundings of the dot3, one of the store), through |f| and |Wc| |F^-1| / c.
    The allowance is the sum of the three.

    Metric.  At zero pressure G_cell = -F A / c with A = K V0 (eps_G - eps0): three rows below g give |A|_F <= |F^-1|_2 c sqrt(3) g
    and F^T F - I - 2 eps0 = 2 A / (K V0) (test_cellrelax_host.metric_bound), so |h h^T - h0 (I + 2 eps0) h0^T|_max <=
    (max_i sum_j |h0_ij|)^2 x that, with g = fmax + the allowance above, plus 8 x 2^-24 (max_i sum_j |h_ij|)^2 for h stored in fp32.
    The pressurised system has no closed-form minimum: it is compared with the fp64 driver's.  Both points have cell rows below g,
    and the map F -> F A(F) + p V F^-T is, to first order, K V0 times the strain map corrected by terms of relative size
    |eps_G - eps0| <= 0.05 and p / K = 0.013; twice the zero-pressure bound (both points, each within one bound of the minimum)
    times 2 for those corrections is what the two metrics may differ by."""
    fmax = 1e-3
    c, host = host_crystal(fmax)
    B = len(c['ptr']) - 1
    t = cr.crystal_tensors(c, 'cuda', torch.float64)

    def efv(x, h):
        E, f, W = cr.crystal_efv_torch(t, x.double(), h.double())
        return E, f.float(), W.float()
    loop = _DeviceLoop(efv, c['x0'], c['h0'], c['ptr'], c['p'], fmax)
    limit = int(math.floor(1.5 * host['n_steps'].max()))
    for _ in range(limit):
        loop.step()
    loop.step(cr.CHECK_ONLY)
    n_steps, conv = _np(loop.ints[1]), _np(loop.ints[0])
    print(f'crystal: steps per system device {n_steps.tolist()}, host fp64 {host["n_steps"].tolist()}; device fmax {_np(loop.fmax)}')
    assert conv.all(), f'not converged within {limit} steps: {n_steps.tolist()}'
    assert np.all(n_steps <= np.floor(1.5 * host['n_steps'])), (n_steps, host['n_steps'])
    x, h = _np(loop.pos[loop.cur]).astype(np.float64), _np(loop.cell[loop.cur]).astype(np.float64)
    X = _np(loop.X[loop.cur]).astype(np.float64)
    _, f, W = cr.crystal_efv(c, x, h)
    f32, W32 = _np(loop.f), _np(loop.W)
    assert np.array_equal(f32, f.astype(np.float32)) and np.array_equal(W32, W.astype(np.float32))      # (torch and numpy agree)
    for b in range(B):
        a0, a1 = int(c['ptr'][b]), int(c['ptr'][b + 1])
        n = a1 - a0
        h0 = c['h0'][b].astype(np.float64)
        F = np.linalg.solve(h0, h[b]).T
        G = cr.generalised_forces(f[a0:a1], W[b], F, h[b], c['p'][b], float(n))
        g = np.sqrt((G ** 2).sum(1).max())
        r0, rc, r1 = a0 + 3 * b, a1 + 3 * b, a1 + 3 * b + 3
        pro = cr.prologue(X[rc:r1], f32[a0:a1], W32[b], h[b], None, np.float32(c['p'][b]), np.float32(n))
        Finv = np.linalg.inv(F)
        dF = np.abs(np.linalg.inv(h0)).sum(1).max() * cr.C_RX * 4 * cr.EPS32 * (np.abs(h0) @ np.abs(F).T).max()
        Wc = np.abs(G[n:]).max() * n
        allow = (cr.C_RX * pro['b_fmax']
                 + np.sqrt(3.0) * (3 * rr.half_ulp32(f[a0:a1]).max() * np.abs(F).max() + 3 * rr.half_ulp32(W[b]).max() * np.abs(Finv).max() / n)
                 + np.sqrt(3.0) * 3 * dF * (np.abs(f[a0:a1]).max() + 3 * Wc * np.abs(Finv).max() / n))
        print(f'  system {b} ({n} atoms): recomputed fmax {g:.3e} (allowed {fmax:.0e} + {allow:.1e})')
        assert g < fmax + allow, (b, g, allow)
        rows = np.abs(h0).sum(1).max() ** 2
        store = 8 * cr.EPS32 * np.abs(h[b]).sum(1).max() ** 2
        bound = rows * metric_bound(c, b, fmax + allow, F) + store
        metric = h[b] @ h[b].T
        if c['p'][b] == 0.0:
            dev = np.abs(metric - h0 @ (np.eye(3) + 2.0 * c['eps0'][b]) @ h0.T).max()
        else:
            dev, bound = np.abs(metric - host['cell'][b] @ host['cell'][b].T).max(), 4.0 * bound
        print(f'             metric deviation {dev:.3e} (bound {bound:.3e})')
        assert dev <= bound, (b, dev, bound)


# ---- 5. model-driven, step by step ------------------------------------------------------------------------------------------------------

def _periodic_case(name):
    if name == 'triclinic64':
        c = util.load_npz('case_virial_triclinic64.npz')
        z, batch = torch.from_numpy(c['z']).long(), torch.from_numpy(c['batch']).long()
        pos, cell = torch.from_numpy(c['pos']).float(), torch.from_numpy(c['cell']).float()
    else:
        z, pos, cell, batch, _ = util.case_inputs(name, torch.float32)
    return cuda(z, pos, cell, batch)


def _virial(model, out):
    return out.virial if 'virial' in model.output_properties else -out.displacement_grad


def _driver_batch(rel):
    """the launch that rel._launch() is about to make, as a batch in the kernel's layout (numpy)"""
    cur = rel._cur
    N, B = rel.n_atoms, rel.n_mol
    d = dict(X=rel._x[cur], pos=rel._pos[cur], f=rel._force, W=rel._virial, cell=rel._cells[cur], h0=rel._h0, ptr=rel._mol_ptr,
             p=rel._p, c=rel._c, S=rel._S, Y=rel._Y, rho=rel._rho, g_prev=rel._g_prev, converged=rel._converged, n_steps=rel._n_steps,
             n_pairs=rel._n_pairs, head=rel._head)
    d = {k: _np(v).copy() for k, v in d.items()}
    d['free'] = np.ones(N, dtype=bool) if rel._free is None else _np(rel._free).astype(bool)
    d.update(kinds=['model'] * B, memory=rel.memory, tol2=rel._tol2, alpha=rel._alpha, maxstep=rel._maxstep)
    return d


def _driver_out(rel):
    cur = rel._cur
    out = dict(G=rel._G, x_out=rel._x[cur], pos_out=rel._pos[cur], cell_out=rel._cells[cur], fmax=rel._fmax, S=rel._S, Y=rel._Y,
               rho=rel._rho, g_prev=rel._g_prev, converged=rel._converged, n_steps=rel._n_steps, n_pairs=rel._n_pairs, head=rel._head)
    return {k: _np(v).copy() for k, v in out.items()}


@pytest.mark.parametrize('case,head,kw', [('pbc_batch2_rand', 'virial', dict(pressure=[0.0, 5000.0])),
                                          ('triclinic64', 'stress', dict(mask=[1, 1, 1, 0, 0, 1], pressure=-2000.0))])
def test_every_recorded_step_follows_from_the_state_before(case, head, kw):
    """20 recorded steps with seeded weights.  The recorded force and virial are the model's at the recorded positions and cell
    (util.FORCE_MAX_TOL; VIRIAL_TOL x max(1, |W|)).  A second relaxation of the same inputs is stepped one launch at a time: before
    each launch the state the device holds is read back, after it cellrelax_ref.check_launch holds the launch to the fp64
    restatement from THOSE fp32 inputs -- the forces and the virial the launch consumed are the recorded ones bit for bit, so the
    model's tolerances need no pushing through the step and nothing compounds -- and the positions and the cell it wrote are the
    next recorded frame, bit for bit."""
    n_rec = 20
    z, pos, cell, batch = _periodic_case(case)
    B = cell.shape[0]
    kw = dict(kw)
    if isinstance(kw['pressure'], list):
        kw['pressure'] = torch.tensor(kw['pressure']).cuda()
    fixed = torch.zeros(pos.shape[0], dtype=torch.bool, device='cuda')
    fixed[::9] = True
    model = make_model(util.load_state('rand'), props=('energy', 'gradient_force', head))
    rel = model.cell_relaxation(z, pos, cell, batch, fixed=fixed, **kw)
    before = model.deferred_stats()
    res = rel.run(n_rec, check_every=0, record_every=1)
    assert model.deferred_stats()['repeats_needed'] == before['repeats_needed']
    assert res.traj_step.tolist() == list(range(1, n_rec + 1)) and res.traj_pos.shape == (n_rec,) + tuple(pos.shape)
    assert res.traj_cell.shape == res.traj_virial.shape == (n_rec, B, 3, 3) and res.traj_force.shape == res.traj_pos.shape
    assert res.traj_energy.shape == res.traj_n_pairs.shape == (n_rec, B)
    worst_f = worst_w = 0.0
    for k in range(n_rec):
        out = model(z, res.traj_pos[k], res.traj_cell[k], batch)
        W = _virial(model, out)
        worst_f = max(worst_f, float((out.gradient_force - res.traj_force[k]).abs().max()))
        worst_w = max(worst_w, float((W - res.traj_virial[k]).abs().max()) / max(1.0, float(W.abs().max())))
    print(f'{case}: recorded against model(recorded pos, cell): force {worst_f:.3e} eV/A (allowed {util.FORCE_MAX_TOL}), virial '
          f'{worst_w:.3e} x max(1, |W|) (allowed {VIRIAL_TOL})')
    assert worst_f <= util.FORCE_MAX_TOL and worst_w <= VIRIAL_TOL
    step = model.cell_relaxation(z, pos, cell, batch, fixed=fixed, **kw)
    step._ensure_state()
    worst, n_amb = {}, 0
    moved = 0.0
    for k in range(n_rec):
        d = _driver_batch(step)
        if k > 0:
            assert _same_bits(d['f'], _np(res.traj_force[k - 1])) and _same_bits(d['W'], _np(res.traj_virial[k - 1]))
        other = 1 - step._cur
        with torch.no_grad():
            for buf in (step._G, step._x[other], step._pos[other], step._cells[other]):
                buf.fill_(SENT)
            step._launch()
            step._evaluate()
        out = _driver_out(step)
        w, seen, ambiguous = cr.check_launch(d, out, step._bits, step._flags)
        n_amb += len(ambiguous)
        worst = {key: max(v, worst.get(key, 0.0)) for key, v in w.items()}
        assert all(s[1] == 'step' for s in seen), seen
        assert _same_bits(out['pos_out'], _np(res.traj_pos[k])) and _same_bits(out['cell_out'], _np(res.traj_cell[k])), f'step {k + 1}'
        assert _same_bits(_np(step._n_pairs.long()), _np(res.traj_n_pairs[k]))
        moved = max(moved, float(np.abs(out['cell_out'] - d['cell']).max()))
    print(f'{case} ({head} head): {n_rec} steps x {B} systems, worst err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items())
          + f'; {n_amb} ambiguous decisions; largest cell change of a step {moved:.2e} A')
    assert n_amb == 0 and moved > 1e-5
    # a fixed atom keeps its reference-frame position and rides with the cell
    X0, X1 = _np(rel._x[rel._cur]), _np(step._x[step._cur])
    assert _same_bits(X0, X1)
    rows = _np(rel._atom_rows)[_np(fixed)]
    q0 = _np(pos)[_np(fixed)]
    assert _same_bits(X1[rows], q0) and not _same_bits(_np(res.pos)[_np(fixed)], q0)
    assert torch.equal(res.pos, res.traj_pos[-1]) and torch.equal(res.cell, res.traj_cell[-1])
    assert torch.equal(res.energy, res.traj_energy[-1]) and res.n_steps.tolist() == [n_rec] * B


# ---- 6. model-driven, against the host fp64 loop ---------------------------------------------------------------------------------------

# tools/cellrelax_host_loop.py: cellrelax_ref.minimise on the oracle's fp64 energy, forces and virial for pbc_batch2_rand (216 and 125
# atoms, seeded weights), hydrostatic, fmax = 0.05 eV/A.  Both boxes converge within 300 steps -- after these many -- with V / V0
# between 0.981 and 1.  (300 fp64 evaluations of the oracle take minutes on a CPU: the test carries the result.)
HOST_STEPS = (299, 177)


def test_boxes_converge_like_the_host_fp64_loop():
    """pbc_batch2_rand, seeded weights, virial head, hydrostatic=True, fmax = 0.05 eV/A.  The host fp64 loop on the oracle finds a
    minimum (HOST_STEPS, volume within 0.5 .. 2 V0), so this test takes the convergence form: both boxes must converge within 1.5 x
    the host's slowest box, the launch's own fmax must be below the threshold, and the generalised fmax recomputed in fp64 from
    model(result) below the threshold plus util.FORCE_MAX_TOL (the allowance test_hip_relax gives the same recomputation)."""
    fmax = 0.05
    z, pos, cell, batch = _periodic_case('pbc_batch2_rand')
    model = make_model(util.load_state('rand'), props=('energy', 'gradient_force', 'virial'))
    limit = int(math.floor(1.5 * max(HOST_STEPS)))
    rel = model.cell_relaxation(z, pos, cell, batch, fmax=fmax, hydrostatic=True)
    h_first = _np(rel.potential_energy).astype(np.float64)
    res = rel.run(limit, check_every=10)
    n_steps = _np(res.n_steps)
    out = model(z, res.pos, res.cell, batch)
    f, W, h = _np(out.gradient_force).astype(np.float64), _np(out.virial).astype(np.float64), _np(res.cell).astype(np.float64)
    ptr = _np(rel._mol_ptr)
    ratio = np.linalg.det(h) / np.linalg.det(_np(cell).astype(np.float64))
    g = []
    for b in range(2):
        sl = slice(int(ptr[b]), int(ptr[b + 1]))
        F = np.linalg.solve(_np(cell)[b].astype(np.float64), h[b]).T
        G = cr.generalised_forces(f[sl], W[b], F, h[b], 0.0, float(ptr[b + 1] - ptr[b]), None, cr.MASK_ALL, cr.HYDROSTATIC)
        g.append(np.sqrt((G ** 2).sum(1).max()))
    print(f'steps per box: device {n_steps.tolist()}, host fp64 {list(HOST_STEPS)} (limit {limit}); fmax device {_np(res.fmax)}, '
          f'recomputed {g}; V / V0 {ratio}; energy drop {h_first - _np(res.energy)}')
    assert bool(res.converged.all()) and not bool(res.failed.any()), f'not converged within {limit} steps: {n_steps.tolist()}, {_np(res.fmax)}'
    assert n_steps.max() <= limit
    assert np.all(_np(res.fmax) < fmax) and np.all(np.array(g) < fmax + util.FORCE_MAX_TOL)
    assert np.all(ratio > 0.5) and np.all(ratio < 2.0) and torch.equal(res.energy, out.energy)


# ---- 7. bitwise properties --------------------------------------------------------------------------------------------------------------

RESULT = ('pos', 'cell', 'volume', 'energy', 'enthalpy', 'stress', 'fmax', 'converged', 'failed', 'n_steps')
BITWISE_FMAX = 0.2        # eV/A: with the seeded weights the boxes of pbc_batch2_rand cross it after 45 and 6 steps (they start at 0.50 and 0.29)


def test_bitwise_properties():
    z, pos, cell, batch = _periodic_case('pbc_batch2_rand')
    keep = [t.clone() for t in (z, pos, cell, batch)]
    model = make_model(util.load_state('rand'), props=('energy', 'gradient_force', 'virial'))
    n_run = 60

    def run(max_steps, check_every, record_every=0, **kw):
        kw.setdefault('fmax', BITWISE_FMAX)
        return model.cell_relaxation(z, pos, cell, batch, hydrostatic=True, **kw).run(max_steps, check_every, record_every)
    # the same run twice; check_every = 0 (never reads, all launches), 1 and 7 (stop early)
    a = run(n_run, 0, record_every=1)
    n_steps = a.n_steps.tolist()
    print(f'bitwise: steps per system {n_steps}, fmax {_np(a.fmax)}, volume / V0 {_np(a.volume / torch.linalg.det(cell))}')
    assert a.traj_step.tolist() == list(range(1, n_run + 1)) and not bool(a.failed.any())
    for every in (0, 1, 7):
        b = run(n_run, every)
        for name in RESULT:
            assert torch.equal(getattr(a, name), getattr(b, name)), f'check_every = {every}: {name}'
    # after n_steps[b] every recorded frame of system b is constant, bit for bit
    assert bool(a.converged.all()) and max(n_steps) < n_run and min(n_steps) >= 2
    ptr = _np(model.cell_relaxation(z, pos, cell, batch)._mol_ptr)
    for b, n in enumerate(n_steps):
        sl = slice(int(ptr[b]), int(ptr[b + 1]))
        for t in (a.traj_pos[:, sl], a.traj_cell[:, b], a.traj_energy[:, b], a.traj_n_pairs[:, b], a.traj_virial[:, b]):
            assert torch.equal(t[n - 1:], t[n - 1].expand_as(t[n - 1:])), f'system {b} changed after step {n}'
        assert not torch.equal(a.traj_pos[n - 2, sl], a.traj_pos[n - 1, sl]) and not torch.equal(a.traj_cell[n - 2, b], a.traj_cell[n - 1, b])
    # run(a); run(b) leaves the bits of run(a + b); recording changes nothing
    rel = model.cell_relaxation(z, pos, cell, batch, hydrostatic=True, fmax=BITWISE_FMAX)
    first = rel.run(1, 0)
    second = rel.run(n_run - 1, 10, record_every=25)
    assert rel.step_count <= n_run and first.n_steps.tolist() == [1, 1]
    for name in RESULT:
        assert torch.equal(getattr(a, name), getattr(second, name)), name
    assert torch.equal(first.pos, a.traj_pos[0]) and torch.equal(first.cell, a.traj_cell[0])
    assert torch.equal(rel.positions, a.pos) and torch.equal(rel.cell, a.cell)
    again = rel.run(5, 0)                                               # everything has converged: nothing changes any more
    for name in RESULT:
        assert torch.equal(getattr(a, name), getattr(again, name)), name
    # hydrostatic: the cell stays a multiple of the input cell (to rounding), and it did change
    ratio = _np(a.cell).astype(np.float64)[cell.cpu().numpy() != 0] / cell.cpu().numpy().astype(np.float64)[cell.cpu().numpy() != 0]
    assert np.ptp(ratio.reshape(2, -1), axis=1).max() < 1e-5 and np.all(ratio != 1.0)
    # every strain component masked, zero pressure: F stays exactly I, the three cell rows add only exact zeros to every sum, and
    # the run is Relaxation's on the same inputs, bit for bit
    m = model.cell_relaxation(z, pos, cell, batch, mask=[0, 0, 0, 0, 0, 0]).run(25, 0, record_every=1)
    r = model.relaxation(z, pos, cell, batch).run(25, 0, record_every=1)
    assert torch.equal(m.traj_cell.view(torch.int32), cell[None].expand(25, -1, -1, -1).contiguous().view(torch.int32))
    assert torch.equal(m.traj_pos, r.traj_pos) and torch.equal(m.pos, r.pos) and torch.equal(m.traj_force, r.traj_force)
    assert torch.equal(m.traj_n_pairs, r.traj_n_pairs) and torch.equal(m.fmax, r.fmax) and torch.equal(m.energy, r.energy)
    assert not torch.equal(m.traj_pos[0], m.traj_pos[-1])
    # the caller's tensors are never modified
    for t, k in zip((z, pos, cell, batch), keep):
        assert torch.equal(t, k)
    assert not pos.requires_grad


# ---- 8. interfaces ------------------------------------------------------------------------------------------------------------------------

class PeriodicAtoms:
    """the accessors MLAseCalculator.format_data uses, for a periodic structure"""

    def __init__(self, numbers, positions, cell):
        self.numbers, self.positions, self.cell = np.asarray(numbers), np.asarray(positions, dtype=np.float64), np.asarray(cell, dtype=np.float64)

    def __len__(self):
        return len(self.numbers)

    def get_atomic_numbers(self):
        return self.numbers

    def get_positions(self, wrap=False):
        return self.positions

    def get_cell(self):
        return self.cell

    def get_pbc(self):
        return np.ones(3, dtype=bool)


def test_calculator_relax_cell_equals_the_model_path():
    from newtonnet_amd.cellrelax import CellRelaxation, CellRelaxResult
    from newtonnet_amd.npt import BAR
    from newtonnet_amd.utils import MLAseCalculator
    z, pos, cell, batch = _periodic_case('pbc_batch2_rand')
    model = make_model(util.load_state('rand'), props=('energy', 'gradient_force', 'stress'))
    sel = _np(batch) == 1
    n = int(sel.sum())
    frames = [PeriodicAtoms(_np(z)[sel], _np(pos)[sel] + 0.01 * k, _np(cell)[1]) for k in range(2)]
    keep = [f.positions.copy() for f in frames]
    calc = MLAseCalculator(model, properties=['energy', 'forces', 'stress'], device='cuda')
    fixed = np.zeros(n, dtype=bool)
    fixed[3] = True
    kw = dict(fmax=0.05, pressure=[0.0, 3000.0], mask=[1, 1, 1, 0, 0, 0], cell_factor=50.0)
    out = calc.relax_cell(frames, max_steps=12, fixed=fixed, **kw)
    assert all(np.array_equal(f.positions, k) for f, k in zip(frames, keep))
    assert out['positions'].shape == (2, n, 3) and out['positions'].dtype == np.float32
    assert out['cell'].shape == out['stress'].shape == (2, 3, 3) and out['cell'].dtype == np.float32
    for k, dt in (('volume', np.float32), ('energy', np.float32), ('enthalpy', np.float32), ('fmax', np.float32),
                  ('converged', np.bool_), ('failed', np.bool_), ('n_steps', np.int64)):
        assert out[k].shape == (2,) and out[k].dtype == dt, k
    zz, pp = torch.cat([z[batch == 1]] * 2), torch.cat([torch.from_numpy(f.positions).float().cuda() for f in frames])
    cc, bb = cell[1:2].repeat(2, 1, 1), torch.arange(2, device='cuda').repeat_interleave(n)
    rel = model.cell_relaxation(zz, pp, cc, bb, fmax=0.05, pressure=torch.tensor([0.0, 3000.0]), mask=[1, 1, 1, 0, 0, 0],
                                cell_factor=50.0, fixed=torch.from_numpy(np.tile(fixed, 2)).cuda())
    assert isinstance(rel, CellRelaxation)
    assert np.array_equal(_np(rel._p), (np.array([0.0, 3000.0]) * BAR).astype(np.float32)) and _np(rel._c).tolist() == [50.0, 50.0]
    res = rel.run(12, check_every=10)
    assert isinstance(res, CellRelaxResult) and res.traj_pos is None
    assert np.array_equal(out['positions'].reshape(2 * n, 3), _np(res.pos)) and np.array_equal(out['cell'], _np(res.cell))
    for k in ('volume', 'energy', 'enthalpy', 'stress', 'fmax', 'converged', 'failed', 'n_steps'):
        assert np.array_equal(out[k], _np(getattr(res, k))), k
    # the result's derived fields: volume = det(cell), enthalpy = E + p V, stress = -W / V in bar; masked components stay put
    V = np.linalg.det(out['cell'].astype(np.float64))
    np.testing.assert_allclose(out['volume'], V, rtol=1e-6)
    np.testing.assert_allclose(out['enthalpy'], out['energy'].astype(np.float64) + np.array([0.0, 3000.0]) * BAR * V, rtol=1e-6, atol=1e-5)
    W = _np(rel.virial).astype(np.float64)
    np.testing.assert_allclose(out['stress'], -W / V[:, None, None] / BAR, rtol=1e-5, atol=1e-3)
    F = np.linalg.solve(_np(cell)[1].astype(np.float64), out['cell'][0].astype(np.float64)).T
    assert np.abs(F - np.diag(np.diag(F))).max() < 1e-6 and np.abs(np.diag(F) - 1.0).min() > 1e-5
    one = calc.relax_cell(frames[0], fmax=0.05, max_steps=3)            # a single frame drops the frame axis
    assert one['positions'].shape == (n, 3) and one['cell'].shape == (3, 3) and one['energy'].shape == () and one['n_steps'] == 3
    for bad in (dict(max_steps=-1), dict(max_steps=3, check_every=-1), dict(max_steps=3, record_every=2.5)):
        with pytest.raises(ValueError):
            rel.run(**bad)
    assert rel.run(0).n_steps.tolist() == res.n_steps.tolist()
    # refusals that need the device: a cell without volume, a left-handed cell, no virial head
    with pytest.raises(ValueError, match='det'):
        model.cell_relaxation(z, pos, torch.zeros_like(cell), batch)
    flipped = cell.clone()
    flipped[1, 0] *= -1.0
    with pytest.raises(ValueError, match='det'):
        model.cell_relaxation(z, pos, flipped, batch)
    with pytest.raises(ValueError, match='virial'):
        make_model(util.load_state('rand')).cell_relaxation(z, pos, cell, batch)
