"""fp64 statement of one nnhip_cell_lbfgs_step launch (csrc/cellrelax.hip) for ONE system, for the tests (numpy), with a first-order
rounding bound next to every output, in the manner of tests/relax_ref.py (whose two-loop part, constants and conventions it imports).

The launch has three stages, and the reference states each from the fp32 values the stage starts from, so that no error compounds:
  prologue   F = X[n:] / c, V = det(cell_in), FinvT = cof(F) / det(F), Wc = (W - p V I) FinvT then hydrostatic / mask / constant
             volume, G = [f F ; Wc / c], fmax.  From the launch's fp32 inputs; every operation of the kernel's chain (the header
             spells it out) is one `Val` operation below, which adds EPS32 |result| to the propagated operand bounds -- the 3x3
             inverse and determinant are bounded through their own operation chain, not through a condition number.
  chain      relax_ref.lbfgs_step on (X, G) over the n + 3 generalised rows, from the fp32 G the prologue STORED (the launch's G
             output) -- so y = fl32(G_prev - G) and S[head] = fl32(X_out - X) stay bitwise statements.
  epilogue   F' = X_out[n:] / c, cell_out = h0 F'^T, pos_out = q_out F'^T, from the fp32 X_out the chain stored.
`check_launch` compares a launch's outputs (the kernel's, or `emulate_launch`'s numpy-float32 ones) stage by stage: floats within
C_RX x bound + TINY32 + half an fp32 ulp, integers, flags, y and S[head] exact, everything untouched bitwise untouched.

Decisions (convergence, pair acceptance, clamp, the sign of det F) are reported AMBIGUOUS when the fp64 value lies within C_RX x its
bound of the threshold; the synthetic batch has none (tests/test_cellrelax_host.py shows it).

`minimise` is the method as a plain fp64 loop driven by a callback (the yardstick of the convergence tests)."""
import math

import numpy as np

from tests import relax_ref as rr

EPS32, C_RX, TINY32 = rr.EPS32, rr.C_RX, rr.TINY32
CHECK_ONLY, HYDROSTATIC, CONSTANT_VOLUME = 1, 2, 4
MASK_ALL = 63
VOIGT = np.array([[0, 5, 4], [5, 1, 3], [4, 3, 2]])
BAR = 1e5 * 1e-30 / 1.602176634e-19


def mask3x3(bits):
    return ((int(bits) >> VOIGT) & 1).astype(bool)


# ---- the method in plain fp64 (no bounds): what the kernel's chain must equal up to rounding ---------------------------------------

def project(Wc, bits=MASK_ALL, flags=0):
    """hydrostatic, mask, constant volume -- in this order"""
    Wc = np.array(Wc, dtype=np.float64)
    if flags & HYDROSTATIC:
        Wc = np.eye(3) * (np.trace(Wc) / 3.0)
    Wc = np.where(mask3x3(bits), Wc, 0.0)
    if flags & CONSTANT_VOLUME:
        Wc = Wc - np.eye(3) * (np.trace(Wc) / 3.0)
    return Wc


def generalised_forces(f, W, F, h, p, c, free=None, bits=MASK_ALL, flags=0):
    """G = [f F ; Wc / c] [n + 3, 3] in fp64:  Wc = project((W - p V I) F^-T),  V = det h;  fixed atoms: zero rows"""
    f, W, F, h = (np.asarray(a, dtype=np.float64) for a in (f, W, F, h))
    V = np.linalg.det(h)
    Wc = project((W - p * V * np.eye(3)) @ np.linalg.inv(F).T, bits, flags)
    return np.concatenate([rr.masked(f @ F, free), Wc / c])


def row_free(free, n):
    """the chain's view of `free` over the n + 3 generalised rows: the cell rows are always free"""
    fr = np.ones(n, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    return np.concatenate([fr, np.ones(3, dtype=bool)])


def minimise(energy_forces_virial, x0, h0, mol_ptr, fmax=0.01, memory=16, maxstep=0.2, alpha=70.0, max_steps=500, pressure=0.0,
             bits=MASK_ALL, flags=0, cell_factor=None, free=None):
    """The method as a plain fp64 loop.  energy_forces_virial(x [N,3], h [B,3,3]) -> (E [B], f [N,3], W [B,3,3]); pressure in
    eV / Angstrom^3, a number or [B]; every system keeps its own state; X stays fp64.  Returns dict(x, cell, F, energy, enthalpy,
    enthalpy_trace (per evaluation [steps+1, B]), volume_trace, fmax, converged, n_steps)."""
    x0, h0 = np.asarray(x0, dtype=np.float64), np.asarray(h0, dtype=np.float64)
    B = len(mol_ptr) - 1
    sl = [slice(int(mol_ptr[b]), int(mol_ptr[b + 1])) for b in range(B)]
    p = np.broadcast_to(np.asarray(pressure, dtype=np.float64), (B,))
    c = [float(cell_factor) if cell_factor is not None else float(max(s.stop - s.start, 1)) for s in sl]
    X = [np.concatenate([x0[s], c[b] * np.eye(3)]) for b, s in enumerate(sl)]
    states = [rr.new_state(s.stop - s.start + 3, memory) for s in sl]
    fr = [None if free is None else np.asarray(free, dtype=bool)[s] for s in sl]
    trace_h, trace_v = [], []
    for it in range(max_steps + 1):
        Fs = [Xb[-3:] / c[b] for b, Xb in enumerate(X)]
        x = np.concatenate([Xb[:-3] @ Fs[b].T for b, Xb in enumerate(X)]) if B else x0
        h = np.stack([h0[b] @ Fs[b].T for b in range(B)]) if B else h0
        E, f, W = (np.asarray(a, dtype=np.float64) for a in energy_forces_virial(x, h))
        V = np.linalg.det(h)
        trace_h.append(E + p * V)
        trace_v.append(V)
        fm = np.zeros(B)
        for b, s in enumerate(sl):
            n = s.stop - s.start
            G = generalised_forces(f[s], W[b], Fs[b], h[b], p[b], c[b], fr[b], bits, flags)
            r = rr.lbfgs_step(X[b], G, row_free(fr[b], n), states[b], fmax * fmax, alpha, maxstep,
                              rr.CHECK_ONLY if it == max_steps else 0, eps=0.0)
            X[b], states[b], fm[b] = r['x_out'], r['state'], r['fmax']
        if all(st['converged'] for st in states):
            break
    return dict(x=x, cell=h, F=np.stack(Fs) if B else np.zeros((0, 3, 3)), energy=E, enthalpy=trace_h[-1],
                enthalpy_trace=np.array(trace_h), volume_trace=np.array(trace_v), fmax=fm,
                converged=np.array([st['converged'] for st in states]), n_steps=np.array([st['n_steps'] for st in states]))


# ---- values with a first-order bound: one method = one fp32 operation of the kernel ------------------------------------------------

class Val:
    """an fp64 value (array) and the first-order bound of its fp32 counterpart"""
    __slots__ = ('v', 'b')

    def __init__(self, v, b=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.b = np.array(np.broadcast_to(np.asarray(b, dtype=np.float64), self.v.shape))

    def __getitem__(self, i):
        return Val(self.v[i], self.b[i])

    def __neg__(self):
        return Val(-self.v, self.b)


def _val(a):
    return a if isinstance(a, Val) else Val(a)


def _op(v, propagated, eps):
    return Val(v, propagated + eps * np.abs(v))


def mul(a, b, eps=EPS32):
    a, b = _val(a), _val(b)
    return _op(a.v * b.v, np.abs(a.v) * b.b + np.abs(b.v) * a.b, eps)


def add(a, b, eps=EPS32):
    a, b = _val(a), _val(b)
    return _op(a.v + b.v, a.b + b.b, eps)


def sub(a, b, eps=EPS32):
    return add(a, -_val(b), eps)


def div(a, b, eps=EPS32):
    a, b = _val(a), _val(b)
    q = a.v / b.v
    return _op(q, a.b / np.abs(b.v) + np.abs(q) * b.b / np.abs(b.v), eps)


def fma(a, b, c, eps=EPS32):
    a, b, c = _val(a), _val(b), _val(c)
    return _op(a.v * b.v + c.v, np.abs(a.v) * b.b + np.abs(b.v) * a.b + c.b, eps)


def dot3(a, b, eps=EPS32):
    """fma(a2, b2, fma(a1, b1, a0 b0)) along the last axis"""
    a, b = _val(a), _val(b)
    return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], mul(a[..., 0], b[..., 0], eps), eps), eps)


def stack(vals, shape=None):
    v, b = np.stack([x.v for x in vals]), np.stack([x.b for x in vals])
    return Val(v.reshape(shape), b.reshape(shape)) if shape else Val(v, b)


def cross3(u, v, eps=EPS32):
    return stack([fma(u[i], v[j], -mul(u[j], v[i], eps), eps) for i, j in ((1, 2), (2, 0), (0, 1))])


def cof3(A, eps=EPS32):
    """the cofactor matrix (rows A1 x A2, A2 x A0, A0 x A1) and the determinant dot3(A0, C0)"""
    C = stack([cross3(A[1], A[2], eps), cross3(A[2], A[0], eps), cross3(A[0], A[1], eps)])
    return C, dot3(A[0], C[0], eps)


def _trace_third(Wc, eps):
    return div(add(add(Wc[0, 0], Wc[1, 1], eps), Wc[2, 2], eps), 3.0, eps)


def prologue(Xc, f, W, cell_in, free, p, c, bits=MASK_ALL, flags=0, eps=EPS32):
    """The prologue for one system.  Xc [3,3]: the cell rows of x_in; f [n,3]; W, cell_in [3,3]; p, c: the fp32 values.  Returns
    dict(skip (det F <= 0 or something not finite), F, V, detF, G (Val [n + 3, 3]), fmax2, b_fmax2, fmax, b_fmax, ambiguous_det)."""
    f = np.asarray(f, dtype=np.float64)
    n = f.shape[0]
    with np.errstate(all='ignore'):
        F = div(Val(Xc), float(c), eps)
        _, V = cof3(Val(cell_in), eps)
        C, detF = cof3(F, eps)
    out = dict(F=F, V=V, detF=detF, ambiguous_det=bool(abs(detF.v) <= C_RX * detF.b))
    ok = np.isfinite(F.v).all() and np.isfinite(detF.v) and np.isfinite(V.v) and detF.v > 0 and np.isfinite(c) and c > 0 and np.isfinite(p)
    out['skip'] = not ok
    if not ok:
        return out
    FinvT = div(C, detF, eps)
    pv = mul(float(p), V, eps)
    Wp = Val(W)
    Wp = Val(Wp.v.copy(), Wp.b.copy())
    for i in range(3):
        d = sub(Wp[i, i], pv, eps)
        Wp.v[i, i], Wp.b[i, i] = d.v, d.b
    Wc = stack([fma(Wp[i, 2], FinvT[2, j], fma(Wp[i, 1], FinvT[1, j], mul(Wp[i, 0], FinvT[0, j], eps), eps), eps)
                for i in range(3) for j in range(3)], (3, 3))
    if flags & HYDROSTATIC:
        t = _trace_third(Wc, eps)
        Wc = Val(np.eye(3) * t.v, np.eye(3) * t.b)
    m = mask3x3(bits)
    Wc = Val(np.where(m, Wc.v, 0.0), np.where(m, Wc.b, 0.0))
    if flags & CONSTANT_VOLUME:
        t = _trace_third(Wc, eps)
        v, b = Wc.v.copy(), Wc.b.copy()
        for i in range(3):
            d = sub(Wc[i, i], t, eps)
            v[i, i], b[i, i] = d.v, d.b
        Wc = Val(v, b)
    Gc = div(Wc, float(c), eps)
    if n:
        Ga = stack([fma(f[:, 2], F[2, j], fma(f[:, 1], F[1, j], mul(f[:, 0], F[0, j], eps), eps), eps) for j in range(3)])
        Ga = Val(Ga.v.T, Ga.b.T)
        if free is not None:
            fr = np.asarray(free, dtype=bool)[:, None]
            Ga = Val(np.where(fr, Ga.v, 0.0), np.where(fr, Ga.b, 0.0))
        G = Val(np.concatenate([Ga.v, Gc.v]), np.concatenate([Ga.b, Gc.b]))
    else:
        G = Gc
    n2 = dot3(G, G, eps)
    k = int(np.argmax(n2.v))
    fmax2, b_fmax2 = float(n2.v[k]), float(n2.b.max())
    fmax = math.sqrt(fmax2)
    b_fmax = (b_fmax2 / (2.0 * fmax) if fmax > 0 else math.sqrt(b_fmax2)) + eps * fmax
    out.update(G=G, fmax2=fmax2, b_fmax2=b_fmax2, fmax=fmax, b_fmax=b_fmax)
    return out


def epilogue(X_out, h0, c, eps=EPS32):
    """cell_out and pos_out (Val) from the stored fp32 X_out [n + 3, 3]"""
    X_out = np.asarray(X_out, dtype=np.float64)
    Fn = div(Val(X_out[-3:]), float(c), eps)
    h0 = np.asarray(h0, dtype=np.float64)
    cell = stack([dot3(Val(h0[i]), Fn[j], eps) for i in range(3) for j in range(3)], (3, 3))
    q = X_out[:-3]
    if q.shape[0]:
        pos = stack([dot3(Val(q), Fn[j], eps) for j in range(3)])
        pos = Val(pos.v.T, pos.b.T)
    else:
        pos = Val(np.zeros((0, 3)))
    return cell, pos


def out_bound(val):
    """the bound a stored fp32 output is held to: C_RX x first order + TINY32 + half an ulp of the stored value"""
    return C_RX * val.b + TINY32 + rr.half_ulp32(val.v)


# ---- numpy float32 emulation of the whole launch, operation for operation ----------------------------------------------------------

def _f32_cross(u, v):
    f32 = np.float32
    return np.array([rr._fma32(u[i], v[j], -f32(u[j] * v[i])) for i, j in ((1, 2), (2, 0), (0, 1))], dtype=f32)


def _f32_dot3(a, b):
    return rr._fma32(a[2], b[2], rr._fma32(a[1], b[1], np.float32(a[0] * b[0])))


def _f32_cof(A):
    C = np.stack([_f32_cross(A[1], A[2]), _f32_cross(A[2], A[0]), _f32_cross(A[0], A[1])])
    return C, np.float32(_f32_dot3(A[0], C[0]))


def emulate_system(X, pos, f, W, cell_in, h0, free, p, c, st, tol2, alpha, maxstep, bits=MASK_ALL, flags=0):
    """one launch for one system in float32 arithmetic in the kernel's order.  Returns dict(skip, frozen, fmax, G, x_out, pos_out,
    cell_out, state) with float32 arrays (G None unless the system stepped)."""
    f32 = np.float32
    X, f, W, cell_in, h0 = (np.asarray(a, dtype=f32) for a in (X, f, W, cell_in, h0))
    n = f.shape[0]
    p, c = f32(p), f32(c)
    with np.errstate(all='ignore'):
        F = (X[n:] / c).astype(f32)
        _, V = _f32_cof(cell_in)
        C, detF = _f32_cof(F)
    if not (detF > 0 and np.isfinite(detF) and np.isfinite(V) and np.isfinite(F).all() and c > 0 and np.isfinite(c) and np.isfinite(p)):
        return dict(skip=True)
    FinvT = (C / detF).astype(f32)
    pv = f32(p * V)
    Wp = W.copy()
    for i in range(3):
        Wp[i, i] = f32(W[i, i] - pv)
    Wc = np.array([[rr._fma32(Wp[i, 2], FinvT[2, j], rr._fma32(Wp[i, 1], FinvT[1, j], f32(Wp[i, 0] * FinvT[0, j])))
                    for j in range(3)] for i in range(3)], dtype=f32)

    def third(A):
        return f32(f32(f32(A[0, 0] + A[1, 1]) + A[2, 2]) / f32(3.0))
    if flags & HYDROSTATIC:
        Wc = (np.eye(3, dtype=f32) * third(Wc)).astype(f32)
    Wc = np.where(mask3x3(bits), Wc, f32(0))
    if flags & CONSTANT_VOLUME:
        t = third(Wc)
        for i in range(3):
            Wc[i, i] = f32(Wc[i, i] - t)
    Gc = (Wc / c).astype(f32)
    Ga = np.stack([rr._fma32(f[:, 2], F[2, j], rr._fma32(f[:, 1], F[1, j], (f[:, 0] * F[0, j]).astype(f32))) for j in range(3)],
                  axis=1).astype(f32) if n else np.zeros((0, 3), f32)
    if free is not None and n:
        Ga = np.where(np.asarray(free, dtype=bool)[:, None], Ga, f32(0))
    G = np.concatenate([Ga, Gc]).astype(f32)
    fmax2 = rr._dot3_32(G, G).max()
    fmax = np.sqrt(fmax2, dtype=f32)
    now = bool(fmax2 < f32(tol2))
    if st['converged'] or now or (flags & CHECK_ONLY):
        new = rr.copy_state(st)
        new['converged'] = bool(st['converged'] or now)
        return dict(skip=False, frozen=True, fmax=fmax, G=None, x_out=X.copy(), pos_out=np.asarray(pos, dtype=f32).copy(),
                    cell_out=cell_in.copy(), state=new)
    # (tol2 = 0: the chain's own convergence test can never fire; the decision was taken above)
    x_out, _, new = rr.emulate_step(X, G, row_free(free, n), st, 0.0, alpha, maxstep, 0)
    Fn = (x_out[n:] / c).astype(f32)
    cell_out = np.array([[_f32_dot3(h0[i], Fn[j]) for j in range(3)] for i in range(3)], dtype=f32)
    q = x_out[:n]
    pos_out = np.stack([rr._fma32(q[:, 2], Fn[j, 2], rr._fma32(q[:, 1], Fn[j, 1], (q[:, 0] * Fn[j, 0]).astype(f32)))
                        for j in range(3)], axis=1).astype(f32) if n else np.zeros((0, 3), f32)
    return dict(skip=False, frozen=False, fmax=fmax, G=G, x_out=x_out, pos_out=pos_out, cell_out=cell_out, state=new)


# ---- batches in the kernel's layout -----------------------------------------------------------------------------------------------

INTS = ('converged', 'n_steps', 'n_pairs', 'head')
SENT = 777.0


def rows_of(d, b):
    """(first row, first cell row, end row) of system b among the generalised rows"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    return a0 + 3 * b, a1 + 3 * b, a1 + 3 * b + 3


def batch_state(d, b):
    r0, _, r1 = rows_of(d, b)
    m = d['S'].shape[0]
    return dict(converged=bool(d['converged'][b]), n_steps=int(d['n_steps'][b]), n_pairs=int(d['n_pairs'][b]), head=int(d['head'][b]),
                S=d['S'][:, r0:r1].astype(np.float64), Y=d['Y'][:, r0:r1].astype(np.float64), rho=d['rho'][b].astype(np.float64),
                b_rho=np.zeros(m), f_prev=d['g_prev'][r0:r1].astype(np.float64))


def slice_batch(d, b):
    """system b of a batch as a batch of its own"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    r0, _, r1 = rows_of(d, b)
    out = dict(d, ptr=np.array([0, a1 - a0], dtype=np.int32), kinds=[d['kinds'][b]])
    for k in ('pos', 'f', 'free'):
        out[k] = d[k][a0:a1]
    for k in ('X', 'g_prev'):
        out[k] = d[k][r0:r1]
    for k in ('S', 'Y'):
        out[k] = np.ascontiguousarray(d[k][:, r0:r1])
    for k in ('rho', 'W', 'cell', 'h0', 'p', 'c') + INTS:
        out[k] = d[k][b:b + 1]
    return out


def emulate_launch(d, bits=MASK_ALL, flags=0):
    """emulate_system over a batch, with the outputs laid out (and sentinel-filled) as the GPU test's launch leaves them"""
    f32 = np.float32
    out = {k: d[k].copy() for k in ('S', 'Y', 'rho', 'g_prev') + INTS}
    R, N, B = d['X'].shape[0], d['pos'].shape[0], len(d['ptr']) - 1
    out.update(G=np.full((R, 3), SENT, f32), x_out=np.full((R, 3), SENT, f32), pos_out=np.full((N, 3), SENT, f32),
               cell_out=np.full((B, 3, 3), SENT, f32), fmax=np.full(B, SENT, f32))
    for b in range(B):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        r0, rc, r1 = rows_of(d, b)
        r = emulate_system(d['X'][r0:r1], d['pos'][a0:a1], d['f'][a0:a1], d['W'][b], d['cell'][b], d['h0'][b], d['free'][a0:a1],
                           d['p'][b], d['c'][b], batch_state(d, b), d['tol2'], d['alpha'], d['maxstep'], bits, flags)
        if r['skip']:
            out['fmax'][b] = np.nan
            continue
        out['fmax'][b] = r['fmax']
        out['x_out'][r0:r1], out['pos_out'][a0:a1], out['cell_out'][b] = r['x_out'], r['pos_out'], r['cell_out']
        st = r['state']
        out['converged'][b] = int(st['converged'])
        if r['frozen']:
            continue
        out['G'][r0:r1] = r['G']
        out['S'][:, r0:r1], out['Y'][:, r0:r1], out['rho'][b] = st['S'].astype(f32), st['Y'].astype(f32), st['rho'].astype(f32)
        out['g_prev'][r0:r1] = st['f_prev'].astype(f32)
        out['n_steps'][b], out['n_pairs'][b], out['head'][b] = st['n_steps'], st['n_pairs'], st['head']
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_sent(a):
    return bool(np.all(a == np.float32(SENT)))


def check_launch(d, out, bits=MASK_ALL, flags=0):
    """Assert that `out` (arrays named as emulate_launch's: the state after the launch and G, x_out, pos_out, cell_out, fmax, written
    over SENT) is what one launch on the batch `d` must leave.  Returns (worst err / bound per output, the set of branches seen:
    (kind, outcome, accepted, clamped, clamp decided by a cell row), the list of ambiguous decisions)."""
    worst = dict(fmax=0.0, G=0.0, x=0.0, rho=0.0, cell=0.0, pos=0.0)
    seen, ambiguous = set(), []
    m = d['S'].shape[0]

    def within(name, got, val, what):
        err, bound = np.abs(np.asarray(got, dtype=np.float64) - val.v), out_bound(val)
        ratio = float((err / bound).max()) if err.size else 0.0
        assert np.all(err <= bound), f'{what}: {name} err / bound {ratio:.3f}'
        worst[name] = max(worst[name], ratio)

    for b, kind in enumerate(d['kinds']):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        r0, rc, r1 = rows_of(d, b)
        n = a1 - a0
        what = f'system {b} ({kind}, {n} atoms, bits {bits}, flags {flags})'
        st = batch_state(d, b)
        pro = prologue(d['X'][rc:r1], d['f'][a0:a1], d['W'][b], d['cell'][b], d['free'][a0:a1], d['p'][b], d['c'][b], bits, flags)
        if pro['ambiguous_det']:
            ambiguous.append((b, kind, 'det'))
        state_same = (all(_same_bits(out[k][:, r0:r1], d[k][:, r0:r1]) for k in ('S', 'Y')) and _same_bits(out['rho'][b], d['rho'][b])
                      and _same_bits(out['g_prev'][r0:r1], d['g_prev'][r0:r1]) and _all_sent(out['G'][r0:r1])
                      and all(int(out[k][b]) == int(d[k][b]) for k in INTS[1:]))
        if pro['skip']:
            assert np.isnan(out['fmax'][b]), f'{what}: a skipped system has fmax {out["fmax"][b]}'
            assert state_same and int(out['converged'][b]) == int(d['converged'][b]), f'{what}: a skipped system was touched'
            assert _all_sent(out['x_out'][r0:r1]) and _all_sent(out['pos_out'][a0:a1]) and _all_sent(out['cell_out'][b]), what
            seen.add((kind, 'skip', None, False, False))
            continue
        within('fmax', out['fmax'][b], Val(pro['fmax'], pro['b_fmax']), what)
        now = pro['fmax2'] < d['tol2']
        if not st['converged'] and abs(pro['fmax2'] - d['tol2']) <= C_RX * pro['b_fmax2']:
            ambiguous.append((b, kind, 'converge'))
        if st['converged'] or now or (flags & CHECK_ONLY):
            assert int(out['converged'][b]) == int(st['converged'] or now), f'{what}: converged flag'
            assert state_same, f'{what}: a frozen system\'s state was touched'
            assert _same_bits(out['x_out'][r0:r1], d['X'][r0:r1]) and _same_bits(out['pos_out'][a0:a1], d['pos'][a0:a1]) \
                and _same_bits(out['cell_out'][b], d['cell'][b]), f'{what}: a frozen system is not copied bitwise'
            seen.add((kind, 'frozen', None, False, False))
            continue
        assert int(out['converged'][b]) == 0, f'{what}: converged flag'
        # ---- the prologue's G, then the chain from the stored G
        G32 = out['G'][r0:r1]
        within('G', G32, pro['G'], what)
        free = d['free'][a0:a1]
        assert not G32[:n][~free].any(), f'{what}: a fixed atom has a generalised force'
        ref = rr.lbfgs_step(d['X'][r0:r1], G32, row_free(free, n), st, d['tol2'], d['alpha'], d['maxstep'], 0, converge=False)
        for k, a in ref['ambiguous'].items():
            if a and k != 'converge':
                ambiguous.append((b, kind, k))
        new = ref['state']
        for k in INTS[1:]:
            assert int(out[k][b]) == int(new[k]), f'{what}: {k} {out[k][b]} != {int(new[k])}'
        X, Xo = d['X'][r0:r1], out['x_out'][r0:r1]
        err, bx = np.abs(Xo.astype(np.float64) - ref['x_out']), ref['bx'] + rr.half_ulp32(ref['x_out'])
        assert np.all(err <= bx), f'{what}: x_out err / bound {float((err / np.maximum(bx, 1e-300)).max()):.3f}'
        worst['x'] = max(worst['x'], float((err[bx > 0] / bx[bx > 0]).max()) if (bx > 0).any() else 0.0)
        assert _same_bits(Xo[:n][~free], X[:n][~free]), f'{what}: the reference-frame position of a fixed atom moved'
        S1, Y1, rho1 = out['S'][:, r0:r1], out['Y'][:, r0:r1], out['rho'][b]
        S0, Y0, rho0 = d['S'][:, r0:r1], d['Y'][:, r0:r1], d['rho'][b]
        h_old, h_new = st['head'], new['head']
        assert _same_bits(S1[h_new], rr.stored_s(Xo, X).astype(np.float32)), f'{what}: S[head] is not fl32(x_out - x_in)'
        assert _same_bits(out['g_prev'][r0:r1], G32), f'{what}: g_prev is not G'
        for k in range(m):
            if k != h_new:
                assert _same_bits(S1[k], S0[k]), f'{what}: S[{k}] touched'
            if not (ref['accepted'] and k == h_old):
                assert _same_bits(Y1[k], Y0[k]) and _same_bits(rho1[k], rho0[k]), f'{what}: Y / rho [{k}] touched'
        if ref['accepted']:
            assert _same_bits(Y1[h_old], rr.pair_y(d['g_prev'][r0:r1], G32).astype(np.float32)), f'{what}: Y[head] is not fl32(g_prev - G)'
            e, bound = abs(float(rho1[h_old]) - new['rho'][h_old]), ref['b_rho_new'] + rr.half_ulp32(new['rho'][h_old])
            assert e <= bound, f'{what}: rho err / bound {e / bound:.3f}'
            worst['rho'] = max(worst['rho'], e / bound)
        # ---- the epilogue from the stored x_out
        cell, pos = epilogue(Xo, d['h0'][b], d['c'][b])
        within('cell', out['cell_out'][b], cell, what)
        within('pos', out['pos_out'][a0:a1], pos, what)
        step2 = ((ref['x_out'] - X.astype(np.float64)) ** 2).sum(1)
        seen.add((kind, 'step', ref['accepted'], ref['clamped'], bool(np.argmax(step2) >= n)))
    return worst, seen, ambiguous


# ---- synthetic kernel inputs: every branch of a launch at every size class (shared by the host and the GPU tests) -----------------

SYN_SIZES = (0, 1, 2, 21, 61, 62, 200)        # 61 and 62 atoms: 64 and 65 rows, the last register and the first scratch work vector
SYN_MEMORY = 4
SYN_TOL2, SYN_ALPHA, SYN_MAXSTEP = rr.SYN_TOL2, rr.SYN_ALPHA, rr.SYN_MAXSTEP
# (pairs stored, kind).  accept / reject_neg / reject_cos / first / converged / converging: as relax_ref.SYN_VARIANTS, on the generalised
# rows;  det_neg: F with a negative determinant (skipped)
SYN_VARIANTS = ((0, 'first'), (0, 'accept'), (1, 'accept'), (SYN_MEMORY - 1, 'accept'), (SYN_MEMORY, 'accept'),
                (SYN_MEMORY, 'reject_neg'), (SYN_MEMORY - 1, 'reject_cos'), (2, 'reject_neg'), (2, 'converged'), (1, 'converging'),
                (1, 'det_neg'))
# (forces, virial per cell_factor) scales, eV / A: no clamp; the clamp decided by an atom row; by a cell row
SYN_LOADS = (('small', 0.5, 0.5), ('atoms', 30.0, 0.5), ('cell', 0.5, 150.0))
SYN_OPTIONS = ((MASK_ALL, 0), (0b100011, 0), (MASK_ALL, HYDROSTATIC), (MASK_ALL, CONSTANT_VOLUME))      # (strain_mask, flags)


def synthetic_batch(seed=0):
    """The batch of the kernel test: for every size of SYN_SIZES every variant of SYN_VARIANTS under every load of SYN_LOADS.
    Systems alternate between a triclinic and an orthorhombic h0, F = I and F away from I (every third F = I exactly), zero and
    non-zero pressure (+-2e-3 eV / A^3, about 3 kbar), cell_factor = the atom count and 3.5, and (from 2 atoms) a quarter of the
    atoms fixed.  Stored pairs are y = A s with a random SPD A over the generalised rows (fixed atoms: zero rows), heads are placed
    so that rings wrap, unused slots hold 7.0 (S, Y) and 0.5 (rho).  The pending pair is built on the generalised forces of the
    options (all components, no flags); other options change the cell rows of G and with them y, which the reference follows.
    Returns a dict of numpy arrays in the kernel's layout and types, plus kinds / loads (per system)."""
    rng = np.random.default_rng(seed)
    f32, m = np.float32, SYN_MEMORY
    systems = []
    count = 0
    for n in SYN_SIZES:
        for pairs, kind in SYN_VARIANTS:
            for load, f_scale, w_scale in SYN_LOADS:
                count += 1
                free = np.ones(n, dtype=bool)
                if n >= 2 and count % 2:
                    free = rng.random(n) >= 0.25
                    free[rng.integers(n)] = True
                fr_rows = row_free(free, n)
                mask = np.repeat(fr_rows, 3)
                d = 3 * (n + 3)
                c = f32(3.5) if count % 4 == 0 else f32(max(n, 1))
                p = f32((0.0, 2e-3, 0.0, -2e-3)[count % 4]) if count % 5 else f32(1e-3)
                h0 = np.diag(rng.uniform(7.0, 12.0, 3))
                if count % 2 == 0:
                    h0 = h0 + np.tril(rng.normal(0, 1.5, (3, 3)), -1)
                    h0 = h0 @ np.linalg.qr(rng.standard_normal((3, 3)))[0]
                    if np.linalg.det(h0) < 0:
                        h0[2] = -h0[2]
                h0 = h0.astype(f32)
                F = np.eye(3) if count % 3 == 0 else np.eye(3) + rng.normal(0, 0.05, (3, 3))
                if kind == 'det_neg':
                    F = F @ np.diag([1.0, 1.0, -1.0])
                q = rng.uniform(-8, 8, (n, 3))
                X = np.concatenate([q, float(c) * F]).astype(f32)
                F32 = X[n:].astype(np.float64) / float(c)
                cell = (h0.astype(np.float64) @ F32.T).astype(f32)
                pos = (X[:n].astype(np.float64) @ F32.T).astype(f32)
                f = rng.normal(0, f_scale, (n, 3)).astype(f32)
                W = (rng.normal(0, w_scale * float(c), (3, 3))).astype(f32)
                W = ((W + W.T) / 2).astype(f32)
                G = None
                if kind != 'det_neg':
                    G = generalised_forces(f, W, F32, cell, float(p), float(c), free)
                    if kind == 'converging':         # the largest row 0.003: below fmax = 0.01 under every option (constant volume < 2 x)
                        s = 0.003 / np.sqrt((G ** 2).sum(1).max())
                        pv = float(p) * np.linalg.det(cell.astype(np.float64))
                        f = (f.astype(np.float64) * s).astype(f32)
                        W = ((W.astype(np.float64) - pv * np.eye(3)) * s + pv * np.eye(3)).astype(f32)
                        G = generalised_forces(f, W, F32, cell, float(p), float(c), free)
                A = rr._spd(rng, d) * np.outer(mask, mask)
                head = {0: 0, 1: 1, 2: m - 1, m - 1: m - 1, m: 2}[pairs] if kind != 'first' else 0
                S, Y, rho = np.full((m, n + 3, 3), 7.0, dtype=f32), np.full((m, n + 3, 3), 7.0, dtype=f32), np.full(m, 0.5, dtype=f32)
                for k in rr.pair_slots(head, min(pairs, m - 1 if kind != 'first' else m), m):
                    s = (rng.normal(0, 0.05, d) * mask).astype(f32)
                    y = (A @ s.astype(np.float64)).astype(f32)
                    S[k], Y[k] = s.reshape(n + 3, 3), y.reshape(n + 3, 3)
                    rho[k] = f32(1.0 / float(y.astype(np.float64) @ s.astype(np.float64)))
                g_prev = np.full((n + 3, 3), 7.0, dtype=f32)
                n_steps = 0
                if kind != 'first':
                    n_steps = pairs + 3
                    s = (rng.normal(0, 0.05, d) * mask).astype(f32)
                    s64 = s.astype(np.float64)
                    if kind == 'reject_cos':
                        v = rng.normal(0, 1.0, d) * mask
                        v -= (v @ s64) / (s64 @ s64) * s64
                        y = 5.0 * (v / np.linalg.norm(v) + 2e-5 * s64 / np.linalg.norm(s64))
                    else:
                        y = A @ s64 * (-1.0 if kind == 'reject_neg' else 1.0)
                    S[head] = s.reshape(n + 3, 3)
                    if G is not None:
                        g_prev = (G + y.reshape(n + 3, 3)).astype(f32)
                systems.append(dict(n=n, kind=kind, load=load, free=free, X=X, pos=pos, f=f, W=W, cell=cell, h0=h0, p=p, c=c, S=S,
                                    Y=Y, rho=rho, g_prev=g_prev, converged=int(kind == 'converged'), n_steps=n_steps,
                                    n_pairs=pairs if kind != 'first' else 0, head=head))
    out = dict(ptr=np.concatenate([[0], np.cumsum([s['n'] for s in systems])]).astype(np.int32),
               kinds=[s['kind'] for s in systems], loads=[s['load'] for s in systems], memory=m, tol2=SYN_TOL2, alpha=SYN_ALPHA,
               maxstep=SYN_MAXSTEP)
    for k in ('X', 'pos', 'f', 'g_prev', 'free'):
        out[k] = np.concatenate([s[k] for s in systems])
    for k in ('S', 'Y'):
        out[k] = np.ascontiguousarray(np.concatenate([s[k] for s in systems], axis=1))
    for k in ('rho', 'W', 'cell', 'h0'):
        out[k] = np.stack([s[k] for s in systems])
    for k in ('p', 'c'):
        out[k] = np.array([s[k] for s in systems], dtype=f32)
    for k in INTS:
        out[k] = np.array([s[k] for s in systems], dtype=np.int32)
    return out


# ---- the analytic crystal of the convergence tests ---------------------------------------------------------------------------------

def crystal(seed=0, n_sys=8):
    """n_sys systems of 8 .. 40 atoms with  E = (V0 K / 2) |eps_G - eps0|^2 + (k / 2) sum |q_i - q_i0|^2,  eps_G = (F^T F - I) / 2
    the Green-Lagrange strain of the deformation gradient F (h = h0 F^T) and q = x F^-T the reference-frame positions: the minimum
    at zero pressure has F^T F = I + 2 eps0 and q = q0.  Each system has its own symmetric eps0 (entries up to 0.03); the last has
    a non-zero pressure.  K = 1.5 eV / A^3 (about 240 GPa), k = 5 eV / A^2."""
    rng = np.random.default_rng(seed)
    sizes = np.linspace(8, 40, n_sys).astype(int)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    h0 = np.stack([np.diag(rng.uniform(5.0, 8.0, 3)) + np.tril(rng.normal(0, 0.8, (3, 3)), -1) for _ in sizes])
    eps0 = rng.uniform(-0.03, 0.03, (n_sys, 3, 3))
    eps0 = np.triu(eps0) + np.triu(eps0, 1).transpose(0, 2, 1)
    q0 = np.concatenate([rng.uniform(0, 1, (n, 3)) @ h0[b] for b, n in enumerate(sizes)])
    x0 = q0 + rng.normal(0, 0.05, q0.shape)
    p = np.zeros(n_sys)
    p[-1] = 0.02
    return dict(ptr=ptr, h0=h0.astype(np.float32), eps0=eps0, q0=q0, x0=x0.astype(np.float32), p=p, K=1.5, k=5.0,
                V0=np.linalg.det(h0.astype(np.float32).astype(np.float64)))


def crystal_tensors(cr, device, dtype):
    """the crystal's constants as torch tensors for crystal_efv_torch"""
    import torch
    t = {k: torch.as_tensor(np.asarray(cr[k], dtype=np.float64), dtype=dtype, device=device) for k in ('h0', 'eps0', 'q0', 'V0')}
    t['h0_inv'] = torch.linalg.inv(torch.as_tensor(cr['h0'].astype(np.float64), device=device)).to(dtype)
    t['batch'] = torch.as_tensor(np.repeat(np.arange(len(cr['ptr']) - 1), np.diff(cr['ptr'])), device=device)
    t['K'], t['k'] = cr['K'], cr['k']
    return t


def crystal_efv_torch(t, x, h):
    """crystal_efv in torch, batched, in the dtype and on the device of its arguments (t: crystal_tensors)"""
    import torch
    F = (t['h0_inv'] @ h).transpose(1, 2)
    Finv = torch.linalg.inv(F)
    bt = t['batch']
    dq = (x[:, None, :] @ Finv[bt].transpose(1, 2))[:, 0, :] - t['q0']
    strain = (F.transpose(1, 2) @ F - torch.eye(3, dtype=x.dtype, device=x.device)) / 2.0 - t['eps0']
    A = t['K'] * t['V0'][:, None, None] * strain
    E = 0.5 * (A * strain).sum((1, 2))
    E = E.index_add(0, bt, 0.5 * t['k'] * (dq * dq).sum(1))
    f = -t['k'] * (dq[:, None, :] @ Finv[bt])[:, 0, :]
    W = -(F @ A @ F.transpose(1, 2))
    return E, f, W


def crystal_efv(cr, x, h):
    """(E [B], f [N,3], W [B,3,3]) of the analytic crystal at Cartesian positions x and cells h, fp64, closed form:
    with A = K V0 (eps_G - eps0):  dE/dF = F A - sum_i k x_i (q_i - q_i0)^T ... the virial is  W = -(dE/dF) F^T  at fixed q, i.e.
    W = -F A F^T  (the position term moves with the cell: x = q F^T at fixed q carries no strain energy), f = -k (q - q0) F^-1."""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    B = len(cr['ptr']) - 1
    E, f, W = np.zeros(B), np.zeros_like(x), np.zeros((B, 3, 3))
    for b in range(B):
        s = slice(int(cr['ptr'][b]), int(cr['ptr'][b + 1]))
        F = np.linalg.solve(cr['h0'][b].astype(np.float64), h[b]).T          # h = h0 F^T
        Finv = np.linalg.inv(F)
        q = x[s] @ Finv.T
        dq = q - cr['q0'][s]
        A = cr['K'] * cr['V0'][b] * ((F.T @ F - np.eye(3)) / 2.0 - cr['eps0'][b])
        E[b] = 0.5 * (A * ((F.T @ F - np.eye(3)) / 2.0 - cr['eps0'][b])).sum() + 0.5 * cr['k'] * (dq ** 2).sum()
        f[s] = -cr['k'] * dq @ Finv
        W[b] = -F @ A @ F.T
    return E, f, W
