"""Statement of one nnhip_md_step_constrained launch (csrc/rattle.hip) for the tests (numpy): the same stage order, colour-ordered
Gauss-Seidel and molecule-relative coordinates, in two precisions.

`launch(..., fp32=False)` is the fp64 restatement: every operation in fp64 on the SAME fp32 inputs, the solves converged to the
`tol` it is given (the tests use 1e-13).  `launch(..., fp32=True)` is the fp32 EMULATION of the kernel's chain: every operation
rounded to fp32 once (an fma as fp32(fp64(a) fp64(b) + fp64(c)): the product is exact in fp64, the sum rounds twice, which differs
from a true fma in about one case in 2^29 -- the emulation is a yardstick, not a bitwise oracle).  Both vectorise a colour over all
molecules of the batch; a molecule leaves the sweeps as soon as one of its sweeps applied no update, as a wave does.

Bounds.
(1) Constraints as stored.  The solver ends with | d2 - fl(s.s) | <= fl(tol d2) on s = fl(y_i - y_j), in its own fp32 arithmetic,
and the test evaluates |r|^2 in fp64 on the STORED positions.  The two differ by, to first order,
      the stored coordinates:  x_out = fl(x_first + y), one rounding, |x_out - (x_first + y)| <= EPS32 |x_out|; a fixed atom is
                               stored as it came in while the solver saw fl(x - x_first): <= EPS32 |y|.  Both are covered by
                               e_ik = EPS32 (|x_ik| + |y_ik|), and |r|^2 moves by 2 sum_k |r_k| (e_ik + e_jk);
      the kernel's s.s:        s_k = fl(y_i - y_j) is one rounding (2 EPS32 r_k^2 in the square) and the three operations of the
                               dot product one each (<= EPS32 |r|^2 each): 5 EPS32 |r|^2 together.
  stored_bound = tol d2 + C_CON [2 sum_k |r_k| (e_ik + e_jk) + 5 EPS32 |r|^2];  C_CON = 2 stands for what first order leaves out
  (products of two roundings, the rounding of tol d2 itself), as C_MD = 2 does in md_ref.py: chosen before any run.
  The velocity form, |r.(v_i - v_j)| dth <= tol d2 in the kernel: stored velocities are the solver's own bits, so only the
  positions and the evaluation enter: tol d2 + C_CON dth [sum_k (e_ik + e_jk) |u_k| + 5 EPS32 sum_k |r_k u_k|], u = v_i - v_j.
(2) Against fp64.  A solve that stops at a residual of up to tol d2 per constraint (SHAKE) or tol d2 / dth (velocities) leaves
the state within the linearised response  M^-1 J^T (J M^-1 J^T)^-1 residual  of the converged one (J: the constraint Jacobian at
the fp64 solution, M^-1 = diag(w); absolute values taken entry by entry, computed here in fp64).  `launch` sums these over the
solves of the launch as they occur: a SHAKE response enters the positions and, divided by dth, the velocities; a velocity response
the velocities; every drift carries dth x the velocity sum into the positions.  That sum times MARGIN, plus the rounding bound of
the unconstrained chain (md_ref.md_step on the same inputs), the roundings inside the constrained chain (solver_rounding, derived
there) and half an ulp of the stored value, is the bound.
MARGIN cannot be derived: it is 4 x the worst ratio (err - everything but the sum) / sum of the fp32 EMULATION (not of the device
code) against the fp64 restatement over the inputs of tests/test_hip_rattle.py (`case`, the four flag values, with and without
noise), measured on the CPU by `python -m tests.rattle_ref`:
      worst emulation ratios   positions 0.00   velocities 0.704   kinetic energies 0.405      (EMULATION_RATIOS below)
(0.30 - 0.60 for a single velocity solve, FINISH or PROJECT: one solve stops anywhere below its tolerance.  With drifts the
derived rounding term is larger than the emulation's whole error, hence 0.00 for the positions: there the bound is carried by
solver_rounding, which is loose by its count of updates -- every sweep is taken to update every constraint.)
So MARGIN = 4 x 0.704 = 2.82."""
import numpy as np

from tests import md_ref as mr

EPS32 = mr.EPS32
FINISH, BEGIN, PROJECT = 1, 2, 4
GUARD = np.float32(0.1)
C_CON = 2.0
EMULATION_RATIOS = dict(x=0.0, v=0.704, ke=0.405)
MARGIN = 4.0 * max(EMULATION_RATIOS.values())
FS = 0.0982269
K_B = 8.617333262e-5


class _F64:
    dt = np.float64

    @staticmethod
    def c(a):
        return np.asarray(a, dtype=np.float64)
    fma = staticmethod(lambda a, b, c: a * b + c)
    mul = staticmethod(lambda a, b: a * b)
    add = staticmethod(lambda a, b: a + b)
    sub = staticmethod(lambda a, b: a - b)
    div = staticmethod(lambda a, b: a / b)


class _F32:
    dt = np.float32

    @staticmethod
    def c(a):
        return np.asarray(a, dtype=np.float32)

    @staticmethod
    def fma(a, b, c):
        return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
                + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)
    mul = staticmethod(lambda a, b: np.asarray(a, np.float32) * np.asarray(b, np.float32))
    add = staticmethod(lambda a, b: np.asarray(a, np.float32) + np.asarray(b, np.float32))
    sub = staticmethod(lambda a, b: np.asarray(a, np.float32) - np.asarray(b, np.float32))
    div = staticmethod(lambda a, b: np.asarray(a, np.float32) / np.asarray(b, np.float32))


def _dot3(o, a, b):
    return o.fma(a[:, 2], b[:, 2], o.fma(a[:, 1], b[:, 1], o.mul(a[:, 0], b[:, 0])))


class Tables:
    """The sorted constraints of a batch, as the reference walks them: global atom indices gi, gj [C], molecule mol [C], colour
    groups (the constraints of colour k of every molecule), d2 [C] (the fp32 values the kernel gets)"""

    def __init__(self, prep, d2, mol_ptr):
        mol_ptr = np.asarray(mol_ptr, dtype=np.int64)
        self.mol_ptr, self.n_mol = mol_ptr, mol_ptr.size - 1
        per = np.diff(prep.col_ptr.astype(np.int64)[prep.mol_col_ptr.astype(np.int64)])
        self.mol = np.repeat(np.arange(self.n_mol), per)
        self.gi = mol_ptr[self.mol] + prep.local[:, 0]
        self.gj = mol_ptr[self.mol] + prep.local[:, 1]
        self.d2 = np.asarray(d2, dtype=np.float32)
        self.has = per > 0
        self.groups = [np.flatnonzero(prep.colour == k) for k in range(int(prep.colour.max()) + 1 if prep.colour.size else 0)]
        self.batch = np.repeat(np.arange(self.n_mol), np.diff(mol_ptr))
        self.con_atom = self.has[self.batch] if self.batch.size else np.zeros(0, dtype=bool)


def _sweeps(o, T, tol, max_iter, body):
    """Gauss-Seidel in colour order; body(idx) applies colour-mates idx and returns (updated mask, failed mask) over them"""
    active = T.has.copy()
    sweeps, fail = np.zeros(T.n_mol, dtype=np.int64), np.zeros(T.n_mol, dtype=bool)
    it = 0
    while active.any() and it < max_iter:
        upd = np.zeros(T.n_mol, dtype=bool)
        for idx in T.groups:
            idx = idx[active[T.mol[idx]]]
            if idx.size:
                u, f = body(idx)
                upd[T.mol[idx[u]]] = True
                fail[T.mol[idx[f]]] = True
        it += 1
        sweeps[active] += 1
        active &= upd
    return sweeps, fail | active


def shake(o, T, y, r, w, tol, max_iter, disp):
    """every applied update is also added into disp [N,3] (zero on entry): the displacement of the solve"""
    tol = o.c(tol)

    def body(idx):
        i, j, d2 = T.gi[idx], T.gj[idx], o.c(T.d2[idx])
        s, q = o.sub(y[i], y[j]), o.sub(r[i], r[j])
        e = o.sub(d2, _dot3(o, s, s))
        need = np.abs(e) > o.mul(tol, d2)
        sr, ws = _dot3(o, s, q), o.add(w[i], w[j])
        ok = need & (sr > o.mul(o.c(GUARD), d2)) & (ws > 0)
        i, j, q = i[ok], j[ok], q[ok]
        gm = o.div(e[ok], o.mul(o.mul(o.c(2.0), ws[ok]), sr[ok]))
        gi, gj = o.mul(gm, w[i]), -o.mul(gm, w[j])
        y[i] = o.fma(gi[:, None], q, y[i])
        y[j] = o.fma(gj[:, None], q, y[j])
        disp[i] = o.fma(gi[:, None], q, disp[i])
        disp[j] = o.fma(gj[:, None], q, disp[j])
        return ok, need & ~ok
    return _sweeps(o, T, tol, max_iter, body)


def project(o, T, y, v, w, tol, dth, max_iter):
    tol, dth = o.c(tol), o.c(dth)

    def body(idx):
        i, j, d2 = T.gi[idx], T.gj[idx], o.c(T.d2[idx])
        q, u = o.sub(y[i], y[j]), o.sub(v[i], v[j])
        qu = _dot3(o, q, u)
        need = o.mul(np.abs(qu), dth) > o.mul(tol, d2)
        ws = o.add(w[i], w[j])
        ok = need & (ws > 0)
        i, j, q = i[ok], j[ok], q[ok]
        gm = o.div(qu[ok], o.mul(ws[ok], d2[ok]))
        gi, gj = -o.mul(gm, w[i]), o.mul(gm, w[j])
        v[i] = o.fma(gi[:, None], q, v[i])
        v[j] = o.fma(gj[:, None], q, v[j])
        return ok, need & ~ok
    return _sweeps(o, T, tol, max_iter, body)


def response(T, y, w, resid, jac_of_positions):
    """|M^-1 J^T (J M^-1 J^T)^-1| resid per coordinate [N,3], molecule by molecule, in fp64.  J row of constraint c: +p_c at atom
    i, -p_c at atom j, with p_c = 2 (y_i - y_j) for the position constraints (jac_of_positions) and y_i - y_j for the velocity
    ones; resid [C] >= 0"""
    out = np.zeros_like(y, dtype=np.float64)
    y, w = np.asarray(y, np.float64), np.asarray(w, np.float64)
    for b in np.flatnonzero(T.has):
        cs = np.flatnonzero(T.mol == b)
        a0, n = T.mol_ptr[b], T.mol_ptr[b + 1] - T.mol_ptr[b]
        J = np.zeros((cs.size, n, 3))
        p = (2.0 if jac_of_positions else 1.0) * (y[T.gi[cs]] - y[T.gj[cs]])
        J[np.arange(cs.size), T.gi[cs] - a0] = p
        J[np.arange(cs.size), T.gj[cs] - a0] = -p
        J = J.reshape(cs.size, 3 * n)
        WJt = np.repeat(w[a0:a0 + n], 3)[:, None] * J.T
        R = WJt @ np.linalg.pinv(J @ WJt)
        out[a0:a0 + n] = (np.abs(R) @ resid[cs]).reshape(n, 3)
    return out


def launch(flags, x, v, F, hk, mass, w, T, sigma=None, xi=None, c1=1.0, dth=0.0, inv_dth=0.0, tol=1e-13, max_iter=2000,
           fp32=False, bound_tol=None):
    """One launch on the fp32 inputs the kernel gets (x, v, F, xi [N,3]; hk, mass, w, sigma [N]; numbers already rounded to fp32).
    Returns dict(x (None with FINISH alone), v, ke (None without FINISH), n_sweeps [B], failed bool [B]) and, in fp64 with
    bound_tol (the kernel's tolerance), sx, sv, ske: the summed linearised responses of docstring (2) BEFORE MARGIN, and bx, bv,
    bke: the rounding bound of the unconstrained chain."""
    o = _F32 if fp32 else _F64
    x_in = o.c(x)
    v_in, v, w = o.c(v).copy(), o.c(v).copy(), o.c(w)
    F = None if F is None else o.c(F)
    hk = None if hk is None else o.c(hk)[:, None]
    dth_, inv_dth_, c1_ = o.c(dth), o.c(inv_dth), o.c(c1)
    N, B = x_in.shape[0], T.n_mol
    ca = T.con_atom
    x0 = x_in[T.mol_ptr[:-1][T.batch]] if N else x_in
    y = o.sub(x_in, x0)
    sweeps, failed = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool)
    want = bound_tol is not None and not fp32
    sx, sv = np.zeros((N, 3)), np.zeros((N, 3))
    d2 = T.d2.astype(np.float64)

    def do_project():
        nonlocal sweeps, failed, sv
        s, f = project(o, T, y, v, w, tol, dth_, max_iter)
        sweeps, failed = np.maximum(sweeps, s), failed | f
        if want:
            sv = sv + response(T, y, w, bound_tol * d2 / float(dth), False)

    def do_shake(r):
        nonlocal sweeps, failed, sx, sv
        disp = np.zeros_like(y)
        s, f = shake(o, T, y, r, w, tol, max_iter, disp)
        sweeps, failed = np.maximum(sweeps, s), failed | f
        if want:
            d = response(T, y, w, bound_tol * d2, True)
            sx = sx + float(dth) * sv + d
            sv = sv + d / float(dth)
        return disp

    ke = None
    if flags & PROJECT:
        do_shake(y.copy())
        do_project()
    if flags & FINISH:
        v[ca] = o.fma(hk[ca], F[ca], v[ca])
        do_project()
        vv = v
        ke = o.mul(o.mul(o.c(0.5), o.c(mass)), o.fma(vv[:, 2], vv[:, 2], o.fma(vv[:, 1], vv[:, 1], o.mul(vv[:, 0], vv[:, 0]))))
    if flags & BEGIN:
        v[ca] = o.fma(hk[ca], F[ca], v[ca])
        do_project()
        for half in (0, 1):
            if half == 1 and xi is not None:
                v[ca] = o.fma(o.c(sigma)[ca, None], o.c(xi)[ca], o.mul(c1_, v[ca]))
                do_project()
            r = y.copy()
            y[ca] = o.fma(dth_, v[ca], r[ca])
            disp = do_shake(r)
            v[ca] = o.fma(disp[ca], inv_dth_, v[ca])
            do_project()
    moved = bool(flags & (BEGIN | PROJECT))
    x_out = None
    if moved:
        x_out = np.where(((w == 0) | ~ca)[:, None], x_in, o.add(x0, y))
    # the molecules without constraints: nnhip_md_step's chain (PROJECT: nothing moves)
    out = dict(bx=None, bv=np.zeros((N, 3)), bke=None)
    if not flags & PROJECT:
        if fp32:
            u = ~ca
            if flags & FINISH:
                v[u] = o.fma(hk[u], F[u], v[u])
                ke[u] = o.mul(o.mul(o.c(0.5), o.c(mass)[u]), o.fma(v[u, 2], v[u, 2], o.fma(v[u, 1], v[u, 1], o.mul(v[u, 0], v[u, 0]))))
            if flags & BEGIN:
                v[u] = o.fma(hk[u], F[u], v[u])
                xx = o.fma(dth_, v[u], x_in[u])
                if xi is not None:
                    v[u] = o.fma(o.c(sigma)[u, None], o.c(xi)[u], o.mul(c1_, v[u]))
                x_out[u] = o.fma(dth_, v[u], xx)
        else:
            m = mr.md_step(flags, x_in, v_in, F, hk[:, 0], mass, sigma, xi, c1, dth)     # (all atoms: the bounds are used for all)
            u = ~ca
            v[u] = m['v'][u]
            if flags & BEGIN:
                x_out[u] = m['x'][u]
            if flags & FINISH:
                ke[u] = m['ke'][u]
            out.update(bx=m['bx'], bv=m['bv'], bke=m['bke'])
    out.update(x=x_out, v=v, ke=ke, n_sweeps=sweeps, failed=failed, y=y, y_in=np.asarray(o.sub(x_in, x0), np.float64),
               v_in=np.asarray(v_in, np.float64), dth=float(dth), mass=mass)
    if want:
        ske = None if ke is None else np.asarray(mass, np.float64) * ((np.abs(v) * sv).sum(1) + 0.5 * (sv * sv).sum(1))
        out.update(sx=sx, sv=sv, ske=ske)
    return out


# ---- bounds ---------------------------------------------------------------------------------------------------------------------

def stored_residuals(T, x, v, tol, dth):
    """(position err, bound, velocity err, bound) [C] of docstring (1) on stored positions x and velocities v (v may be None)"""
    x = np.asarray(x, np.float64)
    y = x - x[T.mol_ptr[:-1][T.batch]]
    e = EPS32 * (np.abs(x) + np.abs(y))
    d2 = T.d2.astype(np.float64)
    r, ee = x[T.gi] - x[T.gj], e[T.gi] + e[T.gj]
    r2 = (r * r).sum(1)
    p_err, p_bound = np.abs(r2 - d2), tol * d2 + C_CON * (2.0 * (np.abs(r) * ee).sum(1) + 5.0 * EPS32 * r2)
    if v is None:
        return p_err, p_bound, None, None
    v = np.asarray(v, np.float64)
    u = v[T.gi] - v[T.gj]
    v_err = np.abs((r * u).sum(1)) * dth
    v_bound = tol * d2 + C_CON * dth * ((ee * np.abs(u)).sum(1) + 5.0 * EPS32 * np.abs(r * u).sum(1))
    return p_err, p_bound, v_err, v_bound


def solver_rounding(ref, T, flags, with_noise):
    """(rx, rv) [N,1]: first-order bound of what the fp32 roundings INSIDE the constrained chain add to positions and velocities,
    beyond the unconstrained chain's -- they scale with |y| / dth in the velocities, which the tolerance term does not.  Per
    molecule b, Y_b = max |y| and V_b = max |v| over its atoms and the launch, U_b = the sweeps the fp64 solver needs at the
    kernel's tolerance, + 1 for a decision that rounding turns (ref['U']).  In one SHAKE solve a coordinate of atom i is written
    once by the drift and at most deg_i U_b times by updates, one rounding <= EPS32 Y_b each: a_i = (1 + deg_i U_b) EPS32 Y_b.  The
    solve moves an atom by its own error and by those of its deg_i partners (weights <= 1), so an atom carries at most
    (1 + deg_i) A_b, A_b = max_i a_i.  Positions: that per SHAKE solve, + EPS32 Y_b (y = fl(x - x_first)) + EPS32 |x| (x_out) +
    dth rv.  Velocities: that / dth per drift (v takes (y'' - y') / dth) + per velocity solve (1 + deg_i)(1 + deg_max U_b) EPS32
    V_b by the same count.  C_MD multiplies the sum, as in md_ref."""
    N = ref['v'].shape[0]
    deg = np.bincount(np.concatenate([T.gi, T.gj]), minlength=N).astype(np.float64)
    n_shake = 2 if flags & BEGIN else 1 if flags & PROJECT else 0
    n_drift = 2 if flags & BEGIN else 0
    n_proj = (1 if flags & FINISH else 0) + ((4 if with_noise else 3) if flags & BEGIN else 0) + (1 if flags & PROJECT else 0)
    rx, rv = np.zeros((N, 1)), np.zeros((N, 1))
    for b in np.flatnonzero(T.has):
        sl = slice(T.mol_ptr[b], T.mol_ptr[b + 1])
        Y = max(np.abs(ref['y'][sl]).max(), np.abs(ref['y_in'][sl]).max())
        V = max(np.abs(ref['v'][sl]).max(), np.abs(ref['v_in'][sl]).max())
        U = float(ref['U'][b]) + 1.0
        A = ((1.0 + deg[sl] * U) * EPS32 * Y).max()
        carry = (1.0 + deg[sl]) * A
        rv[sl, 0] = n_drift * carry / ref['dth'] + n_proj * (1.0 + deg[sl]) * (1.0 + deg[sl].max() * U) * EPS32 * V
        rx[sl, 0] = n_shake * carry + EPS32 * Y + ref['dth'] * rv[sl, 0]
    return mr.C_MD * rx, mr.C_MD * rv


def fp64_bounds(ref, T, flags, with_noise):
    """(bx, bv, bke) of docstring (2) from `run(..., bound_tol=...)`: MARGIN x the summed responses + the rounding bound of the
    unconstrained chain + solver_rounding + half an ulp of the stored value"""
    rx, rv = solver_rounding(ref, T, flags, with_noise)
    bv = MARGIN * ref['sv'] + ref['bv'] + rv + mr.half_ulp32(ref['v'])
    bx = bke = None
    if ref['x'] is not None:
        chain = ref['bx'] if ref['bx'] is not None else 0.0
        bx = MARGIN * ref['sx'] + chain + rx + mr.C_MD * EPS32 * np.abs(ref['x']) * T.con_atom[:, None] + mr.half_ulp32(ref['x'])
    if ref['ke'] is not None:
        chain = ref['bke'] if ref['bke'] is not None else 0.0
        m = np.asarray(ref['mass'], np.float64)
        bke = MARGIN * ref['ske'] + m * (np.abs(ref['v']) * rv).sum(1) + chain + mr.half_ulp32(ref['ke'])
    return bx, bv, bke


# ---- the inputs of tests/test_hip_rattle.py ---------------------------------------------------------------------------------------

GRID = 2.0 ** -16      # positions are multiples of it, so that x + 100 is exact in fp32 and a shifted batch has the same y bit for bit
TOL = 1e-5
MAX_ITER = 150
BATCHES = {'diatomic': ['diatomic'], 'water': ['water'], 'ch4': ['ch4'],
           'mixed': ['free3', 'empty', 'water', 'ch4', 'mol21', 'pairs70'],
           'mixed9': ['free3', 'empty', 'water', 'ch4', 'mol21', 'pairs70', 'free3', 'empty', 'water'],
           'water_fixed': ['water'], 'mixed_shift': ['free3', 'empty', 'water', 'ch4', 'mol21', 'pairs70']}


def _unit(rng, n):
    u = rng.standard_normal((n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def molecule(kind, rng):
    """(masses [n], positions [n,3] with the first atom at the origin, local pairs [C,2], lengths [C]) of one test molecule"""
    H, Cm, O = 1.008, 12.011, 15.999
    if kind == 'empty':
        return np.zeros(0), np.zeros((0, 3)), np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    if kind == 'free3':
        return np.array([Cm, O, H]), np.concatenate([np.zeros((1, 3)), rng.uniform(-2, 2, (2, 3))]), np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    if kind == 'diatomic':
        return np.array([Cm, H]), np.concatenate([np.zeros((1, 3)), 1.09 * _unit(rng, 1)]), np.array([[0, 1]]), np.array([1.09])
    if kind == 'water':
        a, d = np.deg2rad(104.52), 0.9572
        x = np.array([[0, 0, 0], [d, 0, 0], [d * np.cos(a), d * np.sin(a), 0]])
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        return np.array([O, H, H]), x @ q.T, np.array([[0, 1], [0, 2], [1, 2]]), np.array([d, d, 2 * d * np.sin(a / 2)])
    if kind == 'ch4':
        t = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        return (np.array([Cm, H, H, H, H]), np.concatenate([np.zeros((1, 3)), 1.09 * t @ q.T]), np.array([[0, k] for k in range(1, 5)]),
                np.full(4, 1.09))
    if kind == 'mol21':            # 13 heavy atoms on a jittered 1.4 A grid, one hydrogen at 1.0 A on each of the first 8
        g = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(2), indexing='ij'), -1).reshape(-1, 3)[:13] * 1.4
        heavy = g + rng.normal(0, 0.05, g.shape)
        heavy -= heavy[0]
        h = heavy[:8] + 1.0 * _unit(rng, 8)
        return (np.concatenate([rng.choice([Cm, O], 13), np.full(8, H)]), np.concatenate([heavy, h]),
                np.array([[k, 13 + k] for k in range(8)]), np.full(8, 1.0))
    if kind == 'pairs70':          # 70 disjoint C-H pairs, every atom within 8 A of the first: 70 constraints of ONE colour
        heavy = 6.5 * _unit(rng, 70) * rng.random((70, 1)) ** (1 / 3)
        heavy[0] = 0.0
        h = heavy + 1.09 * _unit(rng, 70)
        x = np.stack([heavy, h], axis=1).reshape(140, 3)
        return np.tile([Cm, H], 70), x, np.array([[2 * k, 2 * k + 1] for k in range(70)]), np.full(70, 1.09)
    raise KeyError(kind)


def case(name, seed=0):
    """The fp32 inputs of one batch of BATCHES, as numpy arrays, with its constraints prepared (newtonnet_amd.constraints.prepare)
    and the reference's Tables: the time step is 2 fs (dth = 1 fs)"""
    from newtonnet_amd import constraints as con
    rng = np.random.default_rng(1000 + seed + sum(map(ord, name)) % 97 if name not in ('mixed', 'mixed_shift') else 1000 + seed)
    f32 = np.float32
    ms, xs, ps, ls, sizes = [], [], [], [], []
    for kind in BATCHES[name]:
        m, x, p, l = molecule(kind, rng)
        x = x + (rng.uniform(-6, 6, 3) if len(m) else 0.0)
        ps.append(np.asarray(p, dtype=np.int64).reshape(-1, 2) + sum(sizes))
        ms.append(m), xs.append(x), ls.append(l), sizes.append(len(m))
    m, x = np.concatenate(ms).astype(f32), np.concatenate(xs)
    x = (np.round(x / GRID) * GRID + (100.0 if name == 'mixed_shift' else 0.0)).astype(f32)
    N = m.size
    pairs, lengths = np.concatenate(ps), np.concatenate(ls).astype(f32)
    v, F = rng.uniform(-0.2, 0.2, (N, 3)).astype(f32), rng.uniform(-5, 5, (N, 3)).astype(f32)
    xi = rng.standard_normal((N, 3)).astype(f32)
    dt = 2.0 * FS
    m64 = m.astype(np.float64)
    hk, w = (0.5 * dt / m64).astype(f32), (1.0 / m64).astype(f32)
    sigma = np.sqrt(0.02 * K_B * 300.0 / m64).astype(f32)
    fixed = np.zeros(N, dtype=bool)
    if name == 'water_fixed':
        fixed[0] = True
    hk[fixed], w[fixed], sigma[fixed], v[fixed] = 0, 0, 0, 0
    mol_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    batch = np.repeat(np.arange(len(sizes)), sizes)
    prep = con.prepare(pairs, lengths, batch, len(sizes), fixed, max_atoms=256)
    d2 = (lengths.astype(np.float64)[prep.order] ** 2).astype(f32)
    dth = float(f32(0.5 * dt))
    return dict(x=x, v=v, F=F, m=m, hk=hk, w=w, sigma=sigma, xi=xi, fixed=fixed, mol_ptr=mol_ptr, batch=batch, prep=prep, d2=d2,
                dth=dth, inv_dth=float(f32(1.0 / dth)), c1=float(f32(np.exp(-0.01))), T=Tables(prep, d2, mol_ptr), sizes=sizes)


def run(d, flags, with_noise, fp32=False, tol=1e-13, max_iter=2000, bound_tol=None):
    """launch on the inputs of a case"""
    args = (flags, d['x'], d['v'], d['F'], d['hk'], d['m'], d['w'], d['T'], d['sigma'] if with_noise else None,
            d['xi'] if with_noise else None, d['c1'], d['dth'], d['inv_dth'])
    out = launch(*args, tol, max_iter, fp32, bound_tol)
    if bound_tol is not None and not fp32:
        out['U'] = launch(*args, bound_tol, max_iter)['n_sweeps']     # the sweeps exact arithmetic needs at the kernel's tolerance
    return out


def ratios(got, ref, T, flags, with_noise):
    """{x, v, ke: worst (err - what is not the summed response) / (summed response)} -- the figure MARGIN is 4 x the worst of --
    and {x, v, ke: worst err / bound}"""
    bx, bv, bke = fp64_bounds(ref, T, flags, with_noise)
    raw, rel = {}, {}
    for k, b, s in (('x', bx, 'sx'), ('v', bv, 'sv'), ('ke', bke, 'ske')):
        if ref[k] is None or got[k] is None:
            continue
        err = np.abs(np.asarray(got[k], np.float64) - ref[k])
        rest = b - MARGIN * ref[s]
        on = ref[s] > 0
        raw[k] = float((np.maximum(err - rest, 0.0)[on] / ref[s][on]).max()) if on.any() else 0.0
        rel[k] = float((err / b).max()) if err.size else 0.0
    return raw, rel


def host_energy_drift(evaluate, x, v, hk, mass, w, T, dth, inv_dth, tol, n_steps):
    """max_n |E_tot(n) - E_tot(0)| per molecule [B] of a host fp64 loop of the constrained velocity-Verlet scheme (launch: BEGIN,
    the forces at the new positions, FINISH) with the solves stopped at `tol`.  evaluate(x fp64 [N,3]) -> (forces [N,3], energies
    [B]) in fp64.  The difference between this figure at the kernel's tolerance and at 1e-13 is what stopping the solves early
    does to the energy: the constraint term of the device test, a reference-only measurement."""
    x, v, m = np.asarray(x, np.float64), np.asarray(v, np.float64), np.asarray(mass, np.float64)

    def total(e, v):
        ke = np.zeros(T.n_mol)
        np.add.at(ke, T.batch, (0.5 * m[:, None] * v * v).sum(1))
        return np.asarray(e, np.float64) + ke
    f, e = evaluate(x)
    energy = [total(e, v)]
    for _ in range(n_steps):
        a = launch(BEGIN, x, v, f, hk, m, w, T, dth=dth, inv_dth=inv_dth, tol=tol)
        x = a['x']
        f, e = evaluate(x)
        v = launch(FINISH, x, a['v'], f, hk, m, w, T, dth=dth, inv_dth=inv_dth, tol=tol)['v']
        energy.append(total(e, v))
    energy = np.asarray(energy)
    return np.abs(energy - energy[0]).max(axis=0)


if __name__ == '__main__':
    worst = {}
    for name in BATCHES:
        d = case(name)
        for flags in (FINISH, BEGIN, FINISH | BEGIN, PROJECT):
            for noise in (False, True):
                if noise and not flags & BEGIN:
                    continue
                ref = run(d, flags, noise, bound_tol=TOL)
                emu = run(d, flags, noise, fp32=True, tol=TOL, max_iter=MAX_ITER)
                raw, rel = ratios(emu, ref, d['T'], flags, noise)
                for k, r in raw.items():
                    worst[k] = max(worst.get(k, 0.0), r)
                print(f'{name:12s} flags {flags} noise {int(noise)}: emulation (err - rest) / sum {raw}; sweeps fp32 '
                      f'{emu["n_sweeps"].tolist()} fp64 {ref["n_sweeps"].tolist()}; failed {emu["failed"].any() or ref["failed"].any()}')
    print('worst emulation ratios', worst, '-> MARGIN = 4 x', max(worst.values()))
