"""fp64 statement of one nnhip_neb_step launch (csrc/neb.hip) for ONE band, for the tests (numpy), with a per-element rounding
bound, in the manner of tests/relax_ref.py.

The kernel's chain (every line ONE fp32 operation per element; dot3(a, b) = fma(az, bz, fma(ay, by, ax bx)); sum_l = lane-local sum
in atom order, lane l owning the atoms l, l + 64, ... of an image, then the butterfly 32, 16, ..., 1; SUM_i = the per-image values
added in image order; every vector of a fixed atom is exactly 0):
    interior image i:  tp = R_{i+1} - R_i;  tm = R_i - R_{i-1}
        E_{i+1} > E_i > E_{i-1}: tau = tp;   E_{i+1} < E_i < E_{i-1}: tau = tm;   otherwise, a = max(|E_{i+1} - E_i|, |E_{i-1} - E_i|),
        b = the min:  tau = fma(cp, tp, cm tm), (cp, cm) = (a, b) if E_{i+1} > E_{i-1} else (b, a)
        nt = sqrt(sum_l dot3(tau, tau));  that = tau / nt  (0 when the sum is 0)
        lp, lm = sqrt(sum_l dot3(tp, tp)), sqrt(sum_l dot3(tm, tm));  fd = sum_l dot3(f, that)
        c = spring (lp - lm) - fd   (the climbing image, climbing set BEFORE the launch:  c = -2 fd);   F = fma(c, that, f)
    fmax2 = max over interior images and atoms of dot3(F, F);  FF, P, VV = SUM_i sum_l dot3 of (F, F), (F, v), (v, v)
    flags (not with CHECK_ONLY, not when converged before):  converged iff fmax2 < tol2 and (no CLIMB or climbing set before);
        climbing |= CLIMB and fmax2 < climb2
    frozen (converged before | converged now | CHECK_ONLY):  x_out = x, nothing else
    first step:  v = 0, dt = dt_start, a = a_start, n_pos = 0;   else
        P > 0:   v = fma(c2, F, c1 v), c1 = 1 - a, c2 = (a sqrt(VV)) / sqrt(FF);  n_pos > n_min:  dt = min(dt f_inc, dt_max), a = a f_a;
                 n_pos += 1
        P <= 0:  v = 0;  a = a_start;  dt = dt f_dec;  n_pos = 0
    v = fma(dt, F, v);  dr = dt v;  nd = sqrt(SUM_i sum_l dot3(dr, dr));  nd > maxstep:  dr = dr (maxstep / nd);  x_out = x + dr

`neb_step` evaluates that in fp64 from the SAME fp32 inputs and state and carries a first-order bound next to every value: an
operation with exact result r adds eps |r| (eps = EPS32 = 2^-24), and the bounds of its operands pass through multiplied by the
magnitudes of the other operands.  A reduction whose terms pass through at most `depth` roundings costs (depth + 1) eps sum |term|
plus the propagated operand bounds; depth = 3 + ceil(n / 64) + 6 for a per-image dot product (relax_ref.dot_depth), and the sum
over the images of a band adds one rounding per interior image.  The energies enter through comparisons and through
fl32(E' - E), ONE correctly rounded subtraction of the inputs, which numpy's float32 reproduces exactly: they carry no bound and
no energy decision is ever ambiguous.  State that a caller hands in as exact has bound 0; `b_vel`, `b_dt`, `b_a` carry the FIRST-ORDER
bounds of a state that came out of an earlier neb_step (the stepwise test of recorded frames).

C_NEB = 2 multiplies the first-order sum at the outputs, for what first order leaves out, as C_MD and C_RX do; it is chosen before
any run.  Results below the normal range add TINY32.

The derived decisions of a step -- convergence (fmax2 < tol2), the climb switch (fmax2 < climb2), the sign of P, the cap of dt and
the clamp (nd > maxstep) -- are reported as AMBIGUOUS when the fp64 value lies within C_NEB x its own bound of its threshold: the
kernel may then decide either way, and a test either constructs inputs without such a case (and says so) or skips and counts it."""
import math

import numpy as np

from tests.relax_ref import EPS32, TINY32, dot_depth, half_ulp32  # noqa: F401

C_NEB = 2.0
CHECK_ONLY, CLIMB = 1, 2
MAX_IMAGES = 64
f32 = np.float32
# ase.optimize.FIRE's defaults as the fp32 values the kernel gets
FIRE = dict(dt=float(f32(0.1)), dt_max=1.0, n_min=5, f_inc=float(f32(1.1)), f_dec=0.5, a_start=float(f32(0.1)), f_a=float(f32(0.99)),
            maxstep=float(f32(0.2)))


def params(spring=0.1, fmax=0.05, climb_below=None, **fire):
    """the launch parameters as the Python floats of their fp32 values (climb_below None: 5 fmax)"""
    climb_below = 5.0 * fmax if climb_below is None else climb_below
    p = dict(FIRE, spring=float(f32(spring)), tol2=float(f32(fmax * fmax)), climb2=float(f32(climb_below * climb_below)))
    p.update({k: float(f32(v)) for k, v in fire.items()})
    return p


def new_state(n_img, n):
    """the state of a band before its first step"""
    z = np.zeros((n_img, n, 3))
    return dict(converged=False, climbing=False, n_steps=0, n_pos=0, dt=0.0, a=0.0, vel=z, b_vel=z.copy(), b_dt=0.0, b_a=0.0)


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def _dot(a, ba, b, bb, eps):
    """sum_l dot3 over the atoms of ONE image: value and first-order bound"""
    t = a * b
    return float(t.sum()), (dot_depth(a.shape[0]) + 1) * eps * float(np.abs(t).sum()) + float((np.abs(a) * bb + np.abs(b) * ba).sum())


def _sqrt(v, b, eps):
    r = math.sqrt(v)
    return r, ((b / (2.0 * r)) if r > 0 else math.sqrt(b)) + eps * r


def climbing_image(E):
    """index of the interior image of highest energy, the lowest index at a tie"""
    return 1 + int(np.argmax(np.asarray(E)[1:-1]))


def tangent_case(E, i, exact=False):
    """('up' | 'down' | 'mixed', cp, cm) of interior image i: the coefficients of tau = cp tp + cm tm"""
    E = np.asarray(E, dtype=np.float64)
    em, e0, ep = E[i - 1], E[i], E[i + 1]
    if ep > e0 > em:
        return 'up', 1.0, 0.0
    if ep < e0 < em:
        return 'down', 0.0, 1.0
    if exact:
        dp, dm = abs(ep - e0), abs(em - e0)
    else:
        dp, dm = abs(float(f32(f32(ep) - f32(e0)))), abs(float(f32(f32(em) - f32(e0))))
    hi, lo = max(dp, dm), min(dp, dm)
    return ('mixed', hi, lo) if ep > em else ('mixed', lo, hi)


def neb_forces(x, F, E, free, climbing, spring, eps=EPS32, vel=None, b_vel=None):
    """Tangents and NEB forces of one band.  x, F [I,n,3], E [I], free bool [I,n] or None.  Returns a dict: that, b_that, Fn, b_F
    [I,n,3] (first order, endpoints 0), fmax2, b_fmax2, top, cases, and the band sums FF, P, VV with their bounds."""
    x, F, E = np.asarray(x, dtype=np.float64), np.asarray(F, dtype=np.float64), np.asarray(E, dtype=np.float64)
    n_img, n = x.shape[0], x.shape[1]
    m = np.ones((n_img, n, 1)) if free is None else np.asarray(free, dtype=np.float64).reshape(n_img, n, 1)
    f = F * m
    v = np.zeros_like(x) if vel is None else np.asarray(vel, dtype=np.float64) * m
    bv = np.zeros_like(x) if b_vel is None else np.asarray(b_vel, dtype=np.float64) * m
    top = climbing_image(E)
    that, b_that, Fn, b_F = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    fmax2 = b_fmax2 = 0.0
    sums = dict(FF=[], P=[], VV=[])
    cases = []
    for i in range(1, n_img - 1):
        tp, tm = (x[i + 1] - x[i]) * m[i], (x[i] - x[i - 1]) * m[i]
        b_tp, b_tm = eps * np.abs(tp), eps * np.abs(tm)
        case, cp, cm = tangent_case(E, i, exact=eps == 0.0)
        cases.append(case)
        if case == 'up':
            tau, b_tau = tp, b_tp
        elif case == 'down':
            tau, b_tau = tm, b_tm
        else:
            u = cm * tm
            tau = cp * tp + u
            b_tau = cp * b_tp + cm * b_tm + eps * np.abs(u) + eps * np.abs(tau)
        tt, b_tt = _dot(tau, b_tau, tau, b_tau, eps)
        if tt > 0.0:
            nt, b_nt = _sqrt(tt, b_tt, eps)
            that[i] = tau / nt
            b_that[i] = b_tau / nt + np.abs(tau) * b_nt / (nt * nt) + eps * np.abs(that[i])
        lp, b_lp = _sqrt(*_dot(tp, b_tp, tp, b_tp, eps), eps)
        lm, b_lm = _sqrt(*_dot(tm, b_tm, tm, b_tm, eps), eps)
        fd, b_fd = _dot(f[i], 0.0, that[i], b_that[i], eps)
        if climbing and i == top:
            c, b_c = -2.0 * fd, 2.0 * b_fd
        else:
            d = lp - lm
            b_d = b_lp + b_lm + eps * abs(d)
            sd = spring * d
            b_sd = spring * b_d + eps * abs(sd)
            c = sd - fd
            b_c = b_sd + b_fd + eps * abs(c)
        Fn[i] = (f[i] + c * that[i]) * m[i]
        b_F[i] = (abs(c) * b_that[i] + np.abs(that[i]) * b_c + eps * np.abs(Fn[i])) * m[i]
        F2 = (Fn[i] * Fn[i]).sum(1)
        b_F2 = 2.0 * (np.abs(Fn[i]) * b_F[i]).sum(1) + 4.0 * eps * F2
        if n:
            fmax2, b_fmax2 = max(fmax2, float(F2.max())), max(b_fmax2, float(b_F2.max()))
        sums['FF'].append(_dot(Fn[i], b_F[i], Fn[i], b_F[i], eps))
        sums['P'].append(_dot(Fn[i], b_F[i], v[i], bv[i], eps))
        sums['VV'].append(_dot(v[i], bv[i], v[i], bv[i], eps))
    out = dict(that=that, b_that=b_that, Fn=Fn, b_F=b_F, fmax2=fmax2, b_fmax2=b_fmax2, top=top, cases=cases, v=v, b_v=bv, mask=m)
    for k, terms in sums.items():
        out[k], out['b_' + k] = _band_sum(terms, eps)
    return out


def _band_sum(terms, eps):
    """the per-image values added in image order: one more rounding per image"""
    val = sum(t[0] for t in terms)
    return val, sum(t[1] for t in terms) + len(terms) * eps * sum(abs(t[0]) for t in terms)


def neb_step(x, F, E, free, st, prm, flags=0, eps=EPS32, decide=None):
    """One launch for one band.  x, F [I,n,3]: the fp32 values the kernel gets; E [I]; free: bool [I,n] or None; st: the state
    (new_state; not modified); prm: params().  Returns a dict:
      tangent, b_tangent, neb_force, b_neb_force [I,n,3]   values and bounds (C_NEB x first order + TINY32 where non-zero)
      fmax, b_fmax;  saddle (image index);  cases (tangent case of every interior image)
      x_out, bx [I,n,3]   frozen bands, endpoints and fixed atoms: x, 0
      state    the state after the launch (vel, dt, a in fp64 with FIRST-ORDER bounds b_vel, b_dt, b_a)
      b_vel_out [I,n,3], b_dt_out, b_a_out   C_NEB x those + TINY32
      frozen, fire ('first' | 'mix' | 'mix_inc' | 'reset' | None), capped, clamped
      ambiguous   dict(converge, climb, P, dt_cap, clamp) of bools
    decide: None, or a dict with some of converge, climb, P, clamp -> the decision to follow instead of the fp64 one, for a caller
    that knows what the kernel decided in an ambiguous case."""
    decide = decide or {}
    x = np.asarray(x, dtype=np.float64)
    n_img, n = x.shape[0], x.shape[1]
    spring = prm['spring']
    first = st['n_steps'] == 0
    r = neb_forces(x, F, E, free, st['climbing'], spring, eps, None if first else st['vel'], None if first else st['b_vel'])
    m, Fn, b_F, v, b_v = r['mask'], r['Fn'], r['b_F'], r['v'], r['b_v']
    amb = dict(converge=False, climb=False, P=False, dt_cap=False, clamp=False)
    fmax2, b_fmax2 = r['fmax2'], r['b_fmax2']
    fmax, b_fmax = _sqrt(fmax2, b_fmax2, eps)

    def widen(b):
        return np.where(b > 0, C_NEB * b + TINY32, 0.0)
    out = dict(tangent=r['that'], b_tangent=widen(r['b_that']), neb_force=Fn, b_neb_force=widen(b_F), fmax=fmax,
               b_fmax=C_NEB * b_fmax + TINY32, saddle=r['top'], cases=r['cases'], fire=None, capped=False, clamped=False, ambiguous=amb)
    check_only, climb_req = bool(flags & CHECK_ONLY), bool(flags & CLIMB)
    new = copy_state(st)
    touch = not check_only and not st['converged']
    conv_now = climb_now = False
    if touch:
        if not climb_req or st['climbing']:
            conv_now = decide.get('converge', fmax2 < prm['tol2'])
            amb['converge'] = abs(fmax2 - prm['tol2']) <= C_NEB * b_fmax2
        if climb_req and not st['climbing']:
            climb_now = decide.get('climb', fmax2 < prm['climb2'])
            amb['climb'] = abs(fmax2 - prm['climb2']) <= C_NEB * b_fmax2
    new['converged'] = bool(st['converged'] or conv_now)
    new['climbing'] = bool(st['climbing'] or climb_now)
    if st['converged'] or conv_now or check_only:
        out.update(x_out=x.copy(), bx=np.zeros_like(x), state=new, frozen=True, b_vel_out=np.zeros_like(x), b_dt_out=0.0, b_a_out=0.0)
        return out
    dt, b_dt, a, b_a, n_pos = st['dt'], st['b_dt'], st['a'], st['b_a'], st['n_pos']
    if first:
        dt, b_dt, a, b_a, n_pos = prm['dt'], 0.0, prm['a_start'], 0.0, 0
        v1, b_v1 = np.zeros_like(x), np.zeros_like(x)
        out['fire'] = 'first'
    else:
        P, b_P = r['P'], r['b_P']
        amb['P'] = abs(P) <= C_NEB * b_P
        if decide.get('P', P > 0.0):
            c1 = 1.0 - a
            b_c1 = b_a + eps * abs(c1)
            nv, b_nv = _sqrt(r['VV'], r['b_VV'], eps)
            nf, b_nf = _sqrt(r['FF'], r['b_FF'], eps)
            an = a * nv
            b_an = a * b_nv + nv * b_a + eps * abs(an)
            c2 = an / nf
            b_c2 = b_an / nf + an * b_nf / (nf * nf) + eps * abs(c2)
            u = c1 * v
            b_u = abs(c1) * b_v + np.abs(v) * b_c1 + eps * np.abs(u)
            v1 = c2 * Fn + u
            b_v1 = abs(c2) * b_F + np.abs(Fn) * b_c2 + b_u + eps * np.abs(v1)
            out['fire'] = 'mix'
            if n_pos > prm['n_min']:
                dtn = dt * prm['f_inc']
                b_dtn = prm['f_inc'] * b_dt + eps * abs(dtn)
                amb['dt_cap'] = dtn != prm['dt_max'] and abs(dtn - prm['dt_max']) <= C_NEB * b_dtn
                out['capped'] = dtn > prm['dt_max']
                dt, b_dt = (prm['dt_max'], 0.0) if out['capped'] else (dtn, b_dtn)
                a = a * prm['f_a']
                b_a = prm['f_a'] * b_a + eps * abs(a)
                out['fire'] = 'mix_inc'
            n_pos += 1
        else:
            v1, b_v1 = np.zeros_like(x), np.zeros_like(x)
            a, b_a = prm['a_start'], 0.0
            dt = dt * prm['f_dec']
            b_dt = prm['f_dec'] * b_dt + eps * abs(dt)
            n_pos = 0
            out['fire'] = 'reset'
    inner = np.zeros((n_img, 1, 1))
    inner[1:-1] = 1.0
    mm = m * inner
    v2 = (v1 + dt * Fn) * mm
    b_v2 = (b_v1 + dt * b_F + np.abs(Fn) * b_dt + eps * np.abs(v2)) * mm
    dr = dt * v2
    b_dr = dt * b_v2 + np.abs(v2) * b_dt + eps * np.abs(dr)
    DD, b_DD = _band_sum([_dot(dr[i], b_dr[i], dr[i], b_dr[i], eps) for i in range(1, n_img - 1)], eps)
    nd, b_nd = _sqrt(DD, b_DD, eps)
    amb['clamp'] = abs(nd - prm['maxstep']) <= C_NEB * b_nd
    clamped = decide.get('clamp', nd > prm['maxstep'])
    if clamped:
        scale = prm['maxstep'] / nd
        b_scale = scale * b_nd / nd + eps * scale
        dr2 = dr * scale
        b_dr = scale * b_dr + np.abs(dr) * b_scale + eps * np.abs(dr2)
        dr = dr2
    x_out = np.where(mm > 0, x + dr, x)
    bx = np.where(mm > 0, b_dr + eps * np.abs(x_out), 0.0)
    # the kernel keeps the velocity rows of fixed atoms and endpoints as they are
    vel_new = np.where(mm > 0, v2, st['vel'])
    new.update(n_steps=st['n_steps'] + 1, n_pos=n_pos, dt=dt, b_dt=b_dt, a=a, b_a=b_a, vel=vel_new, b_vel=b_v2)
    out.update(x_out=x_out, bx=widen(bx), state=new, frozen=False, clamped=bool(clamped), b_vel_out=widen(b_v2),
               b_dt_out=(C_NEB * b_dt + TINY32) if b_dt > 0 else 0.0, b_a_out=(C_NEB * b_a + TINY32) if b_a > 0 else 0.0)
    return out


# ---- the same chain in numpy float32, in the kernel's order of operations (for the host tests) ------------------------------------

def _fma32(a, b, c):
    # (a b is exact in fp64 for fp32 operands; the sum rounds to fp64 and then to fp32 -- a double rounding that differs from a
    # true fma in rare ties only, far inside every bound here)
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def _dot3_32(a, b):
    return _fma32(a[:, 2], b[:, 2], _fma32(a[:, 1], b[:, 1], (a[:, 0] * b[:, 0]).astype(f32)))


def _wave_sum32(t):
    acc = np.zeros(64, dtype=f32)
    for i0 in range(0, t.shape[0], 64):
        chunk = t[i0:i0 + 64]
        acc[:chunk.shape[0]] = acc[:chunk.shape[0]] + chunk
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[lanes ^ d]).astype(f32)
    return acc[0]


def emulate_step(x, F, E, free, st, prm, flags=0):
    """neb_step in float32 arithmetic, operation for operation as the kernel orders them.  Returns a dict with pos_out, tangent,
    neb_force, vel (float32), fmax, dt, a (float32 scalars), converged, climbing, n_steps, n_pos, saddle."""
    x, F, E = np.asarray(x, dtype=f32), np.asarray(F, dtype=f32), np.asarray(E, dtype=f32)
    n_img, n = x.shape[0], x.shape[1]
    fr = np.ones((n_img, n), dtype=bool) if free is None else np.asarray(free, dtype=bool)
    first = st['n_steps'] == 0
    P = {k: f32(v) for k, v in prm.items() if k != 'n_min'}
    vel = np.asarray(st['vel'], dtype=f32).copy()
    that, Fn = np.zeros_like(x), np.zeros_like(x)
    top = climbing_image(E)
    zero = f32(0)
    fmax2 = FF = Pw = VV = zero
    for i in range(1, n_img - 1):
        mk = fr[i][:, None]
        tp = np.where(mk, (x[i + 1] - x[i]).astype(f32), zero)
        tm = np.where(mk, (x[i] - x[i - 1]).astype(f32), zero)
        case, cp, cm = tangent_case(E, i)
        tau = tp if case == 'up' else tm if case == 'down' else _fma32(f32(cp), tp, (f32(cm) * tm).astype(f32))
        tt, sp, sm = _wave_sum32(_dot3_32(tau, tau)), _wave_sum32(_dot3_32(tp, tp)), _wave_sum32(_dot3_32(tm, tm))
        th = (tau / np.sqrt(tt, dtype=f32)).astype(f32) if tt > 0 else np.zeros_like(tau)
        f = np.where(mk, F[i], zero)
        fd = _wave_sum32(_dot3_32(f, th))
        if st['climbing'] and i == top:
            c = f32(f32(-2) * fd)
        else:
            c = f32(f32(P['spring'] * f32(np.sqrt(sp, dtype=f32) - np.sqrt(sm, dtype=f32))) - fd)
        Fi = np.where(mk, _fma32(c, th, f), zero)
        v = np.zeros_like(Fi) if first else np.where(mk, vel[i], zero)
        that[i], Fn[i] = th, Fi
        F2 = _dot3_32(Fi, Fi)
        if n:
            fmax2 = max(fmax2, F2.max())
        FF = f32(FF + _wave_sum32(F2))
        Pw = f32(Pw + _wave_sum32(_dot3_32(Fi, v)))
        VV = f32(VV + _wave_sum32(_dot3_32(v, v)))
    check_only, climb_req = bool(flags & CHECK_ONLY), bool(flags & CLIMB)
    touch = not check_only and not st['converged']
    conv_now = touch and fmax2 < P['tol2'] and (not climb_req or st['climbing'])
    climb_now = touch and climb_req and fmax2 < P['climb2']
    out = dict(tangent=that, neb_force=Fn, fmax=np.sqrt(f32(fmax2), dtype=f32), saddle=top, converged=bool(st['converged'] or conv_now),
               climbing=bool(st['climbing'] or climb_now), n_steps=st['n_steps'], n_pos=st['n_pos'], dt=f32(st['dt']), a=f32(st['a']),
               vel=vel, pos_out=x.copy())
    if st['converged'] or conv_now or check_only:
        return out
    dt, a, n_pos = f32(st['dt']), f32(st['a']), st['n_pos']
    keep = False
    c1 = c2 = zero
    if first:
        dt, a, n_pos = P['dt'], P['a_start'], 0
    elif Pw > 0:
        keep = True
        c1 = f32(f32(1) - a)
        c2 = f32(f32(a * np.sqrt(VV, dtype=f32)) / np.sqrt(FF, dtype=f32))
        if n_pos > prm['n_min']:
            dt = min(f32(dt * P['f_inc']), P['dt_max'])
            a = f32(a * P['f_a'])
        n_pos += 1
    else:
        a, dt, n_pos = P['a_start'], f32(dt * P['f_dec']), 0
    DD = zero
    drs = np.zeros_like(x)
    for i in range(1, n_img - 1):
        mk = fr[i][:, None]
        v = np.where(mk, vel[i], zero) if keep else np.zeros_like(Fn[i])
        if keep:
            v = _fma32(c2, Fn[i], (c1 * v).astype(f32))
        v = _fma32(dt, Fn[i], v)
        vel[i] = np.where(mk, v, vel[i])
        drs[i] = np.where(mk, (dt * v).astype(f32), zero)
        DD = f32(DD + _wave_sum32(_dot3_32(drs[i], drs[i])))
    nd = np.sqrt(DD, dtype=f32)
    if nd > P['maxstep']:
        drs = (drs * f32(P['maxstep'] / nd)).astype(f32)
    pos_out = x.copy()
    for i in range(1, n_img - 1):
        pos_out[i] = np.where(fr[i][:, None], (x[i] + drs[i]).astype(f32), x[i])
    out.update(pos_out=pos_out, vel=vel, dt=f32(dt), a=f32(a), n_pos=n_pos, n_steps=st['n_steps'] + 1)
    return out


# ---- fp64 CI-NEB + FIRE of one band, driven by a callable (the yardstick of the convergence test) ---------------------------------

def minimise(energy_forces, x0, spring=0.1, fmax=0.05, climb=True, climb_below=None, max_steps=1000, free=None, **fire):
    """The contract above as a plain fp64 loop for one band: energy_forces(x [I,n,3] fp64) -> (E [I], F [I,n,3]); positions and
    every operation stay fp64 (eps = 0: energy differences are the fp64 ones too).  Returns dict(x, energy, neb_force, tangent, fmax,
    converged, climbing, n_steps, saddle, barrier_forward, barrier_reverse, climb_step)."""
    x = np.asarray(x0, dtype=np.float64).copy()
    prm = dict(FIRE, spring=float(spring), tol2=float(fmax) ** 2,
               climb2=float(5.0 * fmax if climb_below is None else climb_below) ** 2)
    prm.update({k: float(v) for k, v in fire.items()})
    st = new_state(x.shape[0], x.shape[1])
    flags = CLIMB if climb else 0
    climb_step = None
    for k in range(max_steps + 1):
        E, F = energy_forces(x)
        E, F = np.asarray(E, dtype=np.float64), np.asarray(F, dtype=np.float64)
        r = neb_step(x, F, E, free, st, prm, flags | (CHECK_ONLY if k == max_steps else 0), eps=0.0)
        if r['state']['climbing'] and climb_step is None:
            climb_step = k
        x, st = r['x_out'], r['state']
        if st['converged']:
            break
    top = r['saddle']
    return dict(x=x, energy=E, neb_force=r['neb_force'], tangent=r['tangent'], fmax=r['fmax'], converged=st['converged'],
                climbing=st['climbing'], n_steps=st['n_steps'], saddle=top, barrier_forward=E[top] - E[0],
                barrier_reverse=E[top] - E[-1], climb_step=climb_step)


# ---- a physical path: the rotation of a methyl group (the convergence and the stepwise tests) -------------------------------------

def methyl(z, pos):
    """(C, the heavy atom it is bonded to, [H, H, H]) of the first carbon that carries exactly three hydrogens"""
    z, pos = np.asarray(z), np.asarray(pos, dtype=np.float64)
    d = np.linalg.norm(pos[:, None] - pos[None], axis=2)
    for c in np.flatnonzero(z == 6):
        hs = [int(j) for j in np.flatnonzero((z == 1) & (d[c] < 1.25))]
        heavy = [int(j) for j in np.flatnonzero((z > 1) & (d[c] < 1.75)) if j != c]
        if len(hs) == 3 and len(heavy) == 1:
            return int(c), heavy[0], hs
    raise ValueError('no methyl group')


def methyl_rotation_band(z, pos_a, n_images):
    """[n_images, n, 3] fp64: image i has the methyl hydrogens of pos_a rotated about the C-C axis by (2 pi / 3) i / (n_images - 1);
    the last image is replaced by B = pos_a with the three hydrogen positions cyclically permuted (each hydrogen at the original
    position nearest to where the full rotation takes it)"""
    pos_a = np.asarray(pos_a, dtype=np.float64)
    c, heavy, hs = methyl(z, pos_a)
    axis = pos_a[c] - pos_a[heavy]
    axis /= np.linalg.norm(axis)

    def rotated(angle):
        out = pos_a.copy()
        for h in hs:
            v = pos_a[h] - pos_a[c]
            out[h] = pos_a[c] + (v * math.cos(angle) + np.cross(axis, v) * math.sin(angle) + axis * (axis @ v) * (1.0 - math.cos(angle)))
        return out
    band = np.stack([rotated(2.0 * math.pi / 3.0 * i / (n_images - 1)) for i in range(n_images)])
    b = pos_a.copy()
    took = []
    for h in hs:
        j = hs[int(np.argmin([np.linalg.norm(band[-1][h] - pos_a[k]) for k in hs]))]
        b[h] = pos_a[j]
        took.append(j)
    assert sorted(took) == sorted(hs) and all(j != h for j, h in zip(took, hs))
    band[-1] = b
    return band


# ---- synthetic kernel inputs: every branch of a launch (shared by the host and the GPU tests) -------------------------------------

SYN_SIZES = (1, 2, 21, 63, 64, 65, 200)
SYN_IMAGES = (3, 4, 5, 7, 9)                             # 9: more images than the four waves of a workgroup, twice over
SYN_PROFILES = ('rising', 'falling', 'max_first', 'max_mid', 'max_last', 'min', 'ties')
# first: n_steps = 0;  pos_low / pos_high: P > 0 with n_pos <= / > n_min;  cap: dt f_inc passes dt_max;  neg: P <= 0;
# converged: flag set, large forces;  converging: fmax 0.005 < 0.01 with the climbing flag set;  pending: the same forces with the
# flag clear (converges only without CLIMB);  switch: fmax 0.03 between fmax and climb_below, flag clear;  climbing: flag set
SYN_KINDS = ('first', 'pos_low', 'pos_high', 'cap', 'neg', 'converged', 'converging', 'pending', 'switch', 'climbing')
SYN_FMAX, SYN_CLIMB_BELOW, SYN_SPRING = 0.01, 0.05, 0.1
ULP_E = 2.0 ** -9                                        # one fp32 ulp of an energy of 1.76e4 eV


def _profile(name, n_img, rng):
    """energies of a band in units of ULP_E above the base, as integers"""
    up = np.cumsum(rng.integers(1, 6, n_img))
    if name == 'rising':
        return up
    if name == 'falling':
        return up[::-1].copy()
    if name in ('max_first', 'max_mid', 'max_last', 'min'):
        peak = {'max_first': 1, 'max_mid': n_img // 2, 'max_last': n_img - 2, 'min': n_img // 2}[name]
        e = 40 - np.abs(np.arange(n_img) - peak) * rng.integers(2, 6) - rng.integers(0, 2, n_img)
        e[peak] = 41
        return -e if name == 'min' else e
    e = np.full(n_img, 7)                                # ties: a plateau that holds the maximum, between two lower endpoints
    e[0], e[-1] = 3, 5
    if n_img > 4:
        e[-2] = 6
    return e


def _band(rng, n, n_img, profile, kind, big, fixed):
    prm = params(SYN_SPRING, SYN_FMAX, SYN_CLIMB_BELOW)
    free = np.ones((n_img, n), dtype=bool)
    if fixed and n >= 2:
        free[:] = (rng.random(n) >= 0.25)[None]
        free[:, rng.integers(n)] = True
    a_pos, b_pos = rng.uniform(-8, 8, (n, 3)), None
    b_pos = a_pos + rng.normal(0, 0.25, (n, 3)) * math.sqrt(n_img - 1) / math.sqrt(n)
    w = np.linspace(0, 1, n_img)[:, None, None]
    x = (a_pos[None] * (1 - w) + b_pos[None] * w + rng.normal(0, 0.01 / math.sqrt(n), (n_img, n, 3))).astype(f32)
    E = (f32(-17600.0) + (_profile(profile, n_img, rng) * ULP_E).astype(f32)).astype(f32)
    F = rng.normal(0, 1.0, (n_img, n, 3))
    st = new_state(n_img, n)
    st['vel'] = np.full((n_img, n, 3), 7.0)              # what a first step must not read; endpoints and fixed atoms keep it
    target_fmax = {'converging': 0.005, 'pending': 0.005, 'switch': 0.03}.get(kind)
    target_nd = None if target_fmax else (1.0 if big else 0.03)
    if kind != 'first':
        n_pos, dt = {'pos_low': (2, 0.1), 'pos_high': (7, 0.3), 'cap': (9, 0.95), 'neg': (4, 0.4)}.get(kind, (3, 0.2))
        st.update(n_steps=n_pos + 6, n_pos=n_pos, dt=float(f32(dt)), a=float(f32(0.1 * 0.99 ** max(n_pos - 5, 0))))
        st['converged'], st['climbing'] = kind == 'converged', kind in ('converging', 'climbing')
    v = rng.normal(0, 1.0, (n_img, n, 3))
    for _ in range(8):                                   # scale forces (and velocities with them) to the wanted fmax or step length
        F32 = F.astype(f32)
        if kind != 'first':
            r0 = neb_forces(x, F32, E, free, st['climbing'], prm['spring'], 0.0)
            sign = -1.0 if kind == 'neg' else 1.0
            vv = (sign * 0.3 * r0['Fn'] + 0.1 * np.sqrt((r0['Fn'] ** 2).mean()) * v) * st['dt']
            st['vel'] = np.where((free[:, :, None]) & (np.arange(n_img)[:, None, None] % (n_img - 1) > 0), vv.astype(f32).astype(np.float64), 7.0)
        r = neb_step(x, F32, E, free, dict(st, converged=False), prm, 0, eps=0.0, decide=dict(converge=False, clamp=False))
        if target_fmax:
            F = F * (target_fmax / r['fmax'])
        else:
            nd = math.sqrt(((r['x_out'] - x.astype(np.float64)) ** 2).sum())
            F = F * (target_nd / nd)
    return dict(n=n, n_img=n_img, sizes=[n] * n_img, profile=profile, kind=kind, big=big, x=x, F=F.astype(f32), E=E, free=free,
                vel=st['vel'].astype(f32), converged=int(st['converged']), climbing=int(st['climbing']), n_steps=st['n_steps'],
                n_pos=st['n_pos'], dt=f32(st['dt']), a=f32(st['a']))


def synthetic_bands(seed=0):
    """The bands of the kernel test: every kind of SYN_KINDS at every size of SYN_SIZES, image counts and energy profiles cycling
    through SYN_IMAGES x SYN_PROFILES (35 combinations, each twice), alternately a short step (no clamp) and a long one (clamp),
    every third band of >= 2 atoms per image with a quarter of its atoms fixed.  Then the special bands: 'coincident' (an interior
    image and both its neighbours at the same positions: a zero-length tangent, the image gets its plain force), 'flat' (all
    energies equal: the same through a = b = 0) and 'unequal' (images of 5, 5 and 6 atoms: skipped, fmax = NaN).  Returns a list of
    dicts (x, F, vel [I,n,3]; E [I]; free [I,n]; the state words)."""
    rng = np.random.default_rng(seed)
    bands = []
    for k, kind in enumerate(SYN_KINDS):
        for s, n in enumerate(SYN_SIZES):
            idx = k * len(SYN_SIZES) + s
            bands.append(_band(rng, n, SYN_IMAGES[idx % 5], SYN_PROFILES[idx % 7], kind, bool(idx % 2), idx % 3 == 0))
    c = _band(rng, 21, 4, 'rising', 'pos_low', False, False)
    c['x'][1], c['x'][2] = c['x'][0], c['x'][0]
    c['x'][3] = c['x'][0]
    c['kind'] = 'coincident'
    fl = _band(rng, 21, 5, 'rising', 'pos_low', False, True)
    fl['E'][:] = fl['E'][0]
    fl['kind'], fl['profile'] = 'flat', 'flat'
    u = _band(rng, 6, 3, 'max_mid', 'first', False, False)
    u.update(kind='unequal', sizes=[5, 5, 6])
    mid = _band(rng, 21, 7, 'max_mid', 'climbing', True, True)           # a climbing image away from both ends of its band
    return bands + [c, fl, u, mid]


def flatten(bands):
    """a list of such bands in the kernel's layout and types: dict of numpy arrays (x, F, vel [N,3]; E [B]; free [N]; ptr [B+1];
    band_ptr [K+1]; converged, climbing, n_steps, n_pos int32 [K]; dt, a float32 [K])"""
    rows = {k: [] for k in ('x', 'F', 'vel', 'free')}
    sizes, counts = [], []
    for b in bands:
        total = sum(b['sizes'])
        for k in ('x', 'F', 'vel'):
            rows[k].append(np.asarray(b[k], dtype=f32).reshape(-1, 3)[:total])
        rows['free'].append(np.asarray(b['free'], dtype=bool).reshape(-1)[:total])
        sizes += b['sizes']
        counts.append(len(b['sizes']))
    out = {k: np.ascontiguousarray(np.concatenate(v)) for k, v in rows.items()}
    out['E'] = np.concatenate([np.asarray(b['E'], dtype=f32) for b in bands])
    out['ptr'] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    out['band_ptr'] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    for k in ('converged', 'climbing', 'n_steps', 'n_pos'):
        out[k] = np.array([b[k] for b in bands], dtype=np.int32)
    for k in ('dt', 'a'):
        out[k] = np.array([b[k] for b in bands], dtype=f32)
    return out


def band_state(b):
    """the reference state of such a band (its words taken as exact)"""
    st = new_state(b['n_img'], b['n'])
    st.update(converged=bool(b['converged']), climbing=bool(b['climbing']), n_steps=int(b['n_steps']), n_pos=int(b['n_pos']),
              dt=float(b['dt']), a=float(b['a']), vel=np.asarray(b['vel'], dtype=np.float64))
    return st


def band_step(b, flags=0, eps=EPS32):
    """neb_step of such a band with the synthetic parameters"""
    return neb_step(b['x'], b['F'], b['E'], b['free'], band_state(b), params(SYN_SPRING, SYN_FMAX, SYN_CLIMB_BELOW), flags, eps)
