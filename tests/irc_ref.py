"""fp64 statement of one nnhip_irc_step launch (csrc/irc.hip) for ONE molecule, for the tests (numpy), with a per-element rounding
bound, in the manner of tests/relax_ref.py and tests/neb_ref.py; the same chain in float32; and the whole method as a host loop.

The kernel's chain (every line ONE fp32 operation per element; dot3(a, b) = fma(az, bz, fma(ay, by, ax bx)); sum_l = lane-local sum
in atom order over the FREE atoms, lane l owning the atoms l, l + 64, ..., then the butterfly 32, 16, ..., 1; c = ACCEL):
    f = F (free) or 0 (fixed);  fmax2 = max_i dot3(f_i, f_i);  fmax = sqrt(fmax2);  armed |= fmax2 >= tol2   (status == 0 only)
    P = sum_l dot3(f, vel);  status = 2 if n_steps >= 1 and P < 0, else 1 if armed and fmax2 < tol2   (status == 0, not CHECK_ONLY)
    frozen (status != 0 | no atoms | CHECK_ONLY):  x_out = x, nothing else
    a = (c f) / m;   n_steps >= 1:  w = fma(0.5 (a_prev + a), dt_prev, vel);  nv = sqrt(sum_l dot3(w, w));
                                    v = w (v0 / nv) if nv > 0 else vel            n_steps == 0:  v = vel
    x_out = fma(a, (0.5 dt) dt, fma(v, dt, x));   d = x_out - x;   arc += sqrt(sum_l m dot3(d, d))   (a lane adds by fma(m, dot3, acc))
    n_steps >= 1:  T = dt_prev + dt;  p = fma(a_prev, (0.5 T) T, fma(v_prev, T, x_prev));  e = x_out - p;  Delta = sqrt(sum_l dot3(e, e))
                   Delta > 0:  dt_next = min(max(min(max(dt cbrt(delta0 / Delta), 0.5 dt), 2 dt), dt_min), dt_max);  else dt_next = dt
    x_prev = x;  v_prev = vel = v;  a_prev = a;  dt_prev = dt;  dt = dt_next;  n_steps += 1

`irc_step` evaluates that in fp64 from the SAME fp32 inputs and state and carries a first-order bound next to every value: an
operation with exact result r adds eps |r| (eps = EPS32 = 2^-24, one rounding to nearest), the bounds of its operands pass through
multiplied by the magnitudes of the other operands.  A square root or a cube root adds ROOT_ULPS = 2 ulp = 4 eps |r| instead: they
are not taken as correctly rounded.  A reduction whose terms pass through at most `depth` roundings costs (depth + 1) eps sum |term|
plus the propagated operand bounds; a dot product over n atoms has depth 3 (product, two fmas) + ceil(n / 64) (lane-local adds) + 6
(butterfly).  min and max are exact and pass the bound of their argument through.

C_IRC = 2 multiplies the first-order sum at the outputs, for what first order leaves out (products of two roundings, magnitudes
taken from the fp64 values); it is chosen before any run.  Results below the normal range add TINY32.

The decisions of a step are reported as AMBIGUOUS when the fp64 value lies within C_IRC x its own bound of the threshold -- `turn`
(P < 0), `stop` and `arm` (fmax2 against tol2), `vzero` (nv > 0; exact zeros on both sides are not ambiguous).  One more decision, Delta > 0, touches dt_next alone: a sum
of squares vanishes only when every term does, so the kernel's Delta can be 0 only where NO component of e is provably non-zero;
the step is then checked all the same, and dt_next may be either the bounded value or dt itself (`dt_alt`).
The bound of dt_next is not first order: it is the range of the clamped cube-root law over Delta -+ C_IRC x the bound of Delta, so a
clamp that holds over that whole range leaves no error but the last roundings.  The kernel may decide such a case either
way, and a test either constructs inputs without one (and says so) or skips and counts it."""
import math

import numpy as np

EPS32 = 2.0 ** -24
C_IRC = 2.0
ROOT_ULPS = 2.0
TINY32 = float(np.finfo(np.float32).tiny)
CHECK_ONLY = 1
ACCEL = 0.00964853322                                    # NNHIP_IRC_ACCEL: eV / (Angstrom amu) in Angstrom / fs^2
ACCEL32 = float(np.float32(ACCEL))
ARRAYS = ('vel', 'x_prev', 'v_prev', 'a_prev')
SCALARS = ('dt', 'dt_prev', 'arc')
INTS = ('status', 'armed', 'n_steps')


def half_ulp32(a):
    """half an fp32 ulp of |a| (the stored value's own rounding), fp64"""
    return 0.5 * np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def parameters(speed=0.02, error_target=1.5e-3, timestep_min=0.01, timestep_max=2.0, fmax=0.01):
    """the scalars of a launch as the Python floats of their fp32 values (tol2 = fl32(fl32(fmax)^2) as the driver forms it)"""
    f32 = np.float32
    return dict(v0=float(f32(speed)), delta0=float(f32(error_target)), dt_min=float(f32(timestep_min)),
                dt_max=float(f32(timestep_max)), tol2=float(f32(fmax * fmax)))


def new_state(vel, dt, arc=0.0):
    """the state of a molecule before its first step: the start velocity (norm v0), the first time step, the arc length so far"""
    vel = np.asarray(vel, dtype=np.float64)
    z = np.zeros_like(vel)
    return dict(status=0, armed=0, n_steps=0, dt=float(dt), dt_prev=0.0, arc=float(arc), vel=vel.copy(), x_prev=z.copy(),
                v_prev=z.copy(), a_prev=z.copy())


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def masked(F, free):
    F = np.asarray(F, dtype=np.float64)
    return F if free is None else np.where(np.asarray(free, dtype=bool)[:, None], F, 0.0)


def dot_depth(n):
    return 3 + (n + 63) // 64 + 6


def _sum(t, bt, n, extra, eps):
    """sum of the terms t (each through 3 + extra roundings of its own, bound bt from its operands) over a molecule of n atoms"""
    return float(t.sum()), (dot_depth(n) + extra + 1) * eps * float(np.abs(t).sum()) + float(np.sum(bt))


def _sqrt(v, bv, eps):
    r = math.sqrt(max(v, 0.0))
    return r, (bv / (2.0 * r) if r > 0 else math.sqrt(bv)) + 2.0 * ROOT_ULPS * eps * r


def irc_step(x, F, free, mass, st, par, flags=0, eps=EPS32, decide=None):
    """One launch for one molecule.  x, F [n,3], mass [n]: the fp32 values the kernel gets; free: bool [n] or None; st: the state
    (new_state; not modified); par: parameters().  Returns a dict:
      x_out, bx [n,3]     fp64 positions and their bound (C_IRC x first order + TINY32); frozen molecules and fixed atoms: x, 0
      vel, bv; acc, ba    the damped velocity and the acceleration stored for the next step, with bounds
      dt_next, b_dt; arc, b_arc; fmax, b_fmax
      state               the state after the step
      frozen, zero_v (|v| == 0 was met), step (the mass-weighted length of this step)
      ambiguous           dict(turn, stop, arm, vzero) of bools
      dt_alt              None, or the other value dt_next may take: dt itself, where Delta may vanish in the kernel (below)
    decide: None, or dict(status=, armed=) with what the kernel decided, to follow instead of the fp64 decisions"""
    x, f = np.asarray(x, dtype=np.float64), masked(F, free)
    mass = np.asarray(mass, dtype=np.float64)
    n = x.shape[0]
    fr = np.ones(n, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    frc = fr[:, None]
    v0, delta0, dt_min, dt_max, tol2 = (float(par[k]) for k in ('v0', 'delta0', 'dt_min', 'dt_max', 'tol2'))
    amb = dict(turn=False, stop=False, arm=False, vzero=False)
    may_vanish = False
    steps, dt, dt_prev = st['n_steps'], float(st['dt']), float(st['dt_prev'])
    finish = steps >= 1
    vel = np.where(frc, st['vel'], 0.0)
    n2 = (f * f).sum(1)
    fmax2 = float(n2.max()) if n else 0.0
    b_fmax2 = 4.0 * eps * fmax2
    fmax, b_fmax = _sqrt(fmax2, b_fmax2, eps)
    near_tol = abs(fmax2 - tol2) <= C_IRC * b_fmax2 and (b_fmax2 > 0 or fmax2 != tol2)
    new = copy_state(st)
    status = st['status']
    if status == 0:
        armed = bool(st['armed']) or fmax2 >= tol2
        amb['arm'] = (not st['armed']) and near_tol
        if decide is not None and 'armed' in decide:
            armed = bool(decide['armed'])
        new['armed'] = int(armed)
        if not (flags & CHECK_ONLY):
            now = 0
            P, b_P = _sum((f * vel).sum(1), 0.0, n, 0, eps)
            if finish:
                amb['turn'] = abs(P) <= C_IRC * b_P and b_P > 0
            if finish and P < 0:
                now = 2
            elif armed and fmax2 < tol2:
                now = 1
            if armed and not (finish and P < 0):
                amb['stop'] = near_tol
            if decide is not None and 'status' in decide:
                now = int(decide['status'])
            status = now
            new['status'] = now
    out = dict(fmax=fmax, b_fmax=C_IRC * b_fmax + TINY32, ambiguous=amb, zero_v=False, step=0.0, dt_alt=None)
    if status != 0 or n == 0 or (flags & CHECK_ONLY):
        out.update(x_out=x.copy(), bx=np.zeros_like(x), vel=st['vel'].copy(), bv=np.zeros_like(x), acc=st['a_prev'].copy(),
                   ba=np.zeros_like(x), dt_next=dt, b_dt=0.0, arc=st['arc'], b_arc=0.0, state=new, frozen=True)
        return out
    msafe = np.where(fr, mass, 1.0)[:, None]
    a = ACCEL32 * f / msafe
    ba = 2.0 * eps * np.abs(a)
    if finish:
        a_prev = np.where(frc, st['a_prev'], 0.0)
        s = a_prev + a
        bs = ba + eps * np.abs(s)
        w = vel + 0.5 * s * dt_prev
        bw = 0.5 * dt_prev * bs + eps * np.abs(w)
        vv, b_vv = _sum((w * w).sum(1), 2.0 * (np.abs(w) * bw).sum(1), n, 0, eps)
        nv, b_nv = _sqrt(vv, b_vv, eps)
        amb['vzero'] = nv <= C_IRC * b_nv and b_nv > 0
        if nv > 0:
            scale = v0 / nv
            b_scale = scale * b_nv / nv + eps * scale
            v = w * scale
            bv = scale * bw + np.abs(w) * b_scale + eps * np.abs(v)
        else:
            v, bv = vel.copy(), np.zeros_like(vel)
            out['zero_v'] = True
    else:
        v, bv = vel.copy(), np.zeros_like(vel)
    h = 0.5 * dt * dt
    t1 = x + v * dt
    b1 = dt * bv + eps * np.abs(t1)
    x_out = t1 + a * h
    bx = b1 + np.abs(a) * (eps * h) + h * ba + eps * np.abs(x_out)
    x_out, bx = np.where(frc, x_out, x), np.where(frc, bx, 0.0)
    d = x_out - x
    bd = np.where(frc, bx + eps * np.abs(d), 0.0)
    mf = np.where(fr, mass, 0.0)
    M, b_M = _sum(mf * (d * d).sum(1), mf * 2.0 * (np.abs(d) * bd).sum(1), n, 1, eps)
    ds, b_ds = _sqrt(M, b_M, eps)
    arc = st['arc'] + ds
    b_arc = b_ds + eps * abs(arc)
    dt_next, b_dt = dt, 0.0
    if finish:
        T = dt_prev + dt
        b_T = eps * T
        g = 0.5 * T * T
        b_g = T * b_T + eps * g
        x_prev, v_prev = np.where(frc, st['x_prev'], 0.0), np.where(frc, st['v_prev'], 0.0)
        t = x_prev + v_prev * T
        bt = np.abs(v_prev) * b_T + eps * np.abs(t)
        p = t + a_prev * g
        bp = bt + np.abs(a_prev) * b_g + eps * np.abs(p)
        e = np.where(frc, x_out - p, 0.0)
        be = np.where(frc, bx + bp + eps * np.abs(e), 0.0)
        D2, b_D2 = _sum((e * e).sum(1), 2.0 * (np.abs(e) * be).sum(1), n, 0, eps)
        delta, b_delta = _sqrt(D2, b_D2, eps)
        # dt_next is a clamped function of Delta: its bound is the function's range over Delta -+ C_IRC b_delta (a saturated clamp
        # has none) plus the three roundings behind Delta (quotient, cube root at ROOT_ULPS, product)
        def dt_of(dl):
            if dl <= 0:
                return min(max(2.0 * dt, dt_min), dt_max)
            return min(max(min(max(dt * (delta0 / dl) ** (1.0 / 3.0), 0.5 * dt), 2.0 * dt), dt_min), dt_max)
        lo, hi = delta - C_IRC * b_delta, delta + C_IRC * b_delta
        # the kernel's Delta is exactly 0 only when every component of e is: ambiguous when none of them is provably not
        may_vanish = b_delta > 0 and bool(np.all(np.abs(e) <= C_IRC * be))
        if delta > 0:
            dt_next = dt_of(delta)
            b_dt = max(abs(dt_of(lo) - dt_next), abs(dt_of(hi) - dt_next)) + C_IRC * (2.0 + 2.0 * ROOT_ULPS) * eps * dt_next
    new.update(vel=v.copy(), x_prev=x.copy(), v_prev=v.copy(), a_prev=a.copy(), dt_prev=dt, dt=dt_next, arc=arc, n_steps=steps + 1)
    for k in ARRAYS:
        new[k] = np.where(frc, new[k], st[k])             # a fixed atom's rows are not written

    def cb(b):
        return np.where(np.asarray(b) > 0, C_IRC * np.asarray(b) + TINY32, 0.0)
    out.update(x_out=x_out, bx=cb(bx), vel=new['vel'], bv=cb(np.where(frc, bv, 0.0)), acc=new['a_prev'], ba=cb(np.where(frc, ba, 0.0)),
               dt_next=dt_next, b_dt=b_dt + (TINY32 if b_dt > 0 else 0.0), dt_alt=dt if may_vanish else None, arc=arc, b_arc=float(cb(b_arc)), state=new, frozen=False, step=ds)
    return out


# ---- the same chain in numpy float32, in the kernel's order of operations -----------------------------------------------------------

def _fma32(a, b, c):
    # (a b is exact in fp64 for fp32 operands; the sum rounds to fp64 and then to fp32 -- a double rounding that differs from a
    # true fma in rare ties only, far inside every bound here)
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def _dot3_32(a, b):
    return _fma32(a[:, 2], b[:, 2], _fma32(a[:, 1], b[:, 1], (a[:, 0] * b[:, 0]).astype(np.float32)))


def _wave_sum32(t, fr, weight=None):
    """lane l adds the FREE atoms l, l + 64, ... in that order (t [n] fp32; with `weight` by fma(weight, t, acc)), then the butterfly"""
    acc = np.zeros(64, dtype=np.float32)
    for i0 in range(0, t.shape[0], 64):
        chunk, keep = t[i0:i0 + 64], fr[i0:i0 + 64]
        k = chunk.shape[0]
        new = (acc[:k] + chunk).astype(np.float32) if weight is None else _fma32(weight[i0:i0 + 64], chunk, acc[:k])
        acc[:k] = np.where(keep, new, acc[:k])
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[lanes ^ d]).astype(np.float32)
    return acc[0]


def emulate_step(x, F, free, mass, st, par, flags=0):
    """irc_step in float32 arithmetic, operation for operation as the kernel orders them.  Same state dict (its arrays are read as
    float32); returns (x_out float32, fmax float32, new state with float32-valued entries)."""
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    f = masked(F, free).astype(f32)
    mass = np.asarray(mass, dtype=f32)
    n = x.shape[0]
    fr = np.ones(n, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    frc = fr[:, None]
    v0, delta0, dt_min, dt_max, tol2 = (f32(par[k]) for k in ('v0', 'delta0', 'dt_min', 'dt_max', 'tol2'))
    new = copy_state(st)
    steps, dt, dt_prev = st['n_steps'], f32(st['dt']), f32(st['dt_prev'])
    finish = steps >= 1
    vel, a_prev = st['vel'].astype(f32), st['a_prev'].astype(f32)
    fmax2 = _dot3_32(f, f).max() if n else f32(0)
    fmax = np.sqrt(fmax2, dtype=f32)
    status = st['status']
    if status == 0:
        new['armed'] = int(bool(st['armed']) or fmax2 >= tol2)
        if not (flags & CHECK_ONLY):
            P = _wave_sum32(_dot3_32(f, vel), fr)
            if finish and P < 0:
                status = 2
            elif new['armed'] and fmax2 < tol2:
                status = 1
            new['status'] = status
    if status != 0 or n == 0 or (flags & CHECK_ONLY):
        return x.copy(), fmax, new
    msafe = np.where(fr, mass, f32(1))[:, None]
    a = ((f32(ACCEL) * f).astype(f32) / msafe).astype(f32)
    v = vel
    if finish:
        w = _fma32((f32(0.5) * (a_prev + a).astype(f32)).astype(f32), dt_prev, vel)
        nv = np.sqrt(_wave_sum32(_dot3_32(w, w), fr), dtype=f32)
        if nv > 0:
            v = (w * f32(v0 / nv)).astype(f32)
    h = f32(f32(f32(0.5) * dt) * dt)
    x_out = np.where(frc, _fma32(a, h, _fma32(v, dt, x)), x)
    d = (x_out - x).astype(f32)
    ds = np.sqrt(_wave_sum32(_dot3_32(d, d), fr, weight=mass), dtype=f32)
    dt_next = dt
    if finish:
        T = f32(dt_prev + dt)
        g = f32(f32(f32(0.5) * T) * T)
        p = _fma32(a_prev, g, _fma32(st['v_prev'].astype(f32), T, st['x_prev'].astype(f32)))
        e = (x_out - p).astype(f32)
        delta = np.sqrt(_wave_sum32(_dot3_32(e, e), fr), dtype=f32)
        if delta > 0:
            with np.errstate(over='ignore', divide='ignore'):
                dt_next = f32(dt * np.cbrt(f32(delta0 / delta)))
            dt_next = min(max(dt_next, f32(f32(0.5) * dt)), f32(f32(2) * dt))
            dt_next = min(max(dt_next, dt_min), dt_max)
    upd = dict(vel=v, x_prev=x, v_prev=v, a_prev=a)
    for k in ARRAYS:
        new[k] = np.where(frc, upd[k].astype(np.float64), st[k])
    new.update(dt_prev=float(dt), dt=float(dt_next), arc=float(f32(f32(st['arc']) + ds)), n_steps=steps + 1)
    return x_out.astype(f32), fmax, new


# ---- the whole method as a host fp64 loop (the yardstick of the path tests) ------------------------------------------------------------

def mass_norm(u, mass):
    """|M^1/2 u| of u [n,3]"""
    return math.sqrt(float((np.asarray(mass)[:, None] * np.asarray(u, dtype=np.float64) ** 2).sum()))


def orient(u):
    """u with its sign fixed: the component of largest magnitude (the lowest index at a tie) is positive"""
    u = np.asarray(u, dtype=np.float64)
    flat = u.reshape(-1)
    return -u if flat.size and flat[int(np.argmax(np.abs(flat)))] < 0 else u.copy()


def start(x_saddle, u, mass, sign, displacement, speed):
    """the start of one branch: x_0 = x_saddle + sign displacement u / |M^1/2 u|,  vel = sign speed u / |u|  (u: the Cartesian
    direction M^-1/2 q, zero on fixed atoms)"""
    u = np.asarray(u, dtype=np.float64)
    return (np.asarray(x_saddle, dtype=np.float64) + sign * displacement * u / mass_norm(u, mass),
            sign * speed * u / math.sqrt(float((u * u).sum())))


def follow(energy_forces, x0, vel0, mass, mol_ptr, arc0=0.0, speed=0.02, error_target=1.5e-3, timestep=0.25, timestep_min=0.01,
           timestep_max=2.0, fmax=0.01, max_steps=1000, free=None):
    """The contract above as a plain fp64 loop over a batch: energy_forces(x [N,3] fp64) -> (E [B], F [N,3]); x0, vel0: the start
    positions and velocities of every path (start()).  The scalars are used as given, in fp64.  Returns dict(x, energy, fmax,
    status, n_steps, arc, max_step (the largest single mass-weighted step per molecule), zero_v, traj_pos, traj_energy, traj_arc:
    lists over the steps taken, entry k the state BEFORE step k + 1, the last one the end)."""
    x = np.asarray(x0, dtype=np.float64).copy()
    mass = np.asarray(mass, dtype=np.float64)
    B = len(mol_ptr) - 1
    sl = [slice(int(mol_ptr[b]), int(mol_ptr[b + 1])) for b in range(B)]
    par = dict(v0=speed, delta0=error_target, dt_min=timestep_min, dt_max=timestep_max, tol2=fmax * fmax)
    states = [new_state(np.asarray(vel0, dtype=np.float64)[s], timestep, arc0) for s in sl]
    fr = [None if free is None else np.asarray(free, dtype=bool)[s] for s in sl]
    max_step, zero_v = np.zeros(B), 0
    tp, te, ta = [], [], []
    for k in range(max_steps + 1):
        E, F = energy_forces(x)
        E, F = np.asarray(E, dtype=np.float64), np.asarray(F, dtype=np.float64)
        tp.append(x.copy())
        te.append(E.copy())
        ta.append(np.array([st['arc'] for st in states]))
        last = k == max_steps
        fm = np.zeros(B)
        for b, s in enumerate(sl):
            r = irc_step(x[s], F[s], fr[b], mass[s], states[b], par, CHECK_ONLY if last else 0, eps=0.0)
            x[s], states[b], fm[b] = r['x_out'], r['state'], r['fmax']
            max_step[b] = max(max_step[b], r['step'])
            zero_v += r['zero_v']
        if all(st['status'] != 0 for st in states):
            break
    return dict(x=x, energy=E, fmax=fm, status=np.array([st['status'] for st in states]),
                n_steps=np.array([st['n_steps'] for st in states]), arc=np.array([st['arc'] for st in states]), max_step=max_step,
                zero_v=zero_v, traj_pos=tp, traj_energy=te, traj_arc=ta)


# ---- the Mueller-Brown surface in two coordinates of a two-atom "molecule" -------------------------------------------------------------

MB_A = np.array([-200.0, -100.0, -170.0, 15.0])
MB_a = np.array([-1.0, -1.0, -6.5, 0.7])
MB_b = np.array([0.0, 0.0, 11.0, 0.6])
MB_c = np.array([-10.0, -10.0, -6.5, 0.7])
MB_X = np.array([1.0, 0.0, -0.5, -1.0])
MB_Y = np.array([0.0, 0.5, 1.5, 1.0])
MB_MASS = np.array([1.008, 12.011])
MB_MINIMA = np.array([[-0.5582236346, 1.4417258418], [-0.0500108229, 0.4666941049], [0.6234994049, 0.0280377585]])
MB_SADDLE_GUESSES = np.array([[-0.822, 0.624], [0.212, 0.293]])


def mb(X, Y):
    """(energy, dE/dX, dE/dY) of the Mueller-Brown surface, its numbers read as eV and Angstrom"""
    dx, dy = X - MB_X, Y - MB_Y
    t = MB_A * np.exp(MB_a * dx * dx + MB_b * dx * dy + MB_c * dy * dy)
    return float(t.sum()), float((t * (2 * MB_a * dx + MB_b * dy)).sum()), float((t * (MB_b * dx + 2 * MB_c * dy)).sum())


def mb_energy_forces(x):
    """the surface on X = x[0, 0], Y = x[1, 0] of a two-atom molecule [2,3]; the other four coordinates feel nothing"""
    E, gx, gy = mb(x[0, 0], x[1, 0])
    F = np.zeros((2, 3))
    F[0, 0], F[1, 0] = -gx, -gy
    return np.array([E]), F


def mb_hessian(X, Y, h=1e-5):
    H = np.zeros((2, 2))
    for k, (ex, ey) in enumerate(((h, 0.0), (0.0, h))):
        gp, gm = mb(X + ex, Y + ey)[1:], mb(X - ex, Y - ey)[1:]
        H[:, k] = (np.array(gp) - np.array(gm)) / (2 * h)
    return 0.5 * (H + H.T)


def mb_saddle(k):
    """saddle k (Newton on the gradient from the textbook position) as x [2,3] and its Cartesian direction u [2,3] = M^-1/2 q, q the
    lowest mode of the mass-weighted Hessian, oriented"""
    X, Y = MB_SADDLE_GUESSES[k]
    for _ in range(50):
        g = np.array(mb(X, Y)[1:])
        X, Y = np.array([X, Y]) - np.linalg.solve(mb_hessian(X, Y), g)
    isq = 1.0 / np.sqrt(MB_MASS)
    lam, vec = np.linalg.eigh(mb_hessian(X, Y) * np.outer(isq, isq))
    assert lam[0] < 0 < lam[1]
    x, u = np.zeros((2, 3)), np.zeros((2, 3))
    x[0, 0], x[1, 0] = X, Y
    u[0, 0], u[1, 0] = vec[:, 0] * isq
    return x, orient(u)


def mb_fine_path(x0, ds=2e-4, max_steps=200000, gtol=1e-4):
    """fp64 mass-weighted steepest descent from x0 [2,3] in steps of ds amu^1/2 (midpoint rule): dq/ds = -g_q / |g_q| with q = M^1/2
    x, g_q = M^-1/2 g; ends where |g| < gtol or the energy would rise.  Returns the points [K,2] in (X, Y)."""
    sq = np.sqrt(MB_MASS)
    q = np.array([x0[0, 0], x0[1, 0]]) * sq

    def direction(q):
        E, gx, gy = mb(*(q / sq))
        g = np.array([gx, gy])
        gq = g / sq
        return E, g, -gq / np.linalg.norm(gq)
    pts = [q / sq]
    E, g, t = direction(q)
    for _ in range(max_steps):
        if np.linalg.norm(g) < gtol:
            break
        _, _, tm = direction(q + 0.5 * ds * t)
        qn = q + ds * tm
        En, g, tn = direction(qn)
        if En > E:
            break
        q, E, t = qn, En, tn
        pts.append(q / sq)
    return np.array(pts)


def distance_to_path(points, path):
    """for every point [K,2] the distance to the nearest vertex of path [L,2]"""
    out = np.empty(len(points))
    for k, p in enumerate(points):
        out[k] = np.sqrt(((path - p) ** 2).sum(1).min())
    return out


# ---- synthetic kernel inputs: every branch of a launch at every size class (shared by the host and the GPU tests) ---------------------

SYN_SIZES = (1, 2, 21, 63, 64, 65, 200, 21, 65)           # nine molecules: more than two workgroups' waves
SYN_KINDS = ('first', 'ordinary', 'grow_max', 'shrink_min', 'cap2', 'turned', 'stop_armed', 'below_unarmed', 'stopped', 'vzero')
SYN_MASSES = np.array([1.008, 12.011, 15.999], dtype=np.float32)
SENT = 7.0


def synthetic_batch(kind, seed=0):
    """Nine molecules of SYN_SIZES atoms of H / C / O masses with an empty molecule in the middle, all of one kind:
      first          n_steps = 0, armed = 0, forces ~0.5 eV/A, the unused state words hold 7.0
      ordinary       n_steps = 5, dt = 0.25, dt_prev = 0.2, Delta ~ 0.7 Delta0 (dt grows by ~1.13)
      grow_max       dt = 1.5, Delta ~ Delta0 / 4: the growth by ~1.6 ends at dt_max = 2;   cap2: dt = 0.25, Delta ~ Delta0 / 20: 2 dt
                     (both with forces of ~1e-4 eV/A and not armed, so that the step's own Delta stays far below those)
      shrink_min     dt = 0.015, Delta ~ 8 Delta0: half of dt would be below dt_min = 0.01
      turned         the stored velocity points against the forces: P < 0
      stop_armed     armed, the largest force 0.005 < 0.01, P > 0: status 1;   below_unarmed: the same forces, not armed: it moves on
      stopped        status 1 or 2, large forces: every bit stays
      vzero          F = 0, vel = 0, a_prev = 0, not armed: |v| = 0 exactly (in fp64 as well), nothing may divide, nothing moves
    In every kind but `turned` the velocity has a large component along the forces (P > 0 by a wide margin); about a quarter of the
    atoms of every second molecule of >= 2 atoms are fixed, and hold NaN masses, velocities and state rows the kernel may not read
    into any result.  Returns a dict of numpy arrays in the kernel's layout and types."""
    rng = np.random.default_rng([seed, SYN_KINDS.index(kind)])
    f32 = np.float32
    par = parameters()
    v0, delta0 = par['v0'], par['delta0']
    mols = []
    for j, n in enumerate(SYN_SIZES):
        free = np.ones(n, dtype=bool)
        if n >= 2 and j % 2:
            free = rng.random(n) >= 0.25
            free[rng.integers(n)] = True
        frc = free[:, None]
        mass = SYN_MASSES[rng.integers(0, 3, n)]
        x = rng.uniform(-8, 8, (n, 3)).astype(f32)
        F = rng.normal(0, 0.5, (n, 3)).astype(f32)
        if kind in ('stop_armed', 'below_unarmed'):
            F = (F.astype(np.float64) * (0.005 / np.sqrt((masked(F, free) ** 2).sum(1).max()))).astype(f32)
        if kind in ('grow_max', 'cap2'):                  # (forces so small that the step's own Delta stays far below the target)
            F = (F * f32(2e-4)).astype(f32)
        f = masked(F, free)
        dirn = f / np.linalg.norm(f) * (-1.0 if kind == 'turned' else 1.0)
        if kind == 'vzero':
            F = np.zeros((n, 3), dtype=f32)
        noise = rng.normal(0, 1, (n, 3)) * frc
        dirn = 0.8 * dirn + 0.6 * noise / max(np.linalg.norm(noise), 1e-30) * (kind != 'turned')
        vel = (v0 * dirn / np.linalg.norm(dirn)).astype(f32)
        status, armed, n_steps, dt, dt_prev = 0, 1, 5, 0.25, 0.2
        target = 0.7 * delta0
        if kind == 'first':
            armed, n_steps = 0, 0
        elif kind == 'grow_max':
            armed, dt, dt_prev, target = 0, 1.5, 1.0, delta0 / 4
        elif kind == 'cap2':
            armed, target = 0, delta0 / 20
        elif kind == 'shrink_min':
            dt, dt_prev, target = 0.015, 0.03, 8 * delta0
        elif kind in ('below_unarmed', 'vzero'):
            armed = 0
        elif kind == 'stopped':
            status = 1 + j % 2
        dt, dt_prev = float(f32(dt)), float(f32(dt_prev))
        a_n = (f32(ACCEL) * masked(F, free).astype(f32)).astype(f32) / np.where(free, mass, f32(1))[:, None]
        if kind == 'vzero':
            vel = np.zeros((n, 3), dtype=f32)
            a_prev = np.zeros((n, 3), dtype=f32)
        else:
            a_prev = (a_n.astype(np.float64) * (1 + 0.2 * rng.normal(0, 1, (n, 3)))).astype(f32)
        v_prev = vel.copy()
        shift = rng.normal(0, 1, (n, 3)) * frc
        shift *= target / np.linalg.norm(shift)
        x_prev = (x.astype(np.float64) - v_prev * dt_prev - 0.5 * a_prev * dt_prev ** 2 + shift).astype(f32)
        arc = f32(rng.uniform(0.1, 3.0))
        if kind == 'first':
            a_prev, v_prev, x_prev = (np.full((n, 3), SENT, dtype=f32) for _ in range(3))
            dt_prev = SENT
        mass = mass.copy()
        for arr in (mass, vel, a_prev, v_prev, x_prev):
            arr[~free] = np.nan
        mols.append(dict(n=n, free=free, mass=mass, x=x, F=F, vel=vel, a_prev=a_prev, v_prev=v_prev, x_prev=x_prev, status=status,
                         armed=armed, n_steps=n_steps, dt=dt, dt_prev=dt_prev, arc=arc))
    z3 = np.zeros((0, 3), f32)
    empty = dict(n=0, free=np.ones(0, dtype=bool), mass=np.zeros(0, f32), x=z3, F=z3, vel=z3, a_prev=z3, v_prev=z3, x_prev=z3, status=0,
                 armed=0, n_steps=3, dt=0.25, dt_prev=0.25, arc=f32(0.5))
    mols = mols[:4] + [empty] + mols[4:]
    out = dict(ptr=np.concatenate([[0], np.cumsum([q['n'] for q in mols])]).astype(np.int32), kind=kind, par=par)
    for k in ('x', 'F', 'free', 'mass') + ARRAYS:
        out[k] = np.concatenate([q[k] for q in mols])
    for k in INTS:
        out[k] = np.array([q[k] for q in mols], dtype=np.int32)
    for k in SCALARS:
        out[k] = np.array([q[k] for q in mols], dtype=f32)
    return out


def batch_state(d, b):
    """the reference state of molecule b of a batch in the kernel's layout"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    st = {k: int(d[k][b]) for k in INTS}
    st.update({k: float(d[k][b]) for k in SCALARS})
    st.update({k: d[k][a0:a1].astype(np.float64) for k in ARRAYS})
    return st


def batch_step(d, b, flags=0, use_mask=True, emulate=False):
    """irc_step (or emulate_step) of molecule b of such a batch"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    fn = emulate_step if emulate else irc_step
    return fn(d['x'][a0:a1], d['F'][a0:a1], d['free'][a0:a1] if use_mask else None, d['mass'][a0:a1], batch_state(d, b), d['par'], flags)


def unmasked(d):
    """the batch with every atom free: the NaN rows of the fixed atoms become atoms at rest (carbon mass, no velocity, no previous
    acceleration, x_prev = x), which leave each kind what its name says"""
    out = dict(d, free=np.ones_like(d['free']))
    fixed = ~d['free']
    out['mass'] = np.where(fixed, SYN_MASSES[1], d['mass']).astype(np.float32)
    for k in ARRAYS:
        fill = d['x'] if k == 'x_prev' else np.float32(0)
        out[k] = np.where(fixed[:, None] & np.isnan(d[k]), fill, d[k]).astype(np.float32)
    return out


def compare(ref, x_out, fmax, new, x, what='', skip=()):
    """err / bound of one molecule's outputs (x_out, fmax and the state `new`, float32-valued) against irc_step's `ref`; asserts
    every one <= 1 and returns them as a dict; skip: names (of fmax, pos, vel, acc, dt, arc) the caller has no value of"""
    worst = {}

    def one(name, got, want, bound):
        if name in skip:
            return
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        b = np.asarray(bound, dtype=np.float64) + half_ulp32(want)
        ok = np.isfinite(want)
        r = float((np.abs(got - want)[ok] / b[ok]).max()) if ok.any() else 0.0
        assert r <= 1.0, f'{what}: {name} err / bound {r:.3f}'
        worst[name] = r
    one('fmax', fmax, ref['fmax'], ref['b_fmax'])
    if ref['frozen']:
        return worst
    one('pos', x_out, ref['x_out'], ref['bx'])
    one('vel', new['vel'], ref['vel'], ref['bv'])
    one('acc', new.get('a_prev'), ref['acc'], ref['ba'])
    if ref['dt_alt'] is None or float(new['dt']) != ref['dt_alt']:
        one('dt', new['dt'], ref['dt_next'], ref['b_dt'])
    one('arc', new['arc'], ref['arc'], ref['b_arc'])
    return worst


def main():
    """the emulation against the fp64 statement on every synthetic batch: the worst err / bound (it must be below 1 before any
    run of the kernel) and the share of ambiguous molecule-steps (at most 1 %)"""
    worst, total, ambiguous = {}, 0, 0
    for kind in SYN_KINDS:
        for use_mask in (True, False):
            d = synthetic_batch(kind)
            d = d if use_mask else unmasked(d)
            for flags in (0, CHECK_ONLY):
                for b in range(len(d['ptr']) - 1):
                    ref = batch_step(d, b, flags, use_mask)
                    x_out, fmax, new = batch_step(d, b, flags, use_mask, emulate=True)
                    total += 1
                    if any(ref['ambiguous'].values()):
                        ambiguous += 1
                        continue
                    for k in INTS:
                        assert new[k] == ref['state'][k], (kind, use_mask, flags, b, k, new[k], ref['state'][k])
                    a0 = int(d['ptr'][b])
                    w = compare(ref, x_out, fmax, new, d['x'][a0:a0 + x_out.shape[0]], f'{kind} mask {use_mask} flags {flags} molecule {b}')
                    for k, v in w.items():
                        worst[k] = max(worst.get(k, 0.0), v)
    print(f'emulation against fp64, {total} molecule-steps, {ambiguous} ambiguous ({100.0 * ambiguous / total:.2f} %): worst err / '
          f'bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f' (C_IRC = {C_IRC})')
    assert ambiguous <= 0.01 * total and max(worst.values()) < 1.0
    return worst, total, ambiguous


if __name__ == '__main__':
    main()
