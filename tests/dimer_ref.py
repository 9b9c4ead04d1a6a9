"""fp64 statement of one nnhip_dimer_step launch (csrc/dimer.hip) for ONE molecule, for the tests (numpy), with a per-element
rounding bound, in the manner of tests/relax_ref.py and tests/irc_ref.py; the whole method as a host fp64 loop (`search`); and a
numpy-float32 emulation of the chain.  `python -m tests.dimer_ref` prints the emulation's worst err / bound per output group.

The chain is written ONCE (`_dimer_step`), over an arithmetic A that is one of
  Bound   fp64 values, each carrying a first-order bound: an operation with exact result r adds eps |r| (eps = EPS32 = 2^-24, one
          rounding to nearest -- the device forms its angles from sums, products, quotients and correctly rounded square roots
          alone, so no operation needs more), and the bounds of its operands pass through multiplied by the magnitudes of the other
          operands.  A sum over the atoms whose terms pass through at most `depth` roundings costs (depth + 1) eps sum |term| plus
          the propagated operand bounds (relax_ref.dot_depth).  eps = 0 gives the plain fp64 method (what `search` runs).
  Emu32   numpy float32, operation for operation in the kernel's order (lane-local sums in atom order, then the butterfly).
The translation is relax_ref's L-BFGS step on (center, F+): through the two-loop recursion the bound travels by the recursion's
own linear map (relax_ref._two_loop).  That step takes its force as exact, so a translation is checked in two stages: the F+ the
kernel stored (its row F_PREV) against the fp64 F+ and its bound, and the step from THAT stored F+ (`ft_stored`) -- as relax_ref
checks S[head] from the kernel's own x_out.

C_DM = 2 multiplies the first-order sum at the outputs, for what first order leaves out, as C_RX does; results below the normal
range add TINY32.  Every decision of a launch -- convergence, rotation done (tolerance), the D.G <= 0 reset, beta clipped at 0,
which sign the curvature has, pair accepted, clamp -- is reported AMBIGUOUS when its fp64 value lies within C_DM x its own bound of
its threshold: the kernel may then decide either way."""
import math

import numpy as np

from tests import relax_ref as rr

EPS32 = rr.EPS32
C_DM = 2.0
TINY32 = rr.TINY32
CHECK_ONLY = 1
INTS = ('status', 'phase', 'n_steps', 'n_evals', 'n_rot', 'n_rot_total', 'n_pairs', 'head', 'pending')        # the rows of istate, in order
FLOATS = ('curvature', 'slope', 'c2', 's2', 'd_norm')                                               # of fstate
VECS = ('center', 'mode', 'F0', 'F1', 'theta', 'theta_rot', 'g_old', 'x_prev', 'f_prev')            # of vstate
FLT_MAX = float(np.finfo(np.float32).max)


def new_state(n, m, x, mode):
    """the state of a molecule of n atoms before its first launch"""
    st = {k: 0 for k in INTS}
    st.update({k: 0.0 for k in FLOATS})
    st.update({k: np.zeros((n, 3)) for k in VECS})
    st['center'], st['mode'] = np.array(x, dtype=np.float64), np.array(mode, dtype=np.float64)
    st.update(S=np.zeros((m, n, 3)), Y=np.zeros((m, n, 3)), rho=np.zeros(m))
    return st


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def params(fmax=0.001, dimer_length=0.01, rotation_tolerance=5.0, max_rotations=8, maxstep=0.2, alpha=70.0, fp32=True):
    """the numbers a launch gets (fp32=True: rounded as the driver rounds them)"""
    r = (lambda v: float(np.float32(v))) if fp32 else float
    return dict(tol2=r(fmax * fmax), delta=r(dimer_length), rot_tol=r(math.tan(2.0 * math.radians(rotation_tolerance))),
                max_rotations=int(max_rotations), maxstep=r(maxstep), alpha=r(alpha))


# ---- the two forms of the angles (fp64; the host tests check that they agree) -------------------------------------------------------

def trial_angle_roots(r):
    """(cos 2phi1, sin 2phi1, cos phi1, sin phi1) of tan 2phi1 = r >= 0 by roots and quotients, as the device forms them"""
    c2 = 1.0 / math.sqrt(1.0 + r * r)
    s2 = r * c2
    c1 = math.sqrt(0.5 * (1.0 + c2))
    return c2, s2, c1, s2 / (2.0 * c1)


def trial_angle_atan(r):
    phi = 0.5 * math.atan(r)
    return math.cos(2 * phi), math.sin(2 * phi), math.cos(phi), math.sin(phi)


def min_angle_roots(a1, b1):
    """(cos phi, sin phi) of the minimiser of a1 cos 2phi + b1 sin 2phi, cos phi >= 0; phi = 0 when a1 = b1 = 0"""
    root = math.sqrt(a1 * a1 + b1 * b1)
    if not (0.0 < root < math.inf):
        return 1.0, 0.0
    cm2, sm2 = -a1 / root, -b1 / root
    if cm2 >= 0.0:
        cp = math.sqrt(0.5 * (1.0 + cm2))
        return cp, sm2 / (2.0 * cp)
    sa = math.sqrt(0.5 * (1.0 - cm2))
    return abs(sm2) / (2.0 * sa), math.copysign(sa, sm2)


def min_angle_atan(a1, b1):
    """the same by phi = atan(b1 / a1) / 2, shifted by pi / 2 when that is the maximum, brought to cos phi >= 0"""
    with np.errstate(divide='ignore'):
        phi = 0.5 * math.atan(np.divide(b1, a1))
    if a1 * math.cos(2 * phi) + b1 * math.sin(2 * phi) > 0.0:
        phi += 0.5 * math.pi
    c, s = math.cos(phi), math.sin(phi)
    return (-c, -s) if c < 0 else (c, s)


# ---- the arithmetics ----------------------------------------------------------------------------------------------------------------

class _V:
    """a value (scalar or array, fp64) with its first-order bound"""
    __slots__ = ('v', 'b')

    def __init__(self, v, b=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.b = np.broadcast_to(np.asarray(b, dtype=np.float64), self.v.shape).astype(np.float64)


class Bound:
    def __init__(self, eps=EPS32):
        self.eps = eps

    def const(self, x):
        return _V(x)

    def _r(self, v, b):
        return _V(v, b + self.eps * np.abs(v))

    def neg(self, a):
        return _V(-a.v, a.b)

    def abs(self, a):
        return _V(np.abs(a.v), a.b)

    def copysign(self, a, s):
        return _V(np.copysign(a.v, s.v), a.b)

    def add(self, a, b):
        return self._r(a.v + b.v, a.b + b.b)

    def sub(self, a, b):
        return self._r(a.v - b.v, a.b + b.b)

    def mul(self, a, b):
        return self._r(a.v * b.v, np.abs(a.v) * b.b + np.abs(b.v) * a.b)

    def fma(self, a, b, c):
        return self._r(a.v * b.v + c.v, np.abs(a.v) * b.b + np.abs(b.v) * a.b + c.b)

    def div(self, a, b):
        with np.errstate(divide='ignore', invalid='ignore'):
            q = a.v / b.v
            return self._r(q, (a.b + np.abs(q) * b.b) / np.abs(b.v))

    def sqrt(self, a):
        r = np.sqrt(a.v)
        with np.errstate(divide='ignore', invalid='ignore'):
            return self._r(r, np.where(r > 0, a.b / (2.0 * np.where(r > 0, r, 1.0)), np.sqrt(a.b)))

    def dot(self, a, b):
        """sum over atoms of a_i . b_i"""
        t = a.v * b.v
        n = a.v.shape[0]
        return _V(t.sum(), (rr.dot_depth(n) + 1) * self.eps * np.abs(t).sum() + (np.abs(a.v) * b.b + np.abs(b.v) * a.b).sum())

    def max_norm2(self, a):
        n2 = (a.v * a.v).sum(1)
        return _V(n2.max() if n2.size else 0.0, 4.0 * self.eps * (n2.max() if n2.size else 0.0))

    def exact(self, a):
        return _V(a.v)

    def widen(self, a, extra):
        return _V(a.v, a.b + extra)

    def val(self, a):
        return float(a.v)

    def bnd(self, a):
        return float(a.b)

    def where_rows(self, mask, a, b):
        return _V(np.where(mask, a.v, b.v), np.where(mask, a.b, b.b))

    def stored(self, a):
        """(value, output bound) of a stored result"""
        return a.v.copy(), np.where(a.b > 0, C_DM * a.b + TINY32, 0.0)

    def translate(self, center, ft, free, lb, par):
        return rr.lbfgs_step(center, ft, free, lb, 0.0, par['alpha'], par['maxstep'], 0, eps=self.eps)


class Emu32:
    def const(self, x):
        return np.asarray(x, dtype=np.float32)

    def neg(self, a):
        return -a

    def abs(self, a):
        return np.abs(a)

    def copysign(self, a, s):
        return np.copysign(a, s)

    def add(self, a, b):
        return (a + b).astype(np.float32)

    def sub(self, a, b):
        return (a - b).astype(np.float32)

    def mul(self, a, b):
        return (a * b).astype(np.float32)

    def fma(self, a, b, c):
        return rr._fma32(a, b, c)

    def div(self, a, b):
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            return (a / b).astype(np.float32)

    def sqrt(self, a):
        with np.errstate(invalid='ignore'):
            return np.sqrt(a, dtype=np.float32)

    def dot(self, a, b):
        return rr._wave_sum32(rr._dot3_32(a, b)) if a.shape[0] else np.float32(0)

    def max_norm2(self, a):
        return rr._dot3_32(a, a).max() if a.shape[0] else np.float32(0)

    def exact(self, a):
        return a

    def widen(self, a, extra):
        return a

    def val(self, a):
        return float(a)

    def bnd(self, a):
        return 0.0

    def where_rows(self, mask, a, b):
        return np.where(mask, a, b)

    def stored(self, a):
        return np.asarray(a, dtype=np.float64).copy(), None

    def translate(self, center, ft, free, lb, par):
        x_out, _, new = rr.emulate_step(center, ft, free, lb, 0.0, par['alpha'], par['maxstep'], 0)
        return dict(x_out=x_out.astype(np.float64), bx=None, state=new, accepted=None, clamped=None,
                    ambiguous=dict(accept=False, clamp=False), b_rho_new=None)


# ---- one launch -----------------------------------------------------------------------------------------------------------------------

def impossible(st, m):
    c_known = st['n_steps'] >= 1 or st['phase'] == 2
    return (st['status'] not in (0, 1) or st['phase'] not in (0, 1, 2) or min(st[k] for k in INTS) < 0 or st['n_pairs'] > m
            or st['head'] >= m or st['pending'] > 1 or (st['n_evals'] == 0 and st['phase'] != 0) or (c_known and not math.isfinite(st['curvature'])))


def dimer_step(x, F, free, st, par, flags=0, eps=EPS32, emulate=False, ft_stored=None, energy=None):
    with np.errstate(all='ignore'):                          # (C == 0 divides by it on purpose, as the device does)
        return _dimer_step(x, F, free, st, par, flags, eps, emulate, ft_stored, energy)


def _dimer_step(x, F, free, st, par, flags, eps, emulate, ft_stored, energy):
    """One launch for one molecule.  x, F [n,3]: the fp32 probe and the force there; free: bool [n] or None; st: the state
    (new_state; not modified); par: params().  Returns a dict:
      x_out, bx [n,3]     the next probe and its bound (C_DM x first order + TINY32; 0 where the value is a copy)
      state, bounds       the state after the launch and, per FLOATS / VECS name written by arithmetic, its bound (emulate: None)
      fmax, b_fmax, energy   what fmax_out / energy_out get, None when the launch does not write them (the probe is no centre)
      frozen, path        path: the branches taken, e.g. 'p2>assess>cg>trial' or 'p1>assess>translate:tol:concave'
      translate           relax_ref.lbfgs_step's result for the translation (None without one);  ft, b_ft: F+ and its bound
      ambiguous           dict of bools per decision
    ft_stored: the F+ the kernel stored, to take the translation from (see the module's head)."""
    A = Emu32() if emulate else Bound(eps)
    n, m = np.shape(x)[0], st['S'].shape[0]
    fr = np.ones((n, 1), dtype=bool) if free is None else np.asarray(free, dtype=bool)[:, None]
    x64 = np.asarray(x, dtype=np.float64)
    new = copy_state(st)
    bounds, amb = {}, {}
    out = dict(x_out=x64.copy(), bx=np.zeros_like(x64), state=new, bounds=bounds, fmax=None, b_fmax=None, energy=None, frozen=True,
               path='frozen', translate=None, ft=None, b_ft=None, ambiguous=amb, bad=False)
    if impossible(st, m):
        out.update(bad=True, fmax=math.nan, path='bad')
        return out
    f = A.const(np.where(fr, np.asarray(F, dtype=np.float64), 0.0))           # (a fixed atom's force row may hold anything)
    fmax2 = A.max_norm2(f)
    if st['phase'] == 0:
        fm = A.sqrt(fmax2)
        out.update(fmax=A.val(fm), b_fmax=C_DM * A.bnd(fm) + TINY32, energy=energy)
    if st['status'] != 0 or n == 0 or (flags & CHECK_ONLY):
        return out
    out['frozen'] = False
    new['n_evals'] += 1
    delta = A.const(par['delta'])

    zero = A.const(np.zeros((n, 3)))
    live = {}                                                # vectors this launch has formed, with their bounds

    def ld(name):
        return live[name] if name in live else A.const(np.where(fr, new[name], 0.0))

    def put(name, val):
        v, b = A.stored(val)
        new[name] = np.where(fr, v, st[name])
        if b is not None:
            bounds[name] = np.where(fr, b, 0.0)
        live[name] = A.where_rows(fr, val, zero)

    def put_scalar(name, val):
        new[name] = A.val(val)
        bounds[name] = (C_DM * A.bnd(val) + TINY32 if A.bnd(val) > 0 else 0.0) if not emulate else None

    def decide(name, val, threshold, result):
        if not emulate:
            # (a value without a bound is exact: the device forms the same one and decides alike, also AT the threshold)
            amb[name] = amb.get(name, False) or (A.bnd(val) > 0 and abs(A.val(val) - threshold) <= C_DM * A.bnd(val))
        return result

    def half_angle(c2, s2):
        c1 = A.sqrt(A.mul(A.const(0.5), A.add(A.const(1.0), c2)))
        return c1, A.div(s2, A.mul(A.const(2.0), c1))

    def endpoint(direction):
        xo = A.fma(delta, direction, A.const(new['center']))
        v, b = A.stored(xo)
        out['x_out'] = np.where(fr, v, new['center'])
        out['bx'] = np.where(fr, b, 0.0) if b is not None else None

    C = A.const(st['curvature'])
    if st['phase'] == 0:
        new['F0'] = A.stored(f)[0]
        if st['n_evals'] == 0:
            new['center'] = x64.copy()
        small = decide('converge', fmax2, par['tol2'], A.val(fmax2) < par['tol2'])
        if st['n_steps'] >= 1 and small and st['curvature'] < 0:
            new['status'] = 1
            out['path'] = 'p0>converged'
            return out
        if not (st['n_steps'] >= 1 and st['curvature'] < 0):
            amb['converge'] = False                          # the force's size decides nothing then
        endpoint(ld('mode'))
        new['phase'], new['n_rot'] = 1, 0
        out['path'] = 'p0>first' if st['n_evals'] == 0 else ('p0>refused' if small and st['n_steps'] >= 1 else 'p0>endpoint')
        return out
    path = ['p%d' % st['phase']]
    after_trial = st['phase'] == 2
    if not after_trial:
        new['F1'] = A.stored(f)[0]
    else:
        b1, c2, s2 = A.const(st['slope']), A.const(st['c2']), A.const(st['s2'])
        c1, s1 = half_angle(c2, s2)
        N, Th, F0, F1 = ld('mode'), ld('theta'), ld('F0'), ld('F1')
        nstar = A.fma(s1, Th, A.mul(c1, N))
        Cs = A.div(A.dot(A.sub(F0, f), nstar), delta)
        a1 = A.div(A.fma(b1, s2, A.sub(C, Cs)), A.mul(A.const(2.0), A.mul(s1, s1)))
        root = A.sqrt(A.fma(a1, a1, A.mul(b1, b1)))
        rv = A.val(root)
        if decide('angle', root, 0.0, rv > 0.0 and rv <= FLT_MAX):
            cm2, sm2 = A.div(A.neg(a1), root), A.div(A.neg(b1), root)
        else:
            cm2, sm2 = A.const(1.0), A.const(0.0)
            path.append('phi0')
        if A.val(cm2) >= 0.0:
            cp = A.sqrt(A.mul(A.const(0.5), A.add(A.const(1.0), cm2)))
            sp = A.div(sm2, A.mul(A.const(2.0), cp))
        else:
            sa = A.sqrt(A.mul(A.const(0.5), A.sub(A.const(1.0), cm2)))
            sp = A.copysign(sa, sm2)
            cp = A.div(A.abs(sm2), A.mul(A.const(2.0), sa))
        # The three coefficients add up to 1 whatever cp and sp are, so an error of cp or sp reaches F1 through the DIFFERENCES
        # d F1 / d cp = F1 - F0 and d F1 / d sp = (f - F0 - c1 (F1 - F0)) / s1, not through the forces themselves: the operations
        # are followed with cp, sp taken as exact, and their bounds added through these two derivatives
        cpx, spx = A.exact(cp), A.exact(sp)
        k1 = A.div(A.sub(A.mul(s1, cpx), A.mul(c1, spx)), s1)
        k2 = A.div(spx, s1)
        k0 = A.sub(A.sub(A.const(1.0), cpx), A.mul(spx, A.div(s1, A.add(A.const(1.0), c1))))
        F1n = A.fma(k0, F0, A.fma(k2, f, A.mul(k1, F1)))
        if not emulate:
            dcp = np.abs(F1.v - F0.v)
            dsp = np.abs(f.v - F0.v - c1.v * (F1.v - F0.v)) / abs(s1.v)
            F1n = A.widen(F1n, cp.b * dcp + sp.b * dsp)
        trot = A.fma(cp, Th, A.mul(A.neg(sp), N))
        nw = A.fma(sp, Th, A.mul(cp, N))
        norm = A.sqrt(A.dot(nw, nw))
        Nn = A.div(nw, norm) if A.val(norm) > 0.0 else nw
        put('F1', F1n)
        put('theta_rot', trot)
        put('mode', Nn)
        new['n_rot'] += 1
        new['n_rot_total'] += 1
        out['phi'] = (A.val(cp), A.val(sp))
    # ---- assess
    N, F0, F1 = ld('mode'), ld('F0'), ld('F1')
    g = A.sub(F1, F0)
    gN = A.dot(g, N)
    C = A.div(A.neg(gN), delta)
    G = A.fma(A.neg(gN), N, g)
    out['G'] = np.where(fr, A.stored(G)[0], 0.0)
    D = G
    if after_trial:
        go = ld('g_old')
        num, den = A.dot(G, A.sub(G, go)), A.dot(go, go)
        beta = A.const(0.0)
        if A.val(den) > 0.0:
            q = A.div(num, den)
            pos = decide('beta', num, 0.0, A.val(q) > 0.0)
            beta = q if pos else A.const(0.0)
            path.append('cg' if pos else 'clipped')
        Dc = A.fma(A.mul(beta, A.const(st['d_norm'])), ld('theta_rot'), G)
        Dc = A.fma(A.neg(A.dot(Dc, N)), N, Dc)
        dg = A.dot(Dc, G)
        keep = decide('reset', dg, 0.0, A.val(dg) > 0.0)
        if keep:
            D = Dc
        else:
            path.append('reset')
    d_norm = A.sqrt(A.dot(D, D))
    b1 = r = None
    c2, s2 = A.const(1.0), A.const(0.0)
    zero_d = not (A.val(d_norm) > 0.0)
    r_inf = False
    if not zero_d:
        Th = A.div(D, d_norm)
        put('theta', Th)
        b1 = A.div(A.neg(A.dot(g, Th)), delta)
        r = A.div(A.neg(b1), A.abs(C))
        t = A.fma(r, r, A.const(1.0))
        if A.val(C) == 0.0 or not (A.val(t) <= FLT_MAX):
            c2, s2, r_inf = A.const(0.0), A.const(1.0), True
            path.append('c0')
        else:
            c2 = A.div(A.const(1.0), A.sqrt(t))
            s2 = A.mul(r, c2)
    else:
        b1 = A.const(0.0)
    put_scalar('curvature', C)
    put_scalar('slope', b1)
    put_scalar('c2', c2)
    put_scalar('s2', s2)
    put_scalar('d_norm', d_norm)
    by_tol = False
    if not zero_d and not r_inf:
        by_tol = decide('rotation', r, par['rot_tol'], A.val(r) < par['rot_tol'])
    done = zero_d or by_tol or new['n_rot'] >= par['max_rotations']
    if not done:
        put('g_old', G)
        c1, s1 = half_angle(c2, s2)
        endpoint(A.fma(s1, ld('theta'), A.mul(c1, N)))
        new['phase'] = 2
        out['path'] = '>'.join(path + ['trial'])
        return out
    # ---- translate
    concave = decide('sign', C, 0.0, A.val(C) < 0.0)
    p = A.dot(F0, N)
    Ft = A.fma(A.mul(A.const(-2.0), p), N, F0) if concave else A.mul(A.neg(p), N)
    ft, b_ft = A.stored(Ft)
    ft = np.where(fr, ft, 0.0)
    out['ft'], out['b_ft'] = ft, (np.where(fr, b_ft, 0.0) if b_ft is not None else None)
    given = ft if ft_stored is None else np.asarray(ft_stored, dtype=np.float64)
    if not emulate and ft_stored is None and eps > 0:
        given = ft.astype(np.float32).astype(np.float64)
    # the history holds pairs of concave translations alone: a convex one is the plain step, drops it and leaves none pending
    lb = dict(converged=False, n_steps=int(concave and st['pending'] == 1), n_pairs=st['n_pairs'] if concave else 0, head=st['head'], S=st['S'], Y=st['Y'], rho=st['rho'],
              b_rho=np.zeros(m), f_prev=st['f_prev'])
    tr = A.translate(new['center'], given, None if free is None else np.asarray(free, dtype=bool), lb, par)
    out['translate'] = tr
    new['x_prev'] = new['center'].copy()
    new['center'] = np.asarray(tr['x_out'], dtype=np.float64)
    out['x_out'], out['bx'] = new['center'].copy(), tr['bx']
    for k in ('S', 'Y', 'rho', 'f_prev', 'n_pairs', 'head'):
        new[k] = tr['state'][k]
    new['n_steps'] = st['n_steps'] + 1
    new['phase'], new['pending'] = 0, int(concave)
    amb['accept'], amb['clamp'] = tr['ambiguous']['accept'], tr['ambiguous']['clamp']
    if lb['n_steps'] >= 1 and not (rr.pair_y(st['f_prev'], given).any() and st['S'][st['head']].any()):
        amb['accept'] = False                                # y = 0 or s = 0: the three sums are exact zeros in any arithmetic
    why = 'zero' if zero_d else 'tol' if by_tol else 'cap'
    out['path'] = '>'.join(path + ['translate:%s:%s' % (why, 'concave' if concave else 'convex')])
    return out


# ---- the whole method as a host loop ---------------------------------------------------------------------------------------------------

def search(energy_forces, x0, direction, fmax=0.001, dimer_length=0.01, rotation_tolerance=5.0, max_rotations=8, memory=16,
           maxstep=0.2, alpha=70.0, max_evaluations=1000, free=None, record=False):
    """The contract as a plain fp64 loop for one molecule: energy_forces(x [n,3] fp64) -> (E, F [n,3]).  Returns dict(x, mode,
    energy, fmax, curvature, converged, n_steps, n_evaluations, n_rotations[, probes])."""
    x = np.asarray(x0, dtype=np.float64).copy()
    u = np.asarray(direction, dtype=np.float64).copy()
    if free is not None:
        u = u * np.asarray(free, dtype=bool)[:, None]
    st = new_state(x.shape[0], memory, x, u / math.sqrt((u * u).sum()))
    par = params(fmax, dimer_length, rotation_tolerance, max_rotations, maxstep, alpha, fp32=False)
    probe, e_center, f_center, probes = x, None, None, []
    for _ in range(max_evaluations):
        E, F = energy_forces(probe)
        if record:
            probes.append(probe.copy())
        r = dimer_step(probe, np.asarray(F, dtype=np.float64), free, st, par, 0, eps=0.0, energy=float(np.ravel(E)[0]))
        if r['fmax'] is not None:
            e_center, f_center = r['energy'], r['fmax']
        st, probe = r['state'], r['x_out']
        if st['status']:
            break
    out = dict(x=st['center'], mode=st['mode'], energy=e_center, fmax=f_center, curvature=st['curvature'],
               converged=bool(st['status']), n_steps=st['n_steps'], n_evaluations=st['n_evals'], n_rotations=st['n_rot_total'])
    if record:
        out['probes'] = probes
    return out


# ---- synthetic kernel inputs: every branch of a launch at every size class (shared by the host and the GPU tests) ------------------

SYN_SIZES = (1, 2, 21, 63, 64, 65, 200)
SYN_MEMORY = 4
SYN_PAR = params(fmax=0.01, dimer_length=0.01, rotation_tolerance=5.0, max_rotations=6, maxstep=0.2, alpha=70.0)
# the branches every size must reach (substrings of `path`, or predicates on the reference's result)
SYN_WANTED = ('p0>first', 'p0>endpoint', 'p0>converged', 'p0>refused', 'p1>trial', 'p1>translate:tol', 'p2>cg>trial', 'p2>clipped>trial',
              'p2>cg>reset>trial', 'p2>translate:tol', 'p2>translate:cap', 'p2>phi0', 'p1>c0>trial', ':concave', ':convex',
              'pairs0', 'pairs1', 'pairs3', 'pairs4', 'accepted', 'rejected', 'clamped', 'unclamped', 'status1', 'dropped')


def _labels(r, st):
    """the names of SYN_WANTED a launch with reference result r from state st earns"""
    tok = r['path'].split('>')
    tags = set()
    if tok[0] == 'p0':
        tags.add(r['path'])
    else:
        last, trial = tok[-1], tok[-1] == 'trial'
        if tok[0] == 'p1' and trial:
            tags.add('p1>c0>trial' if 'c0' in tok else 'p1>trial')
        if tok[0] == 'p2' and trial and 'c0' not in tok and 'phi0' not in tok:
            tags.add('p2>clipped>trial' if 'clipped' in tok else 'p2>cg>reset>trial' if 'reset' in tok else 'p2>cg>trial')
        if 'phi0' in tok:
            tags.add('p2>phi0')
        for why in ('tol', 'cap'):
            if last.startswith('translate:' + why):
                tags.add('%s>translate:%s' % (tok[0], why))
        for curv in (':concave', ':convex'):
            if last.endswith(curv):
                tags.add(curv)
    if st['status']:
        tags.add('status1')
    tr = r['translate']
    if tr is not None:
        if tok[-1].endswith(':concave'):
            tags.add('pairs%d' % st['n_pairs'])
        elif st['n_pairs'] > 0:
            tags.add('dropped')
        if tr['accepted'] is not None:
            tags.add('accepted' if tr['accepted'] else 'rejected')
        tags.add('clamped' if tr['clamped'] else 'unclamped')
    return tags & set(SYN_WANTED)


def _saddle_surface(rng, n, free):
    """a quadratic with one negative eigenvalue on the free coordinates of n atoms: (H [3n,3n], x_s [n,3])"""
    d = 3 * n
    mask = np.repeat(free, 3).astype(np.float64)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = np.exp(rng.uniform(np.log(2.0), np.log(60.0), d))
    lam[0] = -3.0
    H = (Q * lam) @ Q.T * np.outer(mask, mask) + np.diag(1.0 - mask)
    return H, rng.uniform(-4, 4, (n, 3))


def _to32(st):
    """a state with every float rounded to fp32 (what the device arrays hold)"""
    out = copy_state(st)
    for k, v in out.items():
        if isinstance(v, np.ndarray):
            out[k] = v.astype(np.float32).astype(np.float64)
        elif isinstance(v, float):
            out[k] = float(np.float32(v))
    return out


def _harvest(n, seed, masked):
    """launch inputs (x32, F32, free, state32) of a molecule of n atoms, harvested from float32 emulations of the method on random
    saddle surfaces started far from (clamped steps) and near the saddle, plus crafted variants of harvested states for the branches
    a healthy search seldom takes.  Returns a list of dicts(x, F, free, st)."""
    rng = np.random.default_rng(seed)
    par, m = SYN_PAR, SYN_MEMORY
    free = np.ones(n, dtype=bool)
    if masked and n >= 2:
        free = rng.random(n) >= 0.25
        free[rng.integers(n)] = True
    frm = free[:, None]
    cases = []

    def force_of(H, xs):
        def fn(x):
            F = -(H @ (np.asarray(x, dtype=np.float64) - xs).reshape(-1)).reshape(n, 3)
            F = F + 2e-3 * np.sin(37.0 * np.asarray(x, dtype=np.float64))          # not exactly quadratic: rotations do not end at once
            F32 = F.astype(np.float32)
            return np.where(frm, F32, np.float32(np.nan)) if masked else F32
        return fn
    for far in (True, False):
        H, xs = _saddle_surface(rng, n, free)
        fn = force_of(H, xs)
        amp = (2.0 if far else 0.02) / math.sqrt(n)
        x = (xs + rng.normal(0, amp, (n, 3)) * frm).astype(np.float32)
        u = rng.standard_normal((n, 3)) * frm
        w, V = np.linalg.eigh(H)
        u = u / np.linalg.norm(u) + 1.5 * V[:, 0].reshape(n, 3) * frm
        st = _to32(new_state(n, m, x, (u / np.linalg.norm(u)).astype(np.float32)))
        probe = x
        for _ in range(60 if far else 40):
            F = fn(probe)
            cases.append(dict(x=probe.copy(), F=F, free=free, st=st))
            r = dimer_step(probe, F, free if masked else None, st, par, emulate=True)
            st, probe = _to32(r['state']), r['x_out'].astype(np.float32)
            if st['status']:
                cases.append(dict(x=probe.copy(), F=fn(probe), free=free, st=st))
                break
    fm = free if masked else None
    crafted = []
    for c in cases:
        st, ph = c['st'], c['st']['phase']
        ref = dimer_step(c['x'], c['F'], fm, st, par, emulate=True)       # (what the launch does, at the emulation's price)
        f = np.where(frm, np.nan_to_num(c['F'].astype(np.float64)), 0.0)
        big = math.sqrt((f * f).sum(1).max())
        if ph == 0 and st['n_steps'] >= 1 and big > 0:
            for curv in (-1.0, 1.0):                                       # converging / refused: a small force, C < 0 / C > 0
                s2 = copy_state(st)
                s2['curvature'] = curv
                F2 = (c['F'].astype(np.float64) * (0.005 / big)).astype(np.float32)
                crafted.append(dict(x=c['x'], F=F2, free=free, st=s2))
            s2 = copy_state(st)
            s2['status'] = 1
            crafted.append(dict(x=c['x'], F=c['F'], free=free, st=s2))
        if ph == 2:
            s2 = copy_state(st)                                            # a1 = b1 = 0: the trial force is F0 itself, C = b1 = 0
            s2.update(curvature=0.0, slope=0.0, c2=0.0, s2=1.0, g_old=np.zeros((n, 3)))     # (G = g_old otherwise: beta on the edge)
            F2 = np.where(frm, s2['F0'], c['F'].astype(np.float64)).astype(np.float32)
            crafted.append(dict(x=c['x'], F=F2, free=free, st=s2))
            if ref['path'].endswith('trial'):
                s2 = copy_state(st)                                        # the rotation cap
                s2['n_rot'] = par['max_rotations'] - 1
                crafted.append(dict(x=c['x'], F=c['F'], free=free, st=s2))
            G = ref['G']
            if (G * G).sum() > 0:
                gn = math.sqrt((G * G).sum())
                s2 = copy_state(st)                                        # beta clipped: G.(G - g_old) = -|G|^2
                s2['g_old'] = (2.0 * G).astype(np.float32).astype(np.float64)
                crafted.append(dict(x=c['x'], F=c['F'], free=free, st=s2))
                # a reset: the new G is all but orthogonal to the rotated old direction (the rotation minimised along it), so a
                # search meets D.G <= 0 by rounding alone.  Here the stored THETA points against G; the launch carries it into
                # theta_rot, and with beta = 2 and DNORM = 2 |G|:  D = G + 4 |G| theta_rot ~ -3 G
                s2 = copy_state(st)
                s2['theta'] = (-G / gn).astype(np.float32).astype(np.float64)
                G2 = dimer_step(c['x'], c['F'], fm, s2, par, eps=0.0)['G']
                s2['g_old'] = (0.5 * G2).astype(np.float32).astype(np.float64)
                s2['d_norm'] = float(np.float32(2.0 * math.sqrt((G2 * G2).sum())))
                crafted.append(dict(x=c['x'], F=c['F'], free=free, st=s2))
        if ph == 1:
            F2 = np.where(frm, 2.0 * st['F0'] - c['F'].astype(np.float64), c['F'].astype(np.float64)).astype(np.float32)
            crafted.append(dict(x=c['x'], F=F2, free=free, st=st))         # g mirrored: the curvature changes its sign
            s2 = copy_state(st)                                            # C == 0: N along one coordinate, g without that one
            i0 = int(np.argmax(free))
            mode = np.zeros((n, 3))
            mode[i0, 0] = 1.0
            s2['mode'] = mode
            F2 = c['F'].astype(np.float64).copy()
            F2[i0, 0] = s2['F0'][i0, 0]
            crafted.append(dict(x=c['x'], F=F2.astype(np.float32), free=free, st=s2))
        if ref['translate'] is not None and st['n_steps'] >= 1 and ref['state']['head'] != st['head']:
            s2 = copy_state(st)                                            # a rejected pair: y mirrored
            s2['f_prev'] = (2.0 * ref['ft'] - st['f_prev']).astype(np.float32).astype(np.float64)
            crafted.append(dict(x=c['x'], F=c['F'], free=free, st=s2))
    return cases + crafted


def _cheap_labels(c, masked):
    """_labels from the float32 emulation alone"""
    st = c['st']
    emu = dimer_step(c['x'], c['F'], c['free'] if masked else None, st, SYN_PAR, emulate=True)
    if emu['translate'] is not None:
        step = np.sqrt(((emu['state']['center'] - emu['state']['x_prev']) ** 2).sum(1)).max()
        emu = dict(emu, translate=dict(accepted=(emu['state']['head'] != st['head']) if st['pending'] and emu['state']['pending'] else None,
                                       clamped=step >= 0.999 * SYN_PAR['maxstep']))
    return _labels(emu, st)


_SYN_CACHE = {}


def synthetic_cases(masked):
    """For every size of SYN_SIZES a minimal list of launch inputs that together earn every label of SYN_WANTED with no ambiguous
    decision.  Returns a list of dicts(n, x, F, free, st, labels, path)."""
    if masked in _SYN_CACHE:
        return _SYN_CACHE[masked]
    chosen = []
    for n in SYN_SIZES:
        missing = set(SYN_WANTED)
        for seed in range(100 * n, 100 * n + 12):
            for c in _harvest(n, seed, masked):
                if not _cheap_labels(c, masked) & missing:           # (the emulation says what a launch does; the reference,
                    continue                                         # which costs a two-loop's matrices, is asked only then)
                ref = dimer_step(c['x'], c['F'], c['free'] if masked else None, c['st'], SYN_PAR)
                if ref['bad'] or any(ref['ambiguous'].values()):
                    continue
                tags = _labels(ref, c['st'])
                if tags & missing:
                    missing -= tags
                    chosen.append(dict(n=n, x=c['x'], F=c['F'], free=c['free'], st=c['st'], labels=tags, path=ref['path']))
            if not missing:
                break
        if missing:
            raise AssertionError(f'synthetic inputs: size {n} (masked={masked}) never reaches {sorted(missing)}')
    _SYN_CACHE[masked] = chosen
    return chosen


def synthetic_batch(masked):
    """The cases of synthetic_cases as ONE batch in the kernel's layout, an empty molecule at the start, in the middle and at the
    end, unused history slots as the emulation left them.  Returns a dict of numpy arrays (ptr, x, F, free, istate, fstate, vstate,
    S, Y, rho) plus `cases` (None for the empty molecules) and par, memory."""
    cases = synthetic_cases(masked)
    cases = [None] + cases[:len(cases) // 2] + [None] + cases[len(cases) // 2:] + [None]
    m, f32 = SYN_MEMORY, np.float32
    sizes = [0 if c is None else c['n'] for c in cases]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N, B = int(ptr[-1]), len(cases)
    d = dict(ptr=ptr, x=np.zeros((N, 3), f32), F=np.zeros((N, 3), f32), free=np.ones(N, dtype=bool),
             istate=np.zeros((len(INTS), B), np.int32), fstate=np.zeros((len(FLOATS), B), f32),
             vstate=np.zeros((len(VECS), N, 3), f32), S=np.zeros((m, N, 3), f32), Y=np.zeros((m, N, 3), f32),
             rho=np.zeros((B, m), f32), cases=cases, par=SYN_PAR, memory=m, masked=masked)
    for b, c in enumerate(cases):
        if c is None:
            continue
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        st = c['st']
        d['x'][a0:a1], d['F'][a0:a1], d['free'][a0:a1] = c['x'], c['F'], c['free']
        for k, name in enumerate(INTS):
            d['istate'][k, b] = st[name]
        for k, name in enumerate(FLOATS):
            d['fstate'][k, b] = st[name]
        for k, name in enumerate(VECS):
            d['vstate'][k, a0:a1] = st[name]
        d['S'][:, a0:a1], d['Y'][:, a0:a1], d['rho'][b] = st['S'], st['Y'], st['rho']
    return d


def batch_state(d, b):
    """the reference state of molecule b of a batch in the kernel's layout"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    st = {name: int(d['istate'][k, b]) for k, name in enumerate(INTS)}
    st.update({name: float(d['fstate'][k, b]) for k, name in enumerate(FLOATS)})
    st.update({name: d['vstate'][k, a0:a1].astype(np.float64) for k, name in enumerate(VECS)})
    st.update(S=d['S'][:, a0:a1].astype(np.float64), Y=d['Y'][:, a0:a1].astype(np.float64), rho=d['rho'][b].astype(np.float64))
    return st


def batch_step(d, b, flags=0, **kw):
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    return dimer_step(d['x'][a0:a1], d['F'][a0:a1], d['free'][a0:a1] if d['masked'] else None, batch_state(d, b), d['par'], flags, **kw)


GROUPS = ('probe', 'scalars', 'vectors', 'ft', 'center')


def compare(ref, got_x, got_state, worst):
    """err / (bound + half an fp32 ulp) of a launch's outputs against its reference, folded into `worst` per GROUPS; got_state: the
    state after the launch as the device (or the emulation) left it.  Returns the largest ratio of this launch."""
    top = 0.0

    def fold(group, err, bound, value):
        nonlocal top
        lim = np.asarray(bound, dtype=np.float64) + rr.half_ulp32(value)
        ratio = float(np.max(np.asarray(err) / lim)) if np.size(err) else 0.0
        worst[group] = max(worst.get(group, 0.0), ratio)
        top = max(top, ratio)
    tr = ref['translate']
    if tr is None:
        fold('probe', np.abs(got_x - ref['x_out']), ref['bx'], ref['x_out'])
    else:
        fold('ft', np.abs(got_state['f_prev'] - ref['ft']), ref['b_ft'], ref['ft'])
        fold('center', np.abs(got_state['center'] - tr['x_out']), tr['bx'], tr['x_out'])
    for name, b in ref['bounds'].items():
        if b is None:
            continue
        v = ref['state'][name]
        if not np.all(np.isfinite(np.asarray(v))):
            continue
        fold('scalars' if name in FLOATS else 'vectors', np.abs(np.asarray(got_state[name]) - v), b, v)
    return top


def main():
    """the float32 emulation against the fp64 reference on every synthetic case; prints and returns (worst, total, ambiguous)"""
    worst, total, ambiguous = {}, 0, 0
    for masked in (False, True):
        for c in synthetic_cases(masked):
            fm = c['free'] if masked else None
            ref = dimer_step(c['x'], c['F'], fm, c['st'], SYN_PAR)
            emu = dimer_step(c['x'], c['F'], fm, c['st'], SYN_PAR, emulate=True)
            total += 1
            ambiguous += any(ref['ambiguous'].values())
            assert emu['path'] == ref['path'], (emu['path'], ref['path'])
            if ref['translate'] is not None:                 # the step is taken from the F+ the emulation stored
                ref = dimer_step(c['x'], c['F'], fm, c['st'], SYN_PAR, ft_stored=emu['ft'])
            compare(ref, emu['x_out'], emu['state'], worst)
    print('float32 emulation against the fp64 reference, worst err / (bound + half an ulp) per output group over', total, 'launches:')
    for g in GROUPS:
        print(f'  {g:8s} {worst.get(g, 0.0):.3f}')
    print('ambiguous decisions:', ambiguous)
    return worst, total, ambiguous


if __name__ == '__main__':
    main()
