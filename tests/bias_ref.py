"""fp64 statement of one nnhip_bias_step launch (csrc/bias.hip) for ONE group, for the tests (numpy), with a rounding bound next to
every output.

The kernel's chain is restated operation by operation on values that carry their bound (class `B`): an fp32 operation with exact
result r adds EPS32 |r| (its one rounding to nearest, EPS32 = 2^-24; an fma rounds once), and the bounds of its operands pass
through it to first order, multiplied by the magnitudes of the actual other operands -- d(ab) = |a| db + |b| da, d(a / b) = da / |b|
+ |a| db / b^2, d sqrt(a) = da / (2 sqrt(a)), d atan2(y, x) = (|x| dy + |y| dx) / (x^2 + y^2), d exp(a) = exp(a) da.  The inputs
are the SAME fp32 values the kernel gets (tables already rounded), so they enter with bound 0.  A library call adds its ulp count
times one ulp, 2 EPS32 |r|; the counts are the named constants below.  The sums over the hills are taken in fp64 and bounded for ANY
order of DEPTH roundings per term: sum of the terms' bounds + DEPTH EPS32 sum |term|, DEPTH = ceil(H / 256) + 8 (a thread's serial
chain, six butterfly levels, two levels over the waves).

C_BIAS = 2 multiplies the first-order sum and TINY32 is added, exactly as tests/md_ref.py does and for its reasons; a correct
kernel shows err / bound <= 0.5 (the tests print it).

Ulp counts of the library calls.  The HIP math documentation is not part of the ROCm tree the tests run against, so -- as the
change that added this file laid down -- each call's worst error against fp64 was measured on the device over the argument ranges
of the tests (tools/probes/math_ulp_probe.hip; the figures are in DESIGN.md section 16) and the constant is TWICE the measured
value.  The probe also shows the division correctly rounded (half an ulp: the plain EPS32 of an operation) and rintf exact, and
__fsqrt_rn NOT correctly rounded on this device (0.916 ulp), so the square root is counted as a library call too.  The constants
were fixed from the probe alone, never fitted to the kernel's output.

Decisions the kernel takes on rounded values are restated on the fp64 ones; where the two could differ (a wrapped difference
within its own bound of half a period) the reference counts an AMBIGUOUS decision, and the tests choose inputs without any."""
import numpy as np

EPS32 = 2.0 ** -24
C_BIAS = 2.0
TINY32 = float(np.finfo(np.float32).tiny)
THREADS = 256
MAX_CVS = 2
DISTANCE, ANGLE, TORSION = 1, 2, 3
DEPOSIT = 1
STATUS_INVALID = 4
K_BOLTZMANN = 8.617333262e-5
TWO_PI32 = float(np.float32(2.0 * np.pi))

# measured worst errors (ulp) on an MI355X over 2^22 arguments each: expf 0.8360 on [-60, 0], atan2f 2.4781 over the plane (3e-4 .. 55
# in either coordinate, every sign), __fsqrt_rn 0.9160, __fdiv_rn 0.5000, rintf 0; the counts are twice that
EXP_ULP = 2.0 * 0.8360
ATAN2_ULP = 2.0 * 2.4781
SQRT_ULP = 2.0 * 0.9160
ULP = 2.0 * EPS32            # one ulp of r is at most 2 EPS32 |r|


class B:
    """a value (fp64 array) and the bound of the fp32 chain's error on it"""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) + e

    @staticmethod
    def of(x):
        return x if isinstance(x, B) else B(x)

    def _round(self, v, e, k=1.0):
        return B(v, e + k * EPS32 * np.abs(v))

    def __neg__(self):
        return B(-self.v, self.e)

    def __add__(self, o):
        o = B.of(o)
        return self._round(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = B.of(o)
        return self._round(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = B.of(o)
        with np.errstate(invalid='ignore'):               # (0 x inf at a singular variable: found non-finite and dropped by the caller)
            return self._round(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def exact_times(self, c):
        """times a power of two: no rounding"""
        return B(self.v * c, self.e * abs(c))

    def __truediv__(self, o):
        o = B.of(o)
        with np.errstate(divide='ignore', invalid='ignore'):
            return self._round(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))

    def sqrt(self):
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.sqrt(self.v)
            return B(r, np.where(self.e > 0, self.e / (2.0 * r), 0.0) + SQRT_ULP * ULP * np.abs(r))

    def exp(self):
        r = np.exp(self.v)
        return B(r, r * self.e + EXP_ULP * ULP * r)


def fma(a, b, c):
    a, b, c = B.of(a), B.of(b), B.of(c)
    v = a.v * b.v + c.v
    return B(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + c.e + EPS32 * np.abs(v))


def atan2(y, x):
    v = np.arctan2(y.v, x.v)
    with np.errstate(divide='ignore', invalid='ignore'):
        r2 = x.v * x.v + y.v * y.v
        e = np.where(r2 > 0, (np.abs(x.v) * y.e + np.abs(y.v) * x.e) / r2, 0.0)
    return B(v, e + ATAN2_ULP * ULP * np.abs(v))


def _sub3(a, b):
    return [a[k] - b[k] for k in range(3)]


def _add3(a, b):
    return [a[k] + b[k] for k in range(3)]


def _neg3(a):
    return [-a[k] for k in range(3)]


def _scale3(c, a):
    return [c * a[k] for k in range(3)]


def _dot3(a, b):
    return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0]))


def _cross3(a, b):
    return [fma(a[1], b[2], -(a[2] * b[1])), fma(a[2], b[0], -(a[0] * b[2])), fma(a[0], b[1], -(a[1] * b[0]))]


def _load3(x, i):
    return [B(x[i, k]) for k in range(3)]


def _finite3(*rows):
    return all(np.isfinite(c.v) and np.isfinite(c.e) for r in rows for c in r)


def variable(kind, idx, x):
    """(s, period, atoms, gradient rows, degenerate) of one variable on the positions x [n, 3] (fp32 values); s and the rows' components
    are B's.  kind 0: s = 0, no atoms."""
    zero = B(0.0)
    if kind == 0:
        return zero, 0.0, [], [], False
    if kind == DISTANCE:
        i, j = idx[:2]
        r = _sub3(_load3(x, j), _load3(x, i))
        d2 = _dot3(r, r)
        s = d2.sqrt()
        gj = _scale3(B(1.0) / s, r)
        atoms, rows = [i, j], [_neg3(gj), gj]
        degenerate = not (d2.v > 0) or not _finite3(gj)
    elif kind == ANGLE:
        i, j, k = idx[:3]
        xj = _load3(x, j)
        a, b = _sub3(_load3(x, i), xj), _sub3(_load3(x, k), xj)
        c = _cross3(a, b)
        c2 = _dot3(c, c)
        cn = c2.sqrt()
        s = atan2(cn, _dot3(a, b))
        gi = _scale3(B(1.0) / (_dot3(a, a) * cn), _cross3(a, c))
        gk = _scale3(B(1.0) / (_dot3(b, b) * cn), _cross3(c, b))
        atoms, rows = [i, j, k], [gi, _neg3(_add3(gi, gk)), gk]
        degenerate = not (c2.v > 0) or not _finite3(gi, gk)
    elif kind == TORSION:
        i, j, k, l = idx[:4]
        xi, xj, xk, xl = (_load3(x, a) for a in (i, j, k, l))
        b1, b2, b3 = _sub3(xj, xi), _sub3(xk, xj), _sub3(xl, xk)
        n1, n2 = _cross3(b1, b2), _cross3(b2, b3)
        b22 = _dot3(b2, b2)
        b2n = b22.sqrt()
        s = atan2(b2n * _dot3(b1, n2), _dot3(n1, n2))
        n12, n22 = _dot3(n1, n1), _dot3(n2, n2)
        gi = _scale3(-(b2n / n12), n1)
        gl = _scale3(b2n / n22, n2)
        p, q = _dot3(b1, b2) / b22, _dot3(b3, b2) / b22
        t = _sub3(_scale3(q, gl), _scale3(p, gi))
        atoms, rows = [i, j, k, l], [gi, _sub3(t, gi), _neg3(_add3(t, gl)), gl]
        degenerate = not (n12.v > 0) or not (n22.v > 0) or not _finite3(*rows)
    else:
        raise ValueError(kind)
    if degenerate:
        atoms, rows = [], []
        if not np.isfinite(s.v):
            s = zero
    return s, (TWO_PI32 if kind == TORSION else 0.0), atoms, rows, degenerate


def wrap(delta, period):
    """(delta - P rint(delta / P), how many decisions were ambiguous): the kernel rounds fl32(delta fl32(1 / P)) to an integer"""
    if not period > 0:
        return delta, 0
    inv = float(np.float32(1.0) / np.float32(period))
    q = delta.v * inv
    k = np.rint(q)
    slack = delta.e * inv + 4.0 * EPS32 * np.abs(q)
    ambiguous = int(np.count_nonzero(np.abs(np.abs(q - np.floor(q)) - 0.5) <= slack))
    return fma(B(-period), B(k), delta), ambiguous


def hill_sum(rows, s0, s1, is0, is1, p0, p1):
    """(V, G0, G1, ambiguous) over the hill rows [H, 4] at the point (s0, s1) (B's): the kernel's block_hill_sum"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    H = rows.shape[0]
    if H == 0:
        return B(0.0), B(0.0), B(0.0), 0
    d0, amb0 = wrap(s0 - B(rows[:, 0]), p0)
    d1, amb1 = wrap(s1 - B(rows[:, 1]), p1)
    a0, a1 = d0 * B(is0), d1 * B(is1)
    e = fma(a1, d1, a0 * d0)
    term = B(rows[:, 2]) * e.exact_times(-0.5).exp()
    depth = -(-H // THREADS) + 8

    def total(v, e_terms):
        return B(v.sum(), e_terms.sum() + depth * EPS32 * np.abs(v).sum())
    V = total(term.v, term.e)
    G0 = total(term.v * a0.v, np.abs(term.v) * a0.e + np.abs(a0.v) * term.e)
    G1 = total(term.v * a1.v, np.abs(term.v) * a1.e + np.abs(a1.v) * term.e)
    return V, G0, G1, amb0 + amb1


def _bound(b):
    return C_BIAS * b.e + TINY32


def walker(x, f_in, cv_def, restraint, hill_par, rows):
    """one molecule: x, f_in fp32 [n, 3]; cv_def int [2, 5]; restraint fp32 [2, 2]; hill_par fp32 [4]; rows fp32 [H, 4], the hills that
    exist.  Returns dict(force, bforce [n, 3]; cv, bcv [2]; bias = (V, U), bbias [2]; height, bheight: the row a deposit would write;
    status; ambiguous; touched: bool [n, 3], components with a bias part)"""
    x, f_in = np.asarray(x, dtype=np.float64), np.asarray(f_in, dtype=np.float64)
    n = x.shape[0]
    cv_def, restraint, hill_par = np.asarray(cv_def), np.asarray(restraint, dtype=np.float64), np.asarray(hill_par, dtype=np.float64)
    out = dict(force=f_in.copy(), bforce=np.zeros_like(f_in), cv=np.zeros(2), bcv=np.zeros(2), bias=np.zeros(2), bbias=np.zeros(2),
               height=0.0, bheight=0.0, status=0, ambiguous=0, touched=np.zeros(f_in.shape, dtype=bool))
    arity = {0: 0, DISTANCE: 2, ANGLE: 3, TORSION: 4}
    for d in range(MAX_CVS):
        kind = int(cv_def[d, 0])
        if kind not in arity or any(not 0 <= int(i) < n for i in cv_def[d, 1:1 + arity.get(kind, 0)]):
            out['status'] = STATUS_INVALID
            return out
    cvs = [variable(int(cv_def[d, 0]), [int(i) for i in cv_def[d, 1:]], x) for d in range(MAX_CVS)]
    (s0, p0, _, _, deg0), (s1, p1, _, _, deg1) = cvs
    V, G0, G1, amb = hill_sum(rows, s0, s1, hill_par[0], hill_par[1], p0, p1)
    coef, U = [], B(0.0)
    us = []
    for d, (s, p, _, _, _) in enumerate(cvs):
        r, a = wrap(s - B(restraint[d, 1]), p)
        amb += a
        k = B(restraint[d, 0]) * r if cv_def[d, 0] else B(0.0)
        us.append(k.exact_times(0.5) * r)
        coef.append(k - (G0, G1)[d])
    U = us[0] + us[1]
    force, bforce = out['force'], out['bforce']
    for i in range(n):
        part = None
        for d, (_, _, atoms, rows_d, _) in enumerate(cvs):
            if i in atoms:
                g = rows_d[atoms.index(i)]
                part = [coef[d] * g[k] for k in range(3)] if part is None else [fma(coef[d], g[k], part[k]) for k in range(3)]
        if part is None:
            continue
        for k in range(3):
            if part[k].v == 0.0 and part[k].e == 0.0:
                continue
            res = B(f_in[i, k]) - part[k]
            force[i, k], bforce[i, k] = res.v, _bound(res)
            out['touched'][i, k] = True
    height = B(hill_par[2]) * (-(V * B(hill_par[3]))).exp()
    out.update(cv=np.array([s0.v, s1.v]), bcv=np.array([_bound(s0), _bound(s1)]), bias=np.array([V.v, U.v]),
               bbias=np.array([_bound(V), _bound(U)]), height=float(height.v), bheight=float(_bound(height)),
               status=(1 if deg0 else 0) | (2 if deg1 else 0), ambiguous=amb)
    return out


def group(x, f_in, cv_def, restraint, hill_par, hills, n_deposits, flags=0):
    """one launch for one group of W walkers: x, f_in [W, n, 3]; cv_def [W, 2, 5]; restraint [W, 2, 2]; hill_par [4]; hills [capacity,
    4].  Returns the walkers' dicts and, with DEPOSIT, `rows` fp64 [W, 4] = what lands in the rows n_deposits W .. + W - 1 (the
    centres are each walker's cv; compare them with the kernel's cv_out bitwise and the heights within bheight)"""
    W = x.shape[0]
    H = n_deposits * W
    assert H + (W if flags & DEPOSIT else 0) <= hills.shape[0]
    walkers = [walker(x[j], f_in[j], cv_def[j], restraint[j], hill_par, hills[:H]) for j in range(W)]
    rows = None
    if flags & DEPOSIT:
        rows = np.array([[w['cv'][0], w['cv'][1], w['height'], 0.0] for w in walkers])
    return walkers, rows


def potential(x, cv_def, restraint, hill_par, rows):
    """V + U of one molecule at positions x (fp64, any precision): for finite differences"""
    w = walker(x, np.zeros_like(x), cv_def, restraint, hill_par, rows)
    return float(w['bias'].sum())


def half_ulp32(a):
    """half an fp32 ulp of |a| (the stored value's own rounding), fp64"""
    return 0.5 * np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def free_energy(V, bias_factor):
    """the estimate from the bias: -gamma / (gamma - 1) V (well-tempered) or -V (plain), shifted to minimum 0"""
    F = (-1.0 if bias_factor is None else -bias_factor / (bias_factor - 1.0)) * np.asarray(V, dtype=np.float64)
    return F - F.min()
