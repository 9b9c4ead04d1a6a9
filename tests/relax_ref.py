"""fp64 statement of one nnhip_lbfgs_step launch (csrc/relax.hip) for ONE molecule, for the tests (numpy), with a per-element
rounding bound, in the manner of tests/md_ref.py.

The kernel's chain (every line ONE fp32 operation per element; dot3(a, b) = fma(az, bz, fma(ay, by, ax bx)); sum_l = lane-local sum
in atom order, lane l owning the atoms l, l + 64, ..., then the butterfly 32, 16, ..., 1):
    f = F (free) or 0 (fixed);  fmax2 = max_i dot3(f_i, f_i);  fmax = sqrt(fmax2)
    frozen (converged already | fmax2 < tol2 | no atoms | CHECK_ONLY):  x_out = x, nothing else
    y = f_prev - f;  ys, yy, ss = sum_l dot3 of (y, s), (y, y), (s, s) with s = S[head]
    accept iff ys > 0 and ys ys > (c c)(yy ss):  Y[head] = y, rho[head] = 1 / ys, n_pairs = min(n_pairs + 1, m), head = (head + 1) % m
    reject:  the slot is reused, and n_pairs = min(n_pairs, m - 1)  (in a full ring the pending s had replaced the oldest pair's)
    q = -f;  newest pair first:  a = rho (sum_l dot3(s, q));  q = fma(-a, y, q)
    z = q / alpha;  oldest pair first:  c = a - rho (sum_l dot3(y, z));  z = fma(c, s, z)
    longest = sqrt(max_i dot3(z_i, z_i));  if longest >= maxstep:  z = z (maxstep / longest)
    x_out = x + (-z) (fixed atoms: x);  S[head] = x_out - x;  f_prev = f;  n_steps += 1

`lbfgs_step` evaluates that in fp64 from the SAME fp32 inputs and state and carries a first-order bound next to every value: an
operation with exact result r adds eps |r| (eps = EPS32 = 2^-24, one rounding to nearest), and the bounds of its operands pass
through multiplied by the magnitudes of the other operands -- through the two-loop recursion by the recursion's own linear map
(`_two_loop` says why and how).  A reduction whose terms pass through at most `depth` roundings costs
(depth + 1) eps sum |term| plus the propagated operand bounds; for a dot product over n atoms depth = 3 (product, two fmas) +
ceil(n / 64) (lane-local adds) + 6 (butterfly).  Two values need NO bound because a single correctly rounded operation on exact
inputs is reproduced exactly in numpy's float32:  y = fl32(f_prev - f)  and  S[head] = fl32(x_out - x) from the kernel's own x_out
(`pair_y`, `stored_s`): the tests demand those bitwise.  rho carries a bound (`b_rho`, zero for a value handed in as exact).

C_RX = 2 multiplies the first-order sum at the outputs, for what first order leaves out (products of two roundings, magnitudes
taken from the fp64 values), as C_MD does in md_ref; it is chosen before any run, and a correct kernel shows err / bound <= 0.5.
Results below the normal range add TINY32.

The three decisions of a step -- convergence (fmax2 < tol2), pair acceptance, step clamp (longest >= maxstep) -- are reported as
AMBIGUOUS when the fp64 value lies within C_RX x its own bound of the threshold: the kernel may then decide either way, and a
test either constructs inputs without such a case (and says so) or skips and counts it."""
import math

import numpy as np

EPS32 = 2.0 ** -24
C_RX = 2.0
TINY32 = float(np.finfo(np.float32).tiny)
CHECK_ONLY = 1
MAX_MEMORY = 64
CURVATURE_MIN = 1e-4                                     # NNHIP_LBFGS_CURVATURE_MIN
_C32 = np.float32(CURVATURE_MIN)
CURVATURE_MIN2 = float(np.float32(_C32 * _C32))          # the fp32 product the kernel forms


def half_ulp32(a):
    """half an fp32 ulp of |a| (the stored value's own rounding), fp64"""
    return 0.5 * np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def new_state(n, m):
    """the state of a molecule of n atoms before its first step"""
    return dict(converged=False, n_steps=0, n_pairs=0, head=0, S=np.zeros((m, n, 3)), Y=np.zeros((m, n, 3)), rho=np.zeros(m),
                b_rho=np.zeros(m), f_prev=np.zeros((n, 3)))


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def masked(F, free):
    F = np.asarray(F, dtype=np.float64)
    return F if free is None else np.where(np.asarray(free, dtype=bool)[:, None], F, 0.0)


def pair_y(f_prev, f):
    """y = fl32(f_prev - f), exactly the kernel's: one correctly rounded fp32 subtraction of fp32 values"""
    return (np.asarray(f_prev, dtype=np.float32) - np.asarray(f, dtype=np.float32)).astype(np.float64)


def stored_s(x_out32, x32):
    """S[head] = fl32(x_out - x) on the STORED fp32 positions"""
    return (np.asarray(x_out32, dtype=np.float32) - np.asarray(x32, dtype=np.float32)).astype(np.float64)


def dot_depth(n):
    return 3 + (n + 63) // 64 + 6


def _dot(a, ba, b, bb, eps):
    t = a * b
    val = float(t.sum())
    bound = (dot_depth(a.shape[0]) + 1) * eps * float(np.abs(t).sum()) + float((np.abs(a) * bb + np.abs(b) * ba).sum())
    return val, bound


def pair_slots(head, n_pairs, m):
    """slots of the stored pairs, newest first"""
    return [(head - 1 - j + 2 * m) % m for j in range(n_pairs)]


def _two_loop(f, pairs, alpha, eps):
    """z = H f by the two-loop recursion (pairs: (s, y, rho, b_rho) flat, newest first) and the first-order bound of the fp32 z.

    The recursion is LINEAR in its work vector, so a rounding error made at one stage reaches z through the composition of the
    remaining stages, a fixed matrix.  The bound of z is the sum, over every rounding of the chain, of |that matrix| x the
    rounding's own bound -- NOT bounds pushed through the updates one at a time with absolute values: that grows by a factor
    1 + sum|s y| / |s.y| >= 2 per update whatever the data, 2^32 over the 32 updates of memory 16, and says nothing.  With
    T_j = W_0 ... W_{j-1} (W_k = I - rho_k s_k y_k^T; T_j carries z after loop-2 pass j to the end), t_j = T_j s_j and G_i the map
    from q after loop-1 pass i to z (G_{np-1} = T_np / alpha, G_{i-1} = G_i - rho_i (G_i y_i) s_i^T + rho_i t_i s_i^T, because
    a_i = rho_i s_i.q both updates q and comes back in loop 2), the roundings are:
      loop 1, pass i   a_i: rho_i x (depth + 1) eps sum|s_i q| (its dot) + |s_i.q| b_rho_i + eps |a_i|, through -G_i y_i + t_i;
                       q = fma(-a_i, y_i, q): eps |q| per element, through G_i
      z = q / alpha    eps |z| per element, through T_np
      loop 2, pass j   c_j = a_j - rho_j (y_j.z): rho_j x (depth + 1) eps sum|y_j z| + |y_j.z| b_rho_j + eps |rho_j y_j.z| + eps |c_j|,
                       through t_j;  z = fma(c_j, s_j, z): eps |z| per element, through T_j
    Returns (z [n,3], bz [n,3]); bz is first order, without C_RX."""
    shape = f.shape
    d, npair = f.size, len(pairs)
    q = -f.reshape(-1)
    if npair == 0:
        z = q / alpha
        return z.reshape(shape), (eps * np.abs(z)).reshape(shape)
    depth1 = dot_depth(shape[0]) + 1
    T = [np.eye(d)]
    for s, y, rho, _ in pairs:
        T.append(T[-1] - rho * np.outer(T[-1] @ s, y))
    t = [T[j] @ pairs[j][0] for j in range(npair)]
    G = [None] * npair
    G[npair - 1] = T[npair] / alpha
    for i in range(npair - 1, 0, -1):
        s, y, rho, _ = pairs[i]
        G[i - 1] = G[i] - rho * np.outer(G[i] @ y, s) + rho * np.outer(t[i], s)
    bz = np.zeros(d)
    a = [0.0] * npair
    for i, (s, y, rho, b_rho) in enumerate(pairs):
        sq = float(s @ q)
        a[i] = rho * sq
        da = abs(rho) * depth1 * eps * float(np.abs(s * q).sum()) + abs(sq) * b_rho + eps * abs(a[i])
        q = q - a[i] * y
        bz += np.abs(t[i] - G[i] @ y) * da + np.abs(G[i]) @ (eps * np.abs(q))
    z = q / alpha
    bz += np.abs(T[npair]) @ (eps * np.abs(z))
    for j in range(npair - 1, -1, -1):
        s, y, rho, b_rho = pairs[j]
        yz = float(y @ z)
        beta = rho * yz
        c = a[j] - beta
        dc = abs(rho) * depth1 * eps * float(np.abs(y * z).sum()) + abs(yz) * b_rho + eps * abs(beta) + eps * abs(c)
        z = z + c * s
        bz += np.abs(t[j]) * dc + np.abs(T[j]) @ (eps * np.abs(z))
    return z.reshape(shape), bz.reshape(shape)


def lbfgs_step(x, F, free, st, tol2, alpha, maxstep, flags=0, eps=EPS32, converge=None, accept=None):
    """One launch for one molecule.  x, F [n,3]: the fp32 values the kernel gets; free: bool [n] or None; st: the state (new_state;
    not modified); tol2, alpha, maxstep: the fp32 values.  Returns a dict:
      x_out, bx [n,3]   fp64 positions and their bound (C_RX x first order + TINY32); frozen molecules and fixed atoms: x, 0
      fmax, b_fmax      sqrt(max |f_i|^2) and its bound
      state             the state after the step (S[head] holds the fp64 x_out - x: a caller that has the stored fp32 positions
                        puts stored_s(...) there); rho / b_rho of an accepted pair are the fp64 1 / ys and its FIRST-ORDER bound
      b_rho_new         C_RX x that bound + TINY32, None when no pair was accepted
      frozen, accepted (None when no pair was pending), clamped
      ambiguous         dict(converge, accept, clamp) of bools
    converge, accept: None, or the decision to follow instead of the fp64 one -- for a caller that knows what the kernel decided in
    an ambiguous case (the clamp needs none: it leaves no trace in the state)"""
    x, f = np.asarray(x, dtype=np.float64), masked(F, free)
    n, m = x.shape[0], st['S'].shape[0]
    tol2, alpha, maxstep = float(tol2), float(alpha), float(maxstep)
    amb = dict(converge=False, accept=False, clamp=False)
    n2 = (f * f).sum(1)
    fmax2 = float(n2.max()) if n else 0.0
    b_fmax2 = 4.0 * eps * fmax2
    fmax = math.sqrt(fmax2)
    b_fmax = (b_fmax2 / (2.0 * fmax) if fmax > 0 else 0.0) + eps * fmax
    now = n == 0 or (fmax2 < tol2 if converge is None else bool(converge))
    if n and not st['converged']:
        amb['converge'] = abs(fmax2 - tol2) <= C_RX * b_fmax2
    out = dict(fmax=fmax, b_fmax=C_RX * b_fmax + TINY32, accepted=None, clamped=False, ambiguous=amb, b_rho_new=None)
    new = copy_state(st)
    if st['converged'] or now or (flags & CHECK_ONLY):
        new['converged'] = bool(st['converged'] or now)
        out.update(x_out=x.copy(), bx=np.zeros_like(x), state=new, frozen=True)
        return out
    head, n_pairs = st['head'], st['n_pairs']
    if st['n_steps'] > 0:
        y, s = pair_y(st['f_prev'], f), st['S'][head]
        ys, b_ys = _dot(y, 0.0, s, 0.0, eps)
        yy, b_yy = _dot(y, 0.0, y, 0.0, eps)
        ss, b_ss = _dot(s, 0.0, s, 0.0, eps)
        lhs = ys * ys
        b_lhs = 2.0 * abs(ys) * b_ys + eps * lhs
        t = yy * ss
        b_t = yy * b_ss + ss * b_yy + eps * t
        rhs = CURVATURE_MIN2 * t
        b_rhs = CURVATURE_MIN2 * b_t + eps * rhs
        accepted = (ys > 0.0 and lhs > rhs) if accept is None else bool(accept)
        amb['accept'] = abs(ys) <= C_RX * b_ys or (ys > 0.0 and abs(lhs - rhs) <= C_RX * (b_lhs + b_rhs))
        out['accepted'] = accepted
        if accepted:
            rho = 1.0 / ys
            b_rho = b_ys / (ys * ys) + eps * abs(rho)
            new['Y'][head], new['rho'][head], new['b_rho'][head] = y, rho, b_rho
            out['b_rho_new'] = C_RX * b_rho + TINY32
            n_pairs, head = min(n_pairs + 1, m), (head + 1) % m
        elif n_pairs == m:
            n_pairs = m - 1              # the rejected s had overwritten the oldest pair's in the full ring: that pair is gone
    S, Y, rho, b_rho = new['S'], new['Y'], new['rho'], new['b_rho']
    z, bz = _two_loop(f, [(S[k].reshape(-1), Y[k].reshape(-1), rho[k], b_rho[k]) for k in pair_slots(head, n_pairs, m)], alpha, eps)
    l2 = (z * z).sum(1)
    b_l2 = 2.0 * (np.abs(z) * bz).sum(1) + 4.0 * eps * l2
    longest2, b_longest2 = float(l2.max()), float(b_l2.max())
    longest = math.sqrt(longest2)
    b_longest = (b_longest2 / (2.0 * longest) if longest > 0 else math.sqrt(b_longest2)) + eps * longest
    clamped = longest >= maxstep
    amb['clamp'] = abs(longest - maxstep) <= C_RX * b_longest
    if clamped:
        scale = maxstep / longest
        b_scale = scale * b_longest / longest + eps * scale
        z_new = z * scale
        bz = scale * bz + np.abs(z) * b_scale + eps * np.abs(z_new)
        z = z_new
    x_out = x - z
    bx = bz + eps * np.abs(x_out)
    if free is not None:
        fr = np.asarray(free, dtype=bool)[:, None]
        x_out, bx = np.where(fr, x_out, x), np.where(fr, bx, 0.0)
    new['S'][head] = x_out - x
    new['f_prev'] = f.copy()
    new['n_steps'], new['n_pairs'], new['head'] = st['n_steps'] + 1, n_pairs, head
    moved = bx > 0
    out.update(x_out=x_out, bx=np.where(moved, C_RX * bx + TINY32, 0.0), state=new, frozen=False, clamped=clamped)
    return out


# ---- the same chain in numpy float32, in the kernel's order of operations (for the host tests) ------------------------------------

def _fma32(a, b, c):
    # (a b is exact in fp64 for fp32 operands; the sum rounds to fp64 and then to fp32 -- a double rounding that differs from a
    # true fma in rare ties only, far inside every bound here)
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def _dot3_32(a, b):
    return _fma32(a[:, 2], b[:, 2], _fma32(a[:, 1], b[:, 1], (a[:, 0] * b[:, 0]).astype(np.float32)))


def _wave_sum32(t):
    acc = np.zeros(64, dtype=np.float32)
    for i0 in range(0, t.shape[0], 64):
        chunk = t[i0:i0 + 64]
        acc[:chunk.shape[0]] = acc[:chunk.shape[0]] + chunk
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[lanes ^ d]).astype(np.float32)
    return acc[0]


def emulate_step(x, F, free, st, tol2, alpha, maxstep, flags=0):
    """lbfgs_step in float32 arithmetic, operation for operation as the kernel orders them.  Same state dict (its arrays are read
    as float32); returns (x_out float32, fmax float32, new state with float32-valued arrays)."""
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    f = masked(F, free).astype(f32)
    n, m = x.shape[0], st['S'].shape[0]
    new = copy_state(st)
    fmax2 = _dot3_32(f, f).max() if n else f32(0)
    now = n == 0 or fmax2 < f32(tol2)
    if st['converged'] or now or (flags & CHECK_ONLY):
        new['converged'] = bool(st['converged'] or now)
        return x.copy(), np.sqrt(fmax2, dtype=f32), new
    S, Y, rho = new['S'].astype(f32), new['Y'].astype(f32), new['rho'].astype(f32)
    head, n_pairs = st['head'], st['n_pairs']
    if st['n_steps'] > 0:
        y, s = (st['f_prev'].astype(f32) - f).astype(f32), S[head]
        ys, yy, ss = _wave_sum32(_dot3_32(y, s)), _wave_sum32(_dot3_32(y, y)), _wave_sum32(_dot3_32(s, s))
        if ys > 0 and f32(ys * ys) > f32(f32(CURVATURE_MIN2) * f32(yy * ss)):
            Y[head], rho[head] = y, f32(1.0) / ys
            n_pairs, head = min(n_pairs + 1, m), (head + 1) % m
        elif n_pairs == m:
            n_pairs = m - 1
    slots = pair_slots(head, n_pairs, m)
    q = -f
    a = {}
    for k in slots:
        a[k] = f32(rho[k] * _wave_sum32(_dot3_32(S[k], q)))
        q = _fma32(-a[k], Y[k], q)
    z = (q / f32(alpha)).astype(f32)
    for k in reversed(slots):
        c = f32(a[k] - f32(rho[k] * _wave_sum32(_dot3_32(Y[k], z))))
        z = _fma32(c, S[k], z)
    longest = np.sqrt(_dot3_32(z, z).max(), dtype=f32)
    if longest >= f32(maxstep):
        z = (z * f32(f32(maxstep) / longest)).astype(f32)
    x_out = (x + (-z)).astype(f32)
    if free is not None:
        x_out = np.where(np.asarray(free, dtype=bool)[:, None], x_out, x)
    S[head] = (x_out - x).astype(f32)
    new.update(S=S.astype(np.float64), Y=Y.astype(np.float64), rho=rho.astype(np.float64), f_prev=f.astype(np.float64),
               n_steps=st['n_steps'] + 1, n_pairs=n_pairs, head=head)
    return x_out, np.sqrt(fmax2, dtype=f32), new


# ---- fp64 L-BFGS of a whole batch, driven by a force callback (the yardstick of the convergence test) -----------------------------

def minimise(energy_forces, x0, mol_ptr, fmax=0.01, memory=16, maxstep=0.2, alpha=70.0, max_steps=500, free=None):
    """The contract above as a plain fp64 loop: energy_forces(x [N,3] fp64) -> (E [B], F [N,3]); every molecule keeps its own
    state; positions stay fp64 (S[head] is the fp64 difference).  Returns dict(x, energy, energy0, fmax, converged, n_steps)."""
    x = np.asarray(x0, dtype=np.float64).copy()
    B = len(mol_ptr) - 1
    sl = [slice(int(mol_ptr[b]), int(mol_ptr[b + 1])) for b in range(B)]
    states = [new_state(s.stop - s.start, memory) for s in sl]
    fr = [None if free is None else np.asarray(free, dtype=bool)[s] for s in sl]
    e0 = None
    for _ in range(max_steps + 1):
        E, F = energy_forces(x)
        E, F = np.asarray(E, dtype=np.float64), np.asarray(F, dtype=np.float64)
        e0 = E.copy() if e0 is None else e0
        last = _ == max_steps
        fm = np.zeros(B)
        for b, s in enumerate(sl):
            r = lbfgs_step(x[s], F[s], fr[b], states[b], fmax * fmax, alpha, maxstep, CHECK_ONLY if last else 0, eps=0.0)
            x[s], states[b], fm[b] = r['x_out'], r['state'], r['fmax']
        if all(st['converged'] for st in states):
            break
    return dict(x=x, energy=E, energy0=e0, fmax=fm, converged=np.array([st['converged'] for st in states]),
                n_steps=np.array([st['n_steps'] for st in states]))


# ---- synthetic kernel inputs: every branch of a launch at every size class (shared by the host and the GPU tests) -----------------

SYN_SIZES = (1, 2, 21, 63, 64, 65, 200)
SYN_MEMORY = 4
SYN_TOL2 = float(np.float32(np.float32(0.01) * np.float32(0.01)))
SYN_ALPHA, SYN_MAXSTEP = 70.0, float(np.float32(0.2))
# (pairs stored, kind).  accept: the pending pair has y = A s;  reject_neg: y = -A s (y.s < 0);  reject_cos: cos(y, s) = 2e-5;
# first: n_steps = 0;  converged: flag set, large forces;  converging: largest force 0.005 < 0.01
SYN_VARIANTS = ((0, 'first'), (0, 'accept'), (1, 'accept'), (SYN_MEMORY - 1, 'accept'), (SYN_MEMORY, 'accept'),
                (SYN_MEMORY, 'reject_neg'), (SYN_MEMORY - 1, 'reject_cos'), (2, 'reject_neg'), (2, 'converged'), (1, 'converging'))


def _spd(rng, d, lo=20.0, hi=2000.0):
    """random symmetric positive definite [d,d], eigenvalues log-uniform in [lo, hi] (both ends present when d > 1): condition 100"""
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = np.exp(rng.uniform(np.log(lo), np.log(hi), d))
    lam[0], lam[-1] = lo, hi if d > 1 else lo
    return (Q * lam) @ Q.T


def synthetic_batch(seed=0):
    """The batch of the kernel test: for every size of SYN_SIZES every variant of SYN_VARIANTS, once with forces of ~0.5 eV/A (no
    clamp) and once with ~30 eV/A (clamp), molecules of >= 2 atoms alternately with a quarter of their atoms fixed; empty molecules
    at the start, in the middle and at the end.  Stored pairs are y = A s with a random SPD A of condition 100 (fixed atoms: zero
    rows), heads are placed so that rings wrap, unused slots hold 7.0 (S, Y) and 0.5 (rho).  Returns a dict of numpy arrays in the
    kernel's layout and types, plus kinds / big (per molecule)."""
    rng = np.random.default_rng(seed)
    f32, m = np.float32, SYN_MEMORY
    mols = []
    count = 0
    for n in SYN_SIZES:
        for pairs, kind in SYN_VARIANTS:
            for big in (False, True):
                count += 1
                free = np.ones(n, dtype=bool)
                if n >= 2 and count % 2:
                    free = rng.random(n) >= 0.25
                    free[rng.integers(n)] = True
                mask = np.repeat(free, 3)
                d = 3 * n
                A = _spd(rng, d) * np.outer(mask, mask)
                head = {0: 0, 1: 1, 2: m - 1, m - 1: m - 1, m: 2}[pairs] if kind != 'first' else 0
                S, Y, rho = np.full((m, n, 3), 7.0, dtype=f32), np.full((m, n, 3), 7.0, dtype=f32), np.full(m, 0.5, dtype=f32)
                for k in pair_slots(head, min(pairs, m - 1 if kind != 'first' else m), m):
                    s = (rng.normal(0, 0.05, d) * mask).astype(f32)
                    y = (A @ s.astype(np.float64)).astype(f32)
                    S[k], Y[k] = s.reshape(n, 3), y.reshape(n, 3)
                    rho[k] = f32(1.0 / float(y.astype(np.float64) @ s.astype(np.float64)))
                scale = 30.0 if big else 0.5
                F = rng.normal(0, scale, (n, 3)).astype(f32)
                if kind == 'converging':
                    F = (F.astype(np.float64) * (0.005 / np.sqrt((masked(F, free) ** 2).sum(1).max()))).astype(f32)
                f = masked(F, free).astype(f32)
                f_prev = np.full((n, 3), 7.0, dtype=f32)
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
                    S[head] = s.reshape(n, 3)
                    f_prev = (f.astype(np.float64) + y.reshape(n, 3)).astype(f32)       # y = fl32(f_prev - f) ~ this y
                mols.append(dict(n=n, kind=kind, big=big, free=free, x=rng.uniform(-8, 8, (n, 3)).astype(f32), F=F, S=S, Y=Y, rho=rho,
                                 f_prev=f_prev, converged=int(kind == 'converged'), n_steps=n_steps,
                                 n_pairs=pairs if kind != 'first' else 0, head=head))
    empty = dict(n=0, kind='empty', big=False, free=np.ones(0, dtype=bool), x=np.zeros((0, 3), f32), F=np.zeros((0, 3), f32),
                 S=np.zeros((m, 0, 3), f32), Y=np.zeros((m, 0, 3), f32), rho=np.full(m, 0.5, f32), f_prev=np.zeros((0, 3), f32),
                 converged=0, n_steps=0, n_pairs=0, head=0)
    mols = [empty] + mols[:len(mols) // 2] + [dict(empty)] + mols[len(mols) // 2:] + [dict(empty)]
    out = dict(ptr=np.concatenate([[0], np.cumsum([q['n'] for q in mols])]).astype(np.int32),
               kinds=[q['kind'] for q in mols], big=[q['big'] for q in mols], memory=m, tol2=SYN_TOL2, alpha=SYN_ALPHA,
               maxstep=SYN_MAXSTEP)
    for k in ('x', 'F', 'f_prev', 'free'):
        out[k] = np.concatenate([q[k] for q in mols])
    for k in ('S', 'Y'):
        out[k] = np.ascontiguousarray(np.concatenate([q[k] for q in mols], axis=1))
    out['rho'] = np.stack([q['rho'] for q in mols])
    for k in ('converged', 'n_steps', 'n_pairs', 'head'):
        out[k] = np.array([q[k] for q in mols], dtype=np.int32)
    return out


def batch_state(d, b):
    """the reference state of molecule b of a batch in the kernel's layout (dict of numpy arrays as synthetic_batch returns)"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    m = d['S'].shape[0]
    return dict(converged=bool(d['converged'][b]), n_steps=int(d['n_steps'][b]), n_pairs=int(d['n_pairs'][b]), head=int(d['head'][b]),
                S=d['S'][:, a0:a1].astype(np.float64), Y=d['Y'][:, a0:a1].astype(np.float64), rho=d['rho'][b].astype(np.float64),
                b_rho=np.zeros(m), f_prev=d['f_prev'][a0:a1].astype(np.float64))


def batch_step(d, b, flags=0, eps=EPS32):
    """lbfgs_step of molecule b of such a batch"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    return lbfgs_step(d['x'][a0:a1], d['F'][a0:a1], d['free'][a0:a1], batch_state(d, b), d['tol2'], d['alpha'], d['maxstep'], flags, eps)
