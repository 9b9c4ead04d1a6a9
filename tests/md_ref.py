"""fp64 statement of one nnhip_md_step launch (csrc/md.hip) for the tests (numpy), with a per-element rounding bound.

The kernel's chain, per atom i and coordinate k, every line ONE fp32 operation (an fma rounds once):
    finish:  v  = fma(hk_i, F_ik, v)
             s  = vx vx;  s = fma(vy, vy, s);  s = fma(vz, vz, s);  ke_i = (0.5 m_i) s         (0.5 m_i is exact)
    begin:   v  = fma(hk_i, F_ik, v)
             x  = fma(dth, v, x_in)
             t  = c1 v;  v = fma(sigma_i, xi_ik, t)                                            (only with noise)
             x_out = fma(dth, v, x)
`md_step` evaluates the same chain in fp64 from the SAME fp32 inputs (hk, sigma, c1, dth already rounded) and carries a first-order
bound next to every value: an operation with exact result r adds EPS32 |r| (its one rounding to nearest, EPS32 = 2^-24), and the
bounds of its operands pass through it multiplied by the magnitudes of the actual other operands -- for r = fma(a, b, c) with a
exact, bound(r) = |a| bound(b) + bound(c) + EPS32 |r|.  Input bounds (dv_in, dx_in) let a test chain two launches (begin with the
forces of step n, finish with those of step n + 1) without ever comparing across more than one step.

C_MD = 2 multiplies the first-order sum.  It stands for what first order leaves out: products of two roundings (relative 7 EPS32 at
the most over the chain of seven operations) and the magnitudes being taken from the fp64 values and not from the computed ones
(same order).  Both are below 1e-6 of the bound, so any constant above 1 + 1e-6 would do; 2 is the one safety constant, chosen
before any run, and a correct kernel shows err / bound <= 0.5 (the tests print it).  Results below the normal range add TINY32 (an
fp32 operation is exact to half a subnormal spacing there)."""
import numpy as np

EPS32 = 2.0 ** -24
C_MD = 2.0
TINY32 = float(np.finfo(np.float32).tiny)
FINISH, BEGIN = 1, 2


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def md_step(flags, x, v, F, hk, mass=None, sigma=None, xi=None, c1=1.0, dth=0.0, dv_in=0.0, dx_in=0.0):
    """One launch.  x, v, F, xi [N,3]; hk, mass, sigma [N]; c1, dth numbers: the fp32 values the kernel gets.  dv_in, dx_in: bounds of
    the inputs v and x (number or array).  Returns dict(x, v, ke: fp64 values -- x None without BEGIN, ke None without FINISH or
    mass; bx, bv, bke: their bounds, C_MD x first order)."""
    x, v, F, xi = _f64(x), _f64(v), _f64(F), _f64(xi)
    hk, sigma, mass = _f64(hk), _f64(sigma), _f64(mass)
    c1, dth = float(c1), float(dth)
    assert (sigma is None) == (xi is None)
    h = hk[:, None]
    bv = np.zeros_like(v) + dv_in
    bx = None
    ke = bke = None
    if flags & FINISH:
        v = h * F + v
        bv = bv + EPS32 * np.abs(v)
        if mass is not None:
            s = v[:, 0] * v[:, 0]
            bs = 2.0 * np.abs(v[:, 0]) * bv[:, 0] + EPS32 * np.abs(s)
            for k in (1, 2):
                s = v[:, k] * v[:, k] + s
                bs = bs + 2.0 * np.abs(v[:, k]) * bv[:, k] + EPS32 * np.abs(s)
            ke = 0.5 * mass * s
            bke = 0.5 * mass * bs + EPS32 * np.abs(ke)
    if flags & BEGIN:
        bx = np.zeros_like(x) + dx_in
        v = h * F + v
        bv = bv + EPS32 * np.abs(v)
        x = dth * v + x
        bx = bx + dth * bv + EPS32 * np.abs(x)
        if xi is not None:
            t = c1 * v
            bt = abs(c1) * bv + EPS32 * np.abs(t)
            v = sigma[:, None] * xi + t
            bv = bt + EPS32 * np.abs(v)
        x = dth * v + x
        bx = bx + dth * bv + EPS32 * np.abs(x)
    out = dict(x=x if flags & BEGIN else None, v=v, ke=ke, bx=None if bx is None else C_MD * bx + TINY32, bv=C_MD * bv + TINY32,
               bke=None if bke is None else C_MD * bke + TINY32)
    return out


def full_step(x, v, F0, F1, hk, mass=None, sigma=None, xi=None, c1=1.0, dth=0.0):
    """One whole MD step from a full-step state: BEGIN with the forces F0 at x, FINISH with the forces F1 at the new positions.
    Returns dict(x, v, ke, bx, bv, bke) of the state after the step; the bounds of the first launch enter the second."""
    a = md_step(BEGIN, x, v, F0, hk, None, sigma, xi, c1, dth)
    # (a['bv'] already carries C_MD: entering it as dv_in multiplies that part by C_MD once more, on the safe side by a factor <= 2)
    b = md_step(FINISH, a['x'], a['v'], F1, hk, mass, dv_in=a['bv'] / C_MD)
    return dict(x=a['x'], v=b['v'], ke=b['ke'], bx=a['bx'], bv=b['bv'], bke=b['bke'])


def half_ulp32(a):
    """half an fp32 ulp of |a| (the stored value's own rounding), fp64"""
    return 0.5 * np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def kinetic_sum_bound(ke):
    """bound of an fp32 sum of n terms in any order against the fp64 sum: n EPS32 sum |ke|"""
    ke = np.asarray(ke, dtype=np.float64)
    return ke.size * EPS32 * np.abs(ke).sum()


# ---- fp64 integrators for the host tests ------------------------------------------------------------------------------------

def harmonic_energy_error(dt, n_steps, k=1.0, m=1.0, x0=1.0):
    """max |E(n) - E(0)| of velocity Verlet (md_step with c1 = 1, no noise) on the 1-D oscillator m x'' = -k x over n_steps"""
    x, v = np.array([[x0, 0.0, 0.0]]), np.zeros((1, 3))
    hk = np.array([0.5 * dt / m])
    e0 = 0.5 * k * x0 * x0
    worst = 0.0
    F = -k * x
    for _ in range(n_steps):
        a = md_step(BEGIN, x, v, F, hk, dth=0.5 * dt)
        x = a['x']
        F = -k * x
        v = md_step(FINISH, None, a['v'], F, hk)['v']
        e = 0.5 * m * (v ** 2).sum() + 0.5 * k * (x ** 2).sum()
        worst = max(worst, abs(e - e0))
    return worst


def free_variance(c1, sigma, n):
    """Var v after n BAOAB steps with F = 0 from v = 0: every step maps v -> c1 v + sigma xi, so Var_n = c1^2 Var_{n-1} + sigma^2"""
    var = 0.0
    for _ in range(n):
        var = c1 * c1 * var + sigma * sigma
    return var
