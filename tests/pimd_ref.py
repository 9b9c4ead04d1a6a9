"""fp64 statement of one nnhip_pimd_step launch (csrc/pimd.hip) for the tests (numpy), with a per-element rounding bound.

The kernel's chain for one system of P slots and n atoms, per row (mode k, atom i) and coordinate, every line ONE fp32 operation
(an fma rounds once):
    f_k = C[k][0] F_0;  f_k = fma(C[k][s], F_s, f_k)  s = 1 .. P-1                      the mode force
    finish:  w = fma(hk, f_k, w)
             kinetic = (0.5 m) fma(wz,wz,fma(wy,wy,wx wx))                              (0.5 m is exact)
             spring  = (m half_w2) fma(uz,uz,fma(uy,uy,ux ux))                          (m half_w2 is one rounded product)
             virial  = fma(uz,fz,fma(uy,fy,ux fx)) for k > 0, 0 for k = 0
    begin:   w = fma(hk, f_k, w)
             A:  t = a u;  u' = fma(b, w, t);  t = a w;  w' = fma(d, u, t)              both from the old u, w
             O:  t = c1 w;  w = fma(sigma, xi, t)                                       only with noise
             A again
             x_s = C[0][s] u_0;  x_s = fma(C[k][s], u_k, x_s)  k = 1 .. P-1             the bead positions
`pimd_step` evaluates the same chain in fp64 from the SAME fp32 inputs (C, the mode table, hk, sigma already rounded) and carries
a first-order bound next to every value, exactly as tests/md_ref.py does: an operation with exact result r adds EPS32 |r|, and the
bounds of its operands pass through it multiplied by the magnitudes of the actual other operands.  The transform sums carry
sum_s |C[k][s]| bound(F_s) plus one EPS32 |partial sum| per fma.  Input bounds (du_in, dw_in, dF_in) let a test chain launches.

C_PI = 2 multiplies the first-order sum, for the reasons md_ref.C_MD gives (products of two roundings, magnitudes taken from the
fp64 values: both below 1e-5 of the bound even for the 64-term sums); it is the one safety constant, and a correct kernel shows
err / bound <= 0.5.  Results below the normal range add TINY32."""
import numpy as np

EPS32 = 2.0 ** -24
C_PI = 2.0
TINY32 = float(np.finfo(np.float32).tiny)
FINISH, BEGIN = 1, 2


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def transform(C, X, bX, transpose=False):
    """Y[k] = sum_s C[k][s] X[s] (transpose: sum_s C[s][k] X[s]) in the kernel's order, X [P,n,3]; returns (Y, bound of Y)"""
    M = C.T if transpose else C
    P = M.shape[0]
    bX = np.zeros_like(X) + bX
    Y = M[:, 0, None, None] * X[0][None]
    bY = np.abs(M[:, 0, None, None]) * bX[0][None] + EPS32 * np.abs(Y)
    for s in range(1, P):
        Y = M[:, s, None, None] * X[s][None] + Y
        bY = bY + np.abs(M[:, s, None, None]) * bX[s][None] + EPS32 * np.abs(Y)
    return Y, bY


def free_half_step(u, w, bu, bw, a, b, d):
    """A: the exact half step of the free ring polymer, (u, w) -> (a u + b w, d u + a w); a, b, d broadcast against u"""
    t = a * u
    bt = np.abs(a) * bu + EPS32 * np.abs(t)
    un = b * w + t
    bun = np.abs(b) * bw + bt + EPS32 * np.abs(un)
    t = a * w
    bt = np.abs(a) * bw + EPS32 * np.abs(t)
    wn = d * u + t
    bwn = np.abs(d) * bu + bt + EPS32 * np.abs(wn)
    return un, wn, bun, bwn


def _dot3(p, q, bp, bq):
    """fma(pz, qz, fma(py, qy, px qx)) over the last axis with its bound"""
    s = p[..., 0] * q[..., 0]
    bs = np.abs(p[..., 0]) * bq[..., 0] + np.abs(q[..., 0]) * bp[..., 0] + EPS32 * np.abs(s)
    for c in (1, 2):
        s = p[..., c] * q[..., c] + s
        bs = bs + np.abs(p[..., c]) * bq[..., c] + np.abs(q[..., c]) * bp[..., c] + EPS32 * np.abs(s)
    return s, bs


def pimd_step(flags, u, w, F, C, tab, hk, mass=None, sigma=None, xi=None, du_in=0.0, dw_in=0.0, dF_in=0.0, estimators=True):
    """One launch for ONE system.  u, w, F, xi [P,n,3]; C [P,P]; tab [P,5] (a, b, d, c1, half_w2); hk, mass, sigma [P,n]: the values
    the kernel gets.  Returns dict(u, w: the state after the launch; x [P,n,3]: the bead positions, None without BEGIN; est
    [P,n,4], None without FINISH or mass; bu, bw, bx, best: their bounds, C_PI x first order)."""
    u, w, F, xi, C, tab = _f64(u), _f64(w), _f64(F), _f64(xi), _f64(C), _f64(tab)
    hk, mass, sigma = _f64(hk), _f64(mass), _f64(sigma)
    assert (sigma is None) == (xi is None)
    P = C.shape[0]
    a, b, d, c1, hw2 = (tab[:, j, None, None] for j in range(5))
    h = hk[:, :, None]
    bu, bw = np.zeros_like(u) + du_in, np.zeros_like(w) + dw_in
    f, bf = transform(C, F, dF_in)
    x = bx = est = best = None
    if flags & FINISH:
        w = h * f + w
        bw = bw + h * bf + EPS32 * np.abs(w)
        if mass is not None and estimators:
            s, bs = _dot3(w, w, bw, bw)
            kin = 0.5 * mass * s
            bkin = 0.5 * mass * bs + EPS32 * np.abs(kin)
            cm = mass * hw2[:, :, 0]
            bcm = EPS32 * np.abs(cm)
            s, bs = _dot3(u, u, bu, bu)
            spr = cm * s
            bspr = cm * bs + np.abs(s) * bcm + EPS32 * np.abs(spr)
            vir, bvir = _dot3(u, f, bu, bf)
            vir[0], bvir[0] = 0.0, 0.0
            est = np.stack([kin, spr, vir, np.zeros_like(kin)], axis=-1)
            best = np.stack([bkin, bspr, bvir, np.zeros_like(kin)], axis=-1)
    if flags & BEGIN:
        w = h * f + w
        bw = bw + h * bf + EPS32 * np.abs(w)
        u, w, bu, bw = free_half_step(u, w, bu, bw, a, b, d)
        if xi is not None:
            t = c1 * w
            bt = np.abs(c1) * bw + EPS32 * np.abs(t)
            w = sigma[:, :, None] * xi + t
            bw = bt + EPS32 * np.abs(w)
        u, w, bu, bw = free_half_step(u, w, bu, bw, a, b, d)
        x, bx = transform(C, u, bu, transpose=True)
    return dict(u=u, w=w, x=x, est=est, bu=C_PI * bu + TINY32, bw=C_PI * bw + TINY32, bx=None if bx is None else C_PI * bx + TINY32,
                best=None if best is None else C_PI * best + TINY32)


def full_step(u, w, F0, F1, C, tab, hk, mass=None, sigma=None, xi=None, dF1=0.0):
    """One whole step from a full-step state: BEGIN with the bead forces F0 at the current beads, FINISH with the forces F1 at the
    new ones (dF1: their bound).  Returns dict(u, w, x, est, bu, bw, bx, best) of the state after the step."""
    p = pimd_step(BEGIN, u, w, F0, C, tab, hk, None, sigma, xi)
    # (p['bw'] already carries C_PI: entering it as dw_in multiplies that part by C_PI once more, on the safe side)
    q = pimd_step(FINISH, p['u'], p['w'], F1, C, tab, hk, mass, du_in=p['bu'] / C_PI, dw_in=p['bw'] / C_PI, dF_in=dF1)
    return dict(u=p['u'], w=q['w'], x=p['x'], est=q['est'], bu=p['bu'], bw=q['bw'], bx=p['bx'], best=q['best'])


def systems(mol_ptr, P):
    """(first row, atoms per slot) of every system of a flat layout"""
    ptr = np.asarray(mol_ptr)
    return [(int(ptr[g]), int(ptr[g + 1] - ptr[g])) for g in range(0, len(ptr) - 1, P)]


def flat(fn, mol_ptr, P, per_row, per_mol, **kw):
    """Apply fn (pimd_step / full_step bound to its flags) system by system to flat arrays: per_row {name: [N, ...]} are cut into
    [P, n, ...] blocks, per_mol {name: [B, ...]} into [P, ...] blocks; the dict results are put back into flat arrays"""
    N = int(np.asarray(mol_ptr)[-1])
    out = {}
    for g, (base, n) in enumerate(systems(mol_ptr, P)):
        args = {k: None if v is None else np.asarray(v)[base:base + P * n].reshape((P, n) + np.asarray(v).shape[1:])
                for k, v in per_row.items()}
        args.update({k: np.asarray(v)[g * P:(g + 1) * P] for k, v in per_mol.items()})
        r = fn(**args, **kw)
        for k, v in r.items():
            if v is None:
                continue
            if k not in out:
                out[k] = np.zeros((N,) + v.shape[2:])
            out[k][base:base + P * n] = v.reshape((P * n,) + v.shape[2:])
    return out


def half_ulp32(a):
    """half an fp32 ulp of |a| (the stored value's own rounding), fp64"""
    return 0.5 * np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)
