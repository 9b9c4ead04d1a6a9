"""Float64 statements of the last stage of "tangent over reverse" (csrc/hessian.hip and the head of csrc/elastic.hip), which the C
interface exports one by one: nnhip_hvp_dgu, nnhip_hvp_dgx, nnhip_hvp_out, nnhip_hess_dirs, nnhip_hess_scatter,
nnhip_strain_tan_geom, nnhip_strain_born.  The conventions are those of tests/edge_ref.py: every statement returns
{output: (reference, bound, defined)}, the graphs come from edge_ref.stage_graph, what a kernel reads of a graph is an
edge_ref.View, and tests/test_hip_hvp_stages.py asserts |got - ref| <= bound element by element.  Numpy only, no GPU.

Statements
  dg_u[e][k] = < dgf[i][k], phi1[p] > + < gf[i][k], dphi1[p] >, i the receiver row of e, p = pid[e]; exactly 0 for a masked
      candidate (xg passed) and in the fourth component.
  dg_x[e]    = sum_f dg_eps[p][f] eps'_f(x) + g_eps[p][f] eps''_f(x) dx_e   on the OWNER edge (edge_index[0][e] < edge_index[1][e])
      of an unmasked pair with x < 1, exactly 0 on every other edge.  THE PREDICATE: x is formed as the kernel forms it,
          x = double(r_fp32) * double(fl32(1 / cutoff)),            (x_of below)
      so that an edge one ulp below the cutoff has a defined side.  eps_f(x) = sum_n W[f][n] env(x) sin(w_n x) / x; the derivatives
      are written here independently of the kernel's factored formulas: the envelope 1 - c0 x^p + c1 x^(p+1) - c2 x^(p+2)
      (c0 = (p+1)(p+2)/2, c1 = p(p+2), c2 = p(p+1)/2) is differentiated term by term, the cosine envelope directly, the Bessel
      factor as  b' = w cos(wx)/x - sin(wx)/x^2,  b'' = -w^2 sin(wx)/x - 2 w cos(wx)/x^2 + 2 sin(wx)/x^3,  all in longdouble, and
      joined by Leibniz' rule.  tests/test_hvp_ref_host.py holds them to mpmath's numerical derivatives and to torch autograd.
  dg_d[e]    = the tangent of g_d = a u + g_u / r, a = g_x / rc - (g_u.u) / r (layer sums) along (du, dr = rc dx):
          da = dg_x / rc - (dg_u.u + g_u.du) / r + (g_u.u) dr / r^2,   dg_d = da u + a du + dg_u / r - g_u dr / r^2,  dg_d.w = 0.
  hv[i]      = sum over the edges e of row i of dg_d[e] - dg_d[rev e]  (a row of degree 0: 0).
  hess_dirs / hess_scatter: integers, compared exactly (hess_dirs, hess_scatter below).
  tgeo (strain seed): dd = eta (r u) with eta = the Voigt matrix of eta6[batch[receiver]] (xx, yy, zz, yz / 2, xz / 2, xy / 2, as
      elastic_ref.voigt_matrix); dr = u.dd; tgeo = ((dd - u dr) / r, dr / rc).
  d2[b][I]   = sum_ab (d eps_ab / d e_I) S_ab, S_ab = sum_e dg_d[e]_a (r u)_e,b over the edges of system b's rows: S_00, S_11, S_22,
      (S_12 + S_21) / 2, (S_02 + S_20) / 2, (S_01 + S_10) / 2.

Bounds, u = 2^-24, by the rule of edge_ref: a sum of n fp32 terms of c roundings each, in ANY order, is within (n + c + 2) u sum|term|
of the exact sum.  A product that the compiler may or may not fuse into the following addition counts as one rounding of its
own (c += 1), so the bounds hold with and without contraction.
  dg_u: n = 2 F = 256 products, c = 1:  (2 F + 3) u sum|term|.
  dg_x: rbf'_n and rbf''_n dx are evaluated in fp64 and ROUNDED TO fp32 ONCE each (relative to their own values); eps' and eps'' dx
      are n_basis fused multiply-adds on them; then 2 F products and the wave sum: n = 2 F, c = n_basis + 1 (the rbf rounding) + 1
      (the product):  (2 F + n_basis + 4) u sum_f (|dg_eps| sum_n |W| |rbf'_n| + |g_eps| sum_n |W| |rbf''_n dx|).  The fp64 evaluation
      itself (sincos, pow, and the cancellation of w cos(wx) - sin(wx)/x at small w x) gets 2^-44 of the same sum taken over the
      magnitudes of the CANCELLING parts (|w cos/x| + |sin/x^2|, ...): 512 fp64 ulps of them.  The envelope VALUE is one of them:
      the kernel evaluates env' and env'' in factored form (-K x^(p-1) (1-x)^2, ...) but env itself as the expanded polynomial
      1 - c0 x^p + c1 x^(p+1) - c2 x^(p+2) (0.5 (1 + cos pi x) for the cosine), whose terms cancel to (1 - x)^3 at the cutoff, so
      the fp64 error of env b', env b'' is relative to 1 + c0 x^p + c1 x^(p+1) + c2 x^(p+2), not to env.  (Found by the fp32
      restatement on the edge one ulp inside the cutoff, before any kernel ran: with |env| in its place the restatement left the
      bound by 2 to 31 x there.  In absolute terms the allowance is 1e-9 of an ordinary dg_x.)
  dg_d: every output is a sum of products of leaves; along the longest path a leaf meets: the layer sum (L), a dot product of up to
      six products (6 + 1 + 2), two factors 1/r (3 each, as edge_ref.INV_C: the division and its use), dr = dx rc (1), the products
      g.u dr, ... (3), the three-term sum of da (2), the four products and three additions of the output (5), 2 spare for second
      order: GEOM_C + L = 28 + L roundings, relative to the MAGNITUDES of the cancelling terms
          Mda = Mdx / rc + (Mdu.|u| + Mu.|du|) / r + (Mu.|u|) |dr| / r^2,   Ma = Mx / rc + (Mu.|u|) / r,
          M_k = Mda |u_k| + Ma |du_k| + Mdu_k / r + Mu_k |dr| / r^2          (M*: layer sums of magnitudes)
      so that a small r shows as 1/r and 1/r^2 in the bound.
  hv:   n = deg differences of two fp32 dg_d, each rounded (c = 1): (deg + 3) u sum (|dg_d[e]| + |dg_d[rev e]|), and the bounds of the
      kernel's own dg_d ride along (times 1 + (deg + 3) u).
  tgeo: d_k = r (eta u)_k: three products (3 + 1 + 2) and the factor r: 7 u Md_k, Md_k = r sum_l |eta_kl| |u_l|;  dr = u.d: n = 3,
      c = 1 + 7: 13 u Mr, Mr = sum_k |u_k| Md_k;  du_k = (d_k - u_k dr) / r: 13 + the product + the difference + 1/r (3) + 2:
      20 u (Md_k + |u_k| Mr) / r;  dx = dr / rc: 13 + 3 + 2 = 18 u Mr / rc.
  d2:   the kernel forms d = r u exactly in fp64 (24 x 24 bits), accumulates dg d in fp64 and rounds the Voigt combination to
      fp32 once: u |exact| + 2^-50 sum|term| (the fp64 roundings of the products and of the additions).
"""
import numpy as np

from tests import edge_ref as R

U = R.U
F = R.F
f32, f64, LD = np.float32, np.float64, np.longdouble
MAX_NB, MAX_LAYERS, ENV_COSINE = 32, 8, -1
GEOM_C = 28
FP64_ALLOWANCE = 2.0 ** -44
BORN_ALLOWANCE = 2.0 ** -50
PI_LD = LD('3.14159265358979323846264338327950288')
ENVELOPES = (1, 2, 3, 9, ENV_COSINE)
NAN_MARK = np.array([0x7FC5A5A5], np.uint32).view(np.float32)[0]      # a quiet NaN in the padding lanes: it must reach no output


def _all(n):
    return np.ones(n, bool)


def x_of(g):
    """x of every directed edge as hvp_dgx_kernel forms it: double(r) * double(1.0f / cutoff)  (x_exact: an fp64 graph's own x)"""
    if getattr(g, 'x_exact', None) is not None:
        return np.asarray(g.x_exact, f64)
    inv_rc = f32(1.0) / f32(g.cutoff)
    return np.asarray(g.geo[:, 3], f32).astype(f64) * f64(inv_rc)


# ---------------------------------------------------------------------------------------------------------------------------
# the analytic basis
# ---------------------------------------------------------------------------------------------------------------------------
def envelope_d012(x, env):
    """(env, env', env'') at x in longdouble; env: p > 0 PolynomialCutoff(p), 0 = 9, ENV_COSINE"""
    return envelope_terms(x, env)[:3]


def envelope_terms(x, env):
    """(env, env', env'', the sum of the magnitudes of env's own terms) in longdouble"""
    x = np.asarray(x, LD)
    if env == ENV_COSINE:
        c = np.cos(PI_LD * x)
        return LD(0.5) * (1 + c), -LD(0.5) * PI_LD * np.sin(PI_LD * x), -LD(0.5) * PI_LD * PI_LD * c, LD(0.5) * (1 + np.abs(c))
    p = int(env) if env > 0 else 9
    terms = ((-LD((p + 1) * (p + 2)) / 2, p), (LD(p * (p + 2)), p + 1), (-LD(p * (p + 1)) / 2, p + 2))
    e, e1, e2, m = np.ones_like(x), np.zeros_like(x), np.zeros_like(x), np.ones_like(x)
    for c, q in terms:
        e = e + c * x ** q
        m = m + np.abs(c) * x ** q
        e1 = e1 + c * q * x ** (q - 1)
        if q * (q - 1):
            e2 = e2 + c * (q * (q - 1)) * x ** (q - 2)
    return e, e1, e2, m


def bessel_d012(x, w):
    """b = sin(w x) / x and its first two derivatives [n][nb], and the magnitudes of the cancelling parts of b', b''"""
    x, w = np.asarray(x, LD)[:, None], np.asarray(w, LD)[None, :]
    s, c = np.sin(w * x), np.cos(w * x)
    b = s / x
    t1 = (w * c / x, -s / x ** 2)
    t2 = (-w * w * s / x, -2 * w * c / x ** 2, 2 * s / x ** 3)
    return b, t1[0] + t1[1], t2[0] + t2[1] + t2[2], np.abs(t1[0]) + np.abs(t1[1]), np.abs(t2[0]) + np.abs(t2[1]) + np.abs(t2[2])


def rbf_d12(x, freq, env, mut=()):
    """(rbf', rbf'', magnitude of rbf''s cancelling parts, of rbf'''s) [n][nb] float64 of rbf_n = env(x) sin(w_n x) / x"""
    e, e1, e2, me = (np.asarray(t)[:, None] for t in envelope_terms(x, env))
    if 'p1_as_p2' in mut and env == 1:                    # the general formula without its p = 1 branch, as for p = 2
        e2 = np.asarray(envelope_d012(x, 2)[2])[:, None]
    b, b1, b2, m1, m2 = bessel_d012(x, np.asarray(freq, f32).astype(f64))
    cross = 1 if 'env_b_factor1' in mut else 2
    r1 = e1 * b + e * b1
    r2 = e2 * b + cross * e1 * b1 + e * b2
    A1 = np.abs(e1 * b) + me * m1
    A2 = np.abs(e2 * b) + 2 * np.abs(e1) * m1 + me * m2
    return tuple(np.asarray(t, f64) for t in (r1, r2, A1, A2))


# ---------------------------------------------------------------------------------------------------------------------------
# statements
# ---------------------------------------------------------------------------------------------------------------------------
def hvp_dgu(g, gf, dgf, phi1, dphi1, use_mask=True, view=None):
    v = view or R.View(g, use_mask)
    gf, dgf, phi1, dphi1 = (np.asarray(a, f64) for a in (gf, dgf, phi1, dphi1))
    val, B = np.zeros((g.E, 4)), np.zeros((g.E, 4))
    if g.E:
        p1, d1 = phi1[g.pid][:, None, :], dphi1[g.pid][:, None, :]
        t1, t2 = dgf[v.i] * p1, gf[v.i] * d1
        live = v.live[:, None]
        val[:, :3] = np.where(live, (t1 + t2).sum(axis=2), 0.0)
        B[:, :3] = np.where(live, (2 * F + 3) * U * (np.abs(t1) + np.abs(t2)).sum(axis=2), 0.0)
    return {'dg_u': (val, B, _all(g.E))}


def hvp_dgx(g, tgeo, g_eps, dg_eps, W, freq, env, use_mask=True, view=None, mut=()):
    v = view or R.View(g, use_mask)
    W = np.asarray(W, f64)
    nb = W.shape[1]
    val, B = np.zeros(g.E), np.zeros(g.E)
    if g.E:
        x = x_of(g)
        sel = np.flatnonzero(v.owner & v.live & (x < 1.0))
        dx = np.asarray(tgeo, f64)[sel, 3:4]
        r1, r2, A1, A2 = rbf_d12(x[sel], freq, env, mut)
        aW = np.abs(W).T
        e1, M1, L1 = r1 @ W.T, np.abs(r1) @ aW, A1 @ aW
        e2, M2, L2 = (r2 * dx) @ W.T, np.abs(r2 * dx) @ aW, (A2 * np.abs(dx)) @ aW
        ge, dge = np.asarray(g_eps, f64)[g.pid[sel]], np.asarray(dg_eps, f64)[g.pid[sel]]
        if 'no_eps2' in mut:
            e2 = 0 * e2
        val[sel] = (dge * e1 + ge * e2).sum(axis=1)
        B[sel] = ((2 * F + nb + 4) * U * (np.abs(dge) * M1 + np.abs(ge) * M2).sum(axis=1)
                  + FP64_ALLOWANCE * (np.abs(dge) * L1 + np.abs(ge) * L2).sum(axis=1))
    return {'dg_x': (val, B, _all(g.E))}


def hvp_out(g, g_x, g_u, dg_x, dg_u, tgeo, mut=()):
    """g: row_ptr, rev, geo, cutoff, N, E, i (the receiver of every edge); rev need not be an involution (planted)"""
    E, N = g.E, g.N
    L = np.asarray(g_x).reshape(-1, E).shape[0] if E else 1
    g_x, dg_x = (np.asarray(a, f64).reshape(L, E) for a in (g_x, dg_x))
    g_u, dg_u = (np.asarray(a, f64).reshape(L, E, 4)[:, :, :3] for a in (g_u, dg_u))
    use = L - 1 if ('last_layer_out' in mut and L > 1) else L
    gx, dgx, gu, dgu = g_x[:use].sum(0), dg_x[:use].sum(0), g_u[:use].sum(0), dg_u[:use].sum(0)
    Mx, Mdx, Mu, Mdu = np.abs(g_x).sum(0), np.abs(dg_x).sum(0), np.abs(g_u).sum(0), np.abs(dg_u).sum(0)
    geo, tgeo = np.asarray(g.geo, f64), np.asarray(tgeo, f64)
    u, r, du, rc = geo[:, :3], geo[:, 3:4], tgeo[:, :3], float(g.cutoff)
    dr = tgeo[:, 3:4] * rc
    dot = lambda a, b: (a * b).sum(axis=1, keepdims=True)  # noqa: E731
    gdu = dot(gu, u)
    a = gx[:, None] / rc - gdu / r
    sgn = -1.0 if 'sign_gdu_dr' in mut else 1.0
    da = dgx[:, None] / rc - (dot(dgu, u) + (0.0 if 'no_gu_du' in mut else dot(gu, du))) / r + sgn * gdu * dr / r ** 2
    Mgdu = dot(Mu, np.abs(u))
    Ma = Mx[:, None] / rc + Mgdu / r
    Mda = Mdx[:, None] / rc + (dot(Mdu, np.abs(u)) + dot(Mu, np.abs(du))) / r + Mgdu * np.abs(dr) / r ** 2
    gd, Bd = np.zeros((E, 4)), np.zeros((E, 4))
    gd[:, :3] = da * u + a * du + dgu / r - gu * dr / r ** 2
    Bd[:, :3] = (GEOM_C + L) * U * (Mda * np.abs(u) + Ma * np.abs(du) + Mdu / r + Mu * np.abs(dr) / r ** 2)
    rev = np.arange(E) if 'rev_as_e' in mut else np.asarray(g.rev)
    hv, Mh, Bh = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((N, 3))
    if E:
        np.add.at(hv, g.i, gd[:, :3] - gd[rev, :3])
        np.add.at(Mh, g.i, np.abs(gd[:, :3]) + np.abs(gd[rev, :3]))
        np.add.at(Bh, g.i, Bd[:, :3] + Bd[rev, :3])
    n = (np.diff(g.row_ptr).astype(f64)[:, None] + 3) * U
    return {'dg_d': (gd, Bd, _all(E)), 'hv': (hv, n * Mh + (1 + n) * Bh, _all(N))}


def voigt_numpy(e6, mut=()):
    h = 1.0 if 'voigt_no_half' in mut else 0.5
    e = np.asarray(e6, f64)
    return np.array([[e[0], h * e[5], h * e[4]], [h * e[5], e[1], h * e[3]], [h * e[4], h * e[3], e[2]]])


def strain_tan_geom(g, batch, eta6, n_edges=None, mut=()):
    E = g.E if n_edges is None else n_edges
    geo = np.asarray(g.geo, f64)[:E]
    u, r, rc = geo[:, :3], geo[:, 3:4], float(g.cutoff)
    eta = np.stack([voigt_numpy(e, mut) for e in np.asarray(eta6)])[np.asarray(batch)[g.i[:E]]] if E else np.zeros((0, 3, 3))
    d = r * np.einsum('ekl,el->ek', eta, u)
    Md = r * np.einsum('ekl,el->ek', np.abs(eta), np.abs(u))
    dr = (u * d).sum(axis=1, keepdims=True)
    Mr = (np.abs(u) * Md).sum(axis=1, keepdims=True)
    t = np.concatenate([(d - u * dr) / r, dr / rc], axis=1)
    B = np.concatenate([20 * U * (Md + np.abs(u) * Mr) / r, 18 * U * Mr / rc], axis=1)
    return {'tgeo': (t, B, _all(E))}


VOIGT_SUMS = ((0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (1, 2, 2, 1), (0, 2, 2, 0), (0, 1, 1, 0))   # I: (a, b) and (b, a)


def strain_born(dg_d, geo, row_ptr, mol_ptr, mut=(), dtype=f32):
    """dtype: what the inputs are (float64: the chained CPU check)"""
    n_mol = len(mol_ptr) - 1
    dg = np.asarray(dg_d, dtype)[:, :3].astype(LD)
    geo = np.asarray(geo, dtype).astype(LD)
    d = geo[:, 3:4] * geo[:, :3]
    val, B = np.zeros((n_mol, 6)), np.zeros((n_mol, 6))
    for b in range(n_mol):
        a0, a1 = int(mol_ptr[b]), int(mol_ptr[b + 1])
        if 'born_lane64' in mut:
            a1 = min(a1, a0 + 64)
        lo, hi = (int(row_ptr[a0]), int(row_ptr[a1])) if a1 > a0 else (0, 0)
        t = dg[lo:hi, :, None] * d[lo:hi, None, :]
        S, M = t.sum(axis=0), np.abs(t).sum(axis=0)
        for I, (p, q, s, w) in enumerate(VOIGT_SUMS):
            second = S[p, q] if ('s5_twice' in mut and I == 3) else S[s, w]
            val[b, I] = float(LD(0.5) * (S[p, q] + second))
            B[b, I] = U * abs(val[b, I]) + BORN_ALLOWANCE * float(LD(0.5) * (M[p, q] + M[s, w]))
    return {'d2': (val, B, _all(n_mol))}


def hess_dirs(batch, mol_ptr, k, n_rep, n_mol0):
    """v [N][3] of pass k (exact)"""
    batch, mol_ptr = np.asarray(batch, np.int64), np.asarray(mol_ptr, np.int64)
    n = batch.size
    a = np.arange(n) - mol_ptr[batch]
    nb = mol_ptr[batch + 1] - mol_ptr[batch]
    d = k * n_rep + batch // n_mol0
    on = (d < 3 * nb) & (a == d // 3)
    v = np.zeros((n, 3), f32)
    v[np.flatnonzero(on), (d % 3)[on]] = 1.0
    return v


def hess_scatter(hv, batch, mol_ptr, blk_ptr, k, n_rep, n_mol0, mut=()):
    """(flat indices into blocks, values) that pass k writes; blk_ptr has one entry per molecule of the batch when the mutation
    that forgets b % n_mol0 is asked for (the offsets a kernel without it would read)"""
    batch, mol_ptr, blk_ptr = np.asarray(batch, np.int64), np.asarray(mol_ptr, np.int64), np.asarray(blk_ptr, np.int64)
    n = batch.size
    a = np.arange(n) - mol_ptr[batch]
    nb = mol_ptr[batch + 1] - mol_ptr[batch]
    d = k * n_rep + batch // n_mol0
    on = np.flatnonzero(d < 3 * nb)
    slot = batch if 'scatter_no_mod' in mut else batch % n_mol0
    c = np.arange(3)[None, :]
    idx = blk_ptr[slot[on]][:, None] + (3 * a[on][:, None] + c) * (3 * nb[on][:, None]) + d[on][:, None]
    return idx.reshape(-1), np.asarray(hv, f32).reshape(n, 3)[on].reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' own order of operations in fp32 (numpy on the host): "the bound really bounds"
# ---------------------------------------------------------------------------------------------------------------------------
def wave_sum32(v):
    """the xor butterfly of 64 lanes (offsets 32 .. 1) on the last axis, in the array's own precision: every lane's total"""
    lanes = np.arange(64)
    o = 32
    while o:
        v = v + v[..., lanes ^ o]
        o >>= 1
    return v[..., 0]


def dgu32(g, gf, dgf, phi1, dphi1, use_mask=True):
    out = np.zeros((g.E, 4), f32)
    if not g.E:
        return out
    gf, dgf = (np.asarray(a, f32).reshape(g.N, 3, 64, 2)[g.i] for a in (gf, dgf))
    v1, w1 = (np.asarray(a, f32).reshape(-1, 1, 64, 2)[g.pid] for a in (phi1, dphi1))
    t = R.fma32(dgf[..., 0], v1[..., 0], R.fma32(dgf[..., 1], v1[..., 1], R.fma32(gf[..., 0], w1[..., 0], gf[..., 1] * w1[..., 1])))
    out[:, :3] = wave_sum32(t)
    if use_mask:
        out[g.masked] = 0
    return out


def dgx32(g, tgeo, g_eps, dg_eps, W, freq, env, use_mask=True):
    """hvp_dgx_kernel: the basis derivatives by the kernel's own factored formulas in float64, rounded once; the fused chains over
    the basis; the lane products and the butterfly"""
    out = np.zeros(g.E, f32)
    if not g.E:
        return out
    W = np.asarray(W, f32)
    nb = W.shape[1]
    x = x_of(g)
    live = ~g.masked if use_mask else _all(g.E)
    sel = np.flatnonzero((g.i < g.j) & live & (x < 1.0))
    xs = x[sel][:, None]
    env = env if env else 9
    if env == ENV_COSINE:
        e, de, dde = 0.5 * (1 + np.cos(np.pi * xs)), -0.5 * np.pi * np.sin(np.pi * xs), -0.5 * np.pi ** 2 * np.cos(np.pi * xs)
    else:
        p = float(env)
        K = 0.5 * p * (p + 1) * (p + 2)
        xp = xs ** p
        e = 1 - 0.5 * (p + 1) * (p + 2) * xp + p * (p + 2) * xp * xs - 0.5 * p * (p + 1) * xp * xs * xs
        de = -K * xs ** (p - 1) * (1 - xs) * (1 - xs)
        dde = -K * xs ** (p - 2) * (1 - xs) * ((p - 1) - (p + 1) * xs) if env >= 2 else 2 * K * (1 - xs)
    w = np.asarray(freq, f32).astype(f64)[None, :]
    b = np.sin(w * xs) / xs
    db = (w * np.cos(w * xs) - b) / xs
    ddb = -w * w * b - 2 * db / xs
    dx = np.asarray(tgeo, f32)[sel, 3:4].astype(f64)
    my1 = (de * b + e * db).astype(f32)
    my2 = ((dde * b + 2 * de * db + e * ddb) * dx).astype(f32)
    e1, e2 = np.zeros((sel.size, F), f32), np.zeros((sel.size, F), f32)
    for n in range(nb):
        e1 = R.fma32(W[None, :, n], my1[:, n:n + 1], e1)
        e2 = R.fma32(W[None, :, n], my2[:, n:n + 1], e2)
    ge, dge = (np.asarray(a, f32)[g.pid[sel]].reshape(-1, 64, 2) for a in (g_eps, dg_eps))
    e1, e2 = e1.reshape(-1, 64, 2), e2.reshape(-1, 64, 2)
    t = R.fma32(dge[..., 0], e1[..., 0], R.fma32(dge[..., 1], e1[..., 1], R.fma32(ge[..., 0], e2[..., 0], ge[..., 1] * e2[..., 1])))
    out[sel] = wave_sum32(t)
    return out


def out32(g, g_x, g_u, dg_x, dg_u, tgeo):
    """hvp_geom_kernel and hvp_rows_kernel, every operation rounded on its own (no contraction)"""
    E, N = g.E, g.N
    L = np.asarray(g_x).reshape(-1, E).shape[0] if E else 1
    g_x, dg_x = (np.asarray(a, f32).reshape(L, E) for a in (g_x, dg_x))
    g_u, dg_u = (np.asarray(a, f32).reshape(L, E, 4)[:, :, :3] for a in (g_u, dg_u))
    gx, dgx, gu, dgu = np.zeros(E, f32), np.zeros(E, f32), np.zeros((E, 3), f32), np.zeros((E, 3), f32)
    for l in range(L):
        gx, dgx, gu, dgu = gx + g_x[l], dgx + dg_x[l], gu + g_u[l], dgu + dg_u[l]
    geo, t = np.asarray(g.geo, f32), np.asarray(tgeo, f32)
    u, du = geo[:, :3], t[:, :3]
    ir, inv_rc = f32(1) / geo[:, 3], f32(1) / f32(g.cutoff)
    dr = t[:, 3] * f32(g.cutoff)
    dot = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]  # noqa: E731
    gdu = dot(gu, u)
    a = gx * inv_rc - gdu * ir
    s6 = dgu[:, 0] * u[:, 0] + dgu[:, 1] * u[:, 1] + dgu[:, 2] * u[:, 2] + gu[:, 0] * du[:, 0] + gu[:, 1] * du[:, 1] + gu[:, 2] * du[:, 2]
    da = dgx * inv_rc - s6 * ir + gdu * dr * ir * ir
    q = dr * ir * ir
    gd = np.zeros((E, 4), f32)
    for k in range(3):
        gd[:, k] = da * u[:, k] + a * du[:, k] + dgu[:, k] * ir - gu[:, k] * q
    hv = np.zeros((N, 3), f32)
    for i in range(N):
        acc = np.zeros(3, f32)
        for e in range(int(g.row_ptr[i]), int(g.row_ptr[i + 1])):
            acc = acc + (gd[e, :3] - gd[int(g.rev[e]), :3])
        hv[i] = acc
    return gd, hv


def strain_tan32(g, batch, eta6, n_edges=None):
    E = g.E if n_edges is None else n_edges
    geo = np.asarray(g.geo, f32)[:E]
    e6 = np.asarray(eta6, f32)[np.asarray(batch)[g.i[:E]]].reshape(E, 6)
    m = [e6[:, 0], e6[:, 1], e6[:, 2], f32(0.5) * e6[:, 3], f32(0.5) * e6[:, 4], f32(0.5) * e6[:, 5]]
    ux, uy, uz, r = geo[:, 0], geo[:, 1], geo[:, 2], geo[:, 3]
    dx = r * (m[0] * ux + m[5] * uy + m[4] * uz)
    dy = r * (m[5] * ux + m[1] * uy + m[3] * uz)
    dz = r * (m[4] * ux + m[3] * uy + m[2] * uz)
    dr = ux * dx + uy * dy + uz * dz
    ir = f32(1) / r
    inv_rc = f32(1) / f32(g.cutoff)
    return np.stack([(dx - ux * dr) * ir, (dy - uy * dr) * ir, (dz - uz * dr) * ir, dr * inv_rc], axis=1).astype(f32)


def born64(dg_d, geo, row_ptr, mol_ptr):
    """strain_born_kernel: lane = atom row modulo 64, fp64 accumulators, the butterfly, one rounding"""
    n_mol = len(mol_ptr) - 1
    dg = np.asarray(dg_d, f32)[:, :3].astype(f64)
    geo = np.asarray(geo, f32).astype(f64)
    d = geo[:, 3:4] * geo[:, :3]
    out = np.zeros((n_mol, 6), f32)
    for b in range(n_mol):
        s = np.zeros((9, 64))
        for i in range(int(mol_ptr[b]), int(mol_ptr[b + 1])):
            lane = (i - int(mol_ptr[b])) % 64
            for e in range(int(row_ptr[i]), int(row_ptr[i + 1])):
                s[:, lane] += (dg[e][:, None] * d[e][None, :]).reshape(9)
        s = wave_sum32(s)
        out[b] = [s[0], s[4], s[8], 0.5 * (s[5] + s[7]), 0.5 * (s[2] + s[6]), 0.5 * (s[1] + s[3])]
    return out


def ratio(got, ref):
    """the largest |got - ref| / bound over the defined entries (inf where a bound of 0 is missed)"""
    val, B, defined = ref
    got = np.asarray(got, f64).reshape(val.shape)
    if not val.size:
        return 0.0
    err = np.abs(got - val)
    bad = ~np.isfinite(err)
    r = np.where(B > 0, err / np.where(B > 0, B, 1.0), np.where(err > 0, np.inf, 0.0))
    r = np.where(bad, np.inf, r)
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------------------------
# the cases: the same for the CPU restatements (tests/test_hvp_ref_host.py) and the kernels (tests/test_hip_hvp_stages.py)
# ---------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(('hvp stages',) + key).encode()))


def _r(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape, dtype=f32) * f32(scale)).astype(f32)


def chain_graph(n, seed=11):
    """n atoms in one molecule joined in a chain (n - 1 pairs)"""
    return R.stage_graph([(a, a + 1) for a in range(n - 1)], [n] if n else [], seed=seed)


def complete_graph(n=96):
    """every pair of n atoms: n (n - 1) = 9120 directed edges at n = 96, more than the 8192 one trip of hvp_dgx's grid covers"""
    return R.stage_graph([(a, b) for a in range(n) for b in range(a + 1, n)], [n], seed=13)


def last_r_inside(cutoff):
    """the largest fp32 r whose x (x_of) is below 1, and the next fp32 number"""
    inv_rc = f64(f32(1.0) / f32(cutoff))
    r = f32(cutoff) * f32(1.0 + 2.0 ** -20)
    while f64(r) * inv_rc >= 1.0:
        r = np.nextafter(r, f32(0))
    return r, np.nextafter(r, f32(np.inf))


def edges_graph():
    """a chain of 9 atoms whose pairs sit at planted distances: x = 0.02, the last r inside the cutoff and the first outside,
    each once on both directions of a pair, and once on the owner's direction alone"""
    g = chain_graph(9, seed=17)
    inside, outside = last_r_inside(g.cutoff)
    r = {0: f32(0.02 * g.cutoff), 1: inside, 2: outside, 3: f32(0.02 * g.cutoff), 4: inside, 5: outside}
    for e in range(g.E):
        p = int(g.pid[e])
        if p in r and (p < 3 or g.own[e]):
            g.geo[e, 3] = r[p]
    return g


_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        make = dict(R.GRAPHS, complete=complete_graph, edges=edges_graph)
        if name in make:
            _GRAPHS[name] = make[name]()
        else:
            kind, n = name.split(' ')
            _GRAPHS[name] = chain_graph(int(n)) if kind == 'chain' else R.graph_trivial(int(n))
    return _GRAPHS[name]


DGU_CASES = (('degrees', True), ('wide row', True), ('molecules', True), ('masked', True), ('masked', False), ('chain 1', True),
             ('chain 3', True), ('chain 4', True), ('chain 5', True), ('chain 33', True))


def dgu_inputs(name):
    g = graph(name)
    d = R.stage_inputs(g)
    return g, {k: d[k] for k in ('gf', 'dgf', 'phi1', 'dphi1')}


def basis_weights(nb):
    rng = _rng('W', nb)
    return ((rng.random((F, nb)) * 2 - 1) / np.sqrt(nb)).astype(f32), (np.arange(1, nb + 1) * np.pi).astype(f32)


# (graph, n_basis, envelope, xg passed, every directed edge its own pair row)
DGX_CASES = (tuple(('degrees', nb, 9, True, False) for nb in (1, 8, 20, 32))
             + tuple(('degrees', 20, env, True, False) for env in (0, 1, 2, 3, ENV_COSINE))
             + tuple(('edges', 20, env, True, False) for env in ENVELOPES)
             + (('masked', 20, 9, True, False), ('masked', 20, 9, False, False), ('degrees', 20, 9, True, True),
                ('edges', 8, 1, True, True), ('complete', 20, 9, True, False)))


def dgx_inputs(name, nb, own_rows):
    """tgeo [E][4] is drawn per DIRECTED edge, so the two directions of a pair differ; own_rows: pid = e, so g_eps / dg_eps differ
    between the two directions as well"""
    g = graph(name)
    if own_rows:
        g = R.Graph(**dict(g.__dict__, pid=np.arange(g.E, dtype=np.int32)))
    rng = _rng('dgx', name, nb, own_rows)
    rows = g.E if own_rows else g.P
    W, freq = basis_weights(nb)
    return g, dict(tgeo=_r(rng, g.E, 4), g_eps=_r(rng, rows, F), dg_eps=_r(rng, rows, F), W=W, freq=freq)


def planted_rows(n_atoms, n_edges, seed, empty=(), cutoff=5.0):
    """a CSR of n_edges edges over n_atoms rows (the rows in `empty` stay without edges), rev a random permutation, u random unit
    vectors, r in (0.12, 0.97) cutoff: what hvp_out and strain_born read of a graph, at any size"""
    rng = _rng('rows', n_atoms, n_edges, seed)
    ok = np.array([a for a in range(n_atoms) if a not in set(empty)], np.int64)
    i = np.sort(ok[rng.integers(0, ok.size, n_edges)]) if n_edges else np.zeros(0, np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n_atoms))]).astype(np.int32)
    u = rng.standard_normal((n_edges, 3))
    u = u / np.linalg.norm(u, axis=1, keepdims=True)
    geo = np.concatenate([u, cutoff * rng.uniform(0.12, 0.97, (n_edges, 1))], axis=1).astype(f32)
    rev = rng.permutation(n_edges).astype(np.int32)
    j = rng.integers(0, max(n_atoms, 1), n_edges)
    return R.Graph(N=n_atoms, E=n_edges, row_ptr=row_ptr, rev=rev, geo=geo, cutoff=float(cutoff), edge_index=np.stack([i, j]),
                   masked=np.zeros(n_edges, bool))


def short_edge_rows():
    """one edge at r = 0.05 A among edges at 4.9 A"""
    g = planted_rows(7, 24, 3, empty=(2,))
    g.geo[:, 3] = f32(4.9)
    g.geo[5, 3] = f32(0.05)
    return g


# (name, n_layers)
OUT_CASES = (('rows 255', 1), ('rows 256', 3), ('rows 257', 8), ('wide row', 3), ('short edge', 3), ('degrees', 8))


def out_inputs(name, L):
    if name.startswith('rows '):
        n = int(name.split(' ')[1])
        g = planted_rows(n, n, n, empty=(0, n // 2, n - 1))
    elif name == 'short edge':
        g = short_edge_rows()
    else:
        g = graph(name)
    rng = _rng('out', name, L)
    d = dict(g_x=_r(rng, L, g.E), g_u=_r(rng, L, g.E, 4), dg_x=_r(rng, L, g.E), dg_u=_r(rng, L, g.E, 4), tgeo=_r(rng, g.E, 4))
    d['g_u'][..., 3] = NAN_MARK            # (tgeo[e][3] is dx, an operand: only these two fourth lanes are padding)
    d['dg_u'][..., 3] = NAN_MARK
    return g, d


STRAIN_SIZES = (10, 12, 14)
STRAIN_EDGES = (1, 255, 257, None)


def strain_inputs():
    """three fully connected systems (90 + 132 + 182 = 404 directed edges): a general strain, pure shears and no strain"""
    pairs, a0 = [], 0
    for n in STRAIN_SIZES:
        pairs += [(a0 + a, a0 + b) for a in range(n) for b in range(a + 1, n)]
        a0 += n
    g = R.stage_graph(pairs, list(STRAIN_SIZES), seed=19)
    rng = _rng('strain')
    eta6 = np.zeros((3, 6), f32)
    eta6[0] = _r(rng, 6)
    eta6[1, 3:] = _r(rng, 3)
    batch = np.repeat(np.arange(3), STRAIN_SIZES).astype(np.int64)
    return g, batch, eta6


BORN_SIZES = (0, 1, 63, 64, 65, 130)


def born_inputs(swap=False):
    """systems of 0, 1, 63, 64, 65 and 130 atoms: chains with gaps (atoms of degree 0 at local index 4, 11, 18, ...) and a few long
    pairs.  swap: the x and y components of dg_d and of u exchanged, which exchanges S_01 and S_10."""
    pairs, a0 = [], 0
    rng = _rng('born')
    for n in BORN_SIZES:
        pairs += [(a0 + k, a0 + k + 1) for k in range(n - 1) if k % 7 not in (3, 4)]
        pairs += [(a0 + int(a), a0 + int(b)) for a, b in rng.integers(0, max(n, 1), (n // 4, 2)) if a != b and a % 7 != 4 and b % 7 != 4]
        a0 += n
    g = R.stage_graph(pairs, list(BORN_SIZES), seed=23)
    dg_d = _r(rng, g.E, 4)
    dg_d[:, 3] = NAN_MARK
    geo = g.geo.copy()
    if swap:
        dg_d[:, [0, 1]] = dg_d[:, [1, 0]]
        geo[:, [0, 1]] = geo[:, [1, 0]]
    return g, dg_d, geo


HESS_SIZES = (1, 2, 8, 9, 0)
HESS_REPS = (1, 2, 3, 5)


def hess_inputs(n_rep):
    """n_rep replicas of molecules of 1, 2, 8, 9 atoms and an empty slot: (batch, mol_ptr, blk_ptr, n_mol0, block elements)"""
    sizes = np.array(HESS_SIZES * n_rep, np.int64)
    mol_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    batch = np.repeat(np.arange(sizes.size), sizes).astype(np.int64)
    nb = np.array(HESS_SIZES, np.int64)
    blk_ptr = np.concatenate([[0], np.cumsum(9 * nb * nb)]).astype(np.int64)
    return batch, mol_ptr, blk_ptr[:-1].copy(), len(HESS_SIZES), int(blk_ptr[-1])


def hess_hv(n_atoms, k):
    """a column with a different value in every (pass, atom, component)"""
    return (1.0 + np.arange(3 * n_atoms, dtype=f32).reshape(n_atoms, 3) + f32(1000.0) * k).astype(f32)
