"""Float64 statements of the row-local node stages (csrc/node128.hip, csrc/node128s.hip), of the four LayerNorm kernels
(csrc/edge.hip, csrc/train.hip) and of the elementwise update tangents (csrc/train.hip), each with a COMPONENTWISE error bound
computed in float64 from the magnitudes, in the style of tests/edge_ref.py: every statement returns {output: (value, bound,
defined)}.  tests/test_hip_node_stages.py asserts |got - ref| <= bound element by element; tests/test_node_ref_host.py checks
the statements against autograd, checks that an fp32 restatement of each kernel's own order of operations (`restate`) stays inside
the bounds, and that wrong kernels (`MUTATIONS`) leave them.

Products are dense_ref.product: form SPLIT for the kernels that read weight images (hi + lo f16 pieces scaled by the row's /
the matrix's largest element), FP32 for the others; an operand that is itself computed carries its bound in as dA_in.  A weight
argument M always enters as X M^T: the `*T` arguments are the transposed matrices the interface takes.
Elementwise steps, u = 2^-24:
    c = a b                 |a| db + |b| da + da db + u |c|
    k fused / plain adds    k u (sum of the magnitudes of the terms)
    act / act' / act'' of an input                 dense_ref.act_eval_err
    act / act' of a COMPUTED x with bound dx       + L dx, L the largest slope of the function on [x - dx, x + dx]
LayerNorm (one wave per row, lane l on features 2 l, 2 l + 1; a sum of 128 terms is one pair add and a 6-level butterfly, the
mean one more product: 9 u mean|terms|):
    mean      9 u mean|x|
    x - mean  u (|x| + |mean|) + d mean          <- the condition number: this absolute error is multiplied by rstd below, so a
                                                    row of mean 1e3 and spread 1e-2 is resolved to 1e3 u / 1e-2 = 6e-3 only
    var       mean(2 |dx| d dx) + 10 u var
    rstd      rstd ((d var + u (var + eps)) / (2 (var + eps)) + 3 u)     (sqrt and divide are correctly rounded: u each)
    xhat      rstd d dx + |dx| d rstd + u |xhat|;   y = xhat gamma + beta: |gamma| d xhat + u |y|
Rows whose largest magnitude has an exponent field below 40 (2^-87) are not scaled by the split (csrc/mlp128s.hip: pow2_scale)
and lose their f16 pieces to underflow: the cases keep their row maxima above it."""
import zlib

import numpy as np

from tests import dense_ref as D
from tests.edge_ref import tree_sum32

U = D.U
F = 128
FP32, SPLIT = D.FP32, D.SPLIT
EPS = 1e-5
N_ELEMENTS = 119
NODE_ROWS = (1, 5, 31, 32, 33, 63, 97)          # 32-row tiles
WAVE_ROWS = (1, 3, 4, 5, 33)                    # 4 rows per 256-thread block
f32 = np.float32


def _f64(a):
    return np.asarray(a, np.float64)


def _all(n):
    return np.ones(n, bool)


def _none(n):
    return np.zeros(n, bool)


def mul(a, da, b, db):
    """(a b, bound) for operands with bounds da, db (None: exact)"""
    c = a * b
    B = U * np.abs(c)
    if da is not None:
        B = B + np.abs(b) * da
    if db is not None:
        B = B + np.abs(a) * db
    if da is not None and db is not None:
        B = B + da * db
    return c, B


def slope(fn, name, x, dx):
    """the largest |fn'| on [x - dx, x + dx] to first order: fn = dense_ref.dact for act, dense_ref.d2act for act'.  The three
    points cover the monotone derivatives of the kinked activations exactly and the smooth ones up to dx |fn''|, which the 1 %
    and the dx term pay for (|act'''| <= 1 for every activation of the factory)."""
    return 1.01 * np.maximum(np.maximum(np.abs(fn(name, x - dx)), np.abs(fn(name, x + dx))), np.abs(fn(name, x))) + dx


# ---------------------------------------------------------------------------------------------------------------------------
# node stages
# ---------------------------------------------------------------------------------------------------------------------------
def _update(f, Wu, form, a_mid):
    """q_k = f_k Wu^T; a_out = a_mid + sum_k f_k q_k"""
    q, Bq = np.empty_like(f), np.empty_like(f)
    for k in range(3):
        q[:, k], Bq[:, k] = D.product(f[:, k], Wu, form)
    mag = np.abs(a_mid) + (np.abs(f) * (np.abs(q) + Bq)).sum(axis=1)
    a = a_mid + (f * q).sum(axis=1)
    return q, Bq, a, (np.abs(f) * Bq).sum(axis=1) + 4 * U * mag


def _got(got, key, val, B):
    """the kernel's own stored value of an intermediate, as an exact operand of what follows it (so that the next product is judged
    alone, as dense_ref.mlp does with H_got); without it the statement's value and its bound are chained"""
    if got is not None and key in got:
        return _f64(got[key]), None
    return val, B


def _prod_got(vb, W, form):
    return D.product(vb[0], W, form, vb[1])


def _mlp_tail(a, Ba, W0, b0, W2, b2, act, form, hn_got=None):
    hn, Bhn = D.product(a, W0, form, Ba)
    hn = hn + b0
    Bhn = Bhn + U * np.abs(hn)
    if hn_got is not None:
        hs = _f64(hn_got)
        m, Bm = D.product(D.act(act, hs), W2, form, D.act_eval_err(hs))
    else:
        m, Bm = D.product(D.act(act, hn), W2, form, D.act_eval_err(hn) + slope(D.dact, act, hn, Bhn) * Bhn)
    m = m + b2
    return hn, Bhn, m, Bm + U * np.abs(m)


def node_fwd(f, a_mid, Wu, W0=None, b0=None, W2=None, b2=None, act='silu', form=FP32, store_q=True, got=None):
    """got: {'a_out', 'hn'} as the kernel stored them -- hn is then judged from that a_out and m from that hn"""
    f, a_mid = _f64(f), _f64(a_mid)
    n = f.shape[0]
    q, Bq, a, Ba = _update(f, _f64(Wu), form, a_mid)
    out = {'q': (q, Bq, _all(n) if store_q else _none(n)), 'a_out': (a, Ba, _all(n))}
    if W0 is not None:
        hn, Bhn, m, Bm = _mlp_tail(*_got(got, 'a_out', a, Ba), _f64(W0), _f64(b0), _f64(W2), _f64(b2), act, form,
                                   None if got is None else got.get('hn'))
        out['hn'], out['m'] = (hn, Bhn, _all(n)), (m, Bm, _all(n))
    else:
        z = np.zeros((n, F))
        out['hn'], out['m'] = (z, z, _none(n)), (z, z, _none(n))
    return out


def _mlp_adjoint(g_top, Bg_top, h, Bh, W2T, W0T, act, form):
    """t = g_top W2T^T; g_hn = t act'(h); g_a = g_hn W0T^T"""
    t, Bt = D.product(g_top, W2T, form, Bg_top)
    d = D.dact(act, h)
    dd = D.act_eval_err(h) + (slope(D.d2act, act, h, Bh) * Bh if Bh is not None else 0.0)
    g, Bg = mul(t, Bt, d, dd)
    ga, Bga = D.product(g, W0T, form, Bg)
    return t, Bt, ga, Bga


def _update_adjoint(ga, Bga, f, q, Bq, G_f, WuT, form):
    """gf_k = G_f,k + g_a q_k + (g_a f_k) WuT^T"""
    gf, Bgf = np.empty_like(f), np.empty_like(f)
    for k in range(3):
        x, Bx = mul(ga, Bga, f[:, k], None)
        o, Bo = D.product(x, WuT, form, Bx)
        gq, Bgq = mul(ga, Bga, q[:, k], None if Bq is None else Bq[:, k])
        g0 = 0.0 if G_f is None else G_f[:, k]
        gf[:, k] = o + gq + g0
        Bgf[:, k] = Bo + Bgq + 3 * U * (np.abs(o) + Bo + np.abs(gq) + Bgq + np.abs(g0))
    return gf, Bgf


def node_bwd(g_a, g_top=None, h_top=None, W2T=None, W0T=None, acc_ga=0, f=None, q=None, G_f=None, WuT=None, Wu=None, act='silu',
             form=FP32, want_T=False, g_a_in=None, got=None):
    """got: {'g_a'} as the kernel stored it -- gf is then judged from that g_a.
    MLP part when W2T is given, update part when WuT is given; q None: formed again as f Wu^T (Wu: the matrix of the image)"""
    g_a = _f64(g_a)
    n = g_a.shape[0]
    z = np.zeros((n, F))
    out = {'T': (z, z, _none(n)), 'gf': (np.zeros((n, 3, F)), np.zeros((n, 3, F)), _none(n))}
    ga, Bga = g_a, None
    if W2T is not None:
        t, Bt, ga, Bga = _mlp_adjoint(_f64(g_top), None, _f64(h_top), None, _f64(W2T), _f64(W0T), act, form)
        if acc_ga:
            ga = ga + (g_a if g_a_in is None else _f64(g_a_in))
            Bga = Bga + U * np.abs(ga)
        out['T'] = (t, Bt, _all(n) if want_T else _none(n))
        out['g_a'] = (ga, Bga, _all(n))
        ga, Bga = _got(got, 'g_a', ga, Bga)
    else:
        out['g_a'] = (g_a, np.zeros_like(g_a), _all(n))          # left as it was
    if WuT is not None:
        f = _f64(f)
        if q is None:
            qv, Bq = np.empty_like(f), np.empty_like(f)
            for k in range(3):
                qv[:, k], Bq[:, k] = D.product(f[:, k], _f64(Wu), form)
        else:
            qv, Bq = _f64(q), None
        gf, Bgf = _update_adjoint(ga, Bga, f, qv, Bq, None if G_f is None else _f64(G_f), _f64(WuT), form)
        out['gf'] = (gf, Bgf, _all(n))
    return out


def node_turn(f, a_mid, Wu, W0, b0, W2, b2, w4, b4, scale, shift, z, W2T, W0T, WuT, act='silu', form=SPLIT, got=None):
    """node_fwd into the head, the head tail, the head adjoint and the update adjoint with G_f = 0.  e1, e2, g_e2 stay on chip: their
    bounds are chained through five products, each of which multiplies the bound by the row sums of |W| -- a valid but weak bound.
    got: {'a_out', 'e1', 'e2', 'g_e2', 'g_a'} as the three-launch composition stored them (whose bits the kernel must reproduce):
    every output is then judged from the stored intermediate in front of it."""
    f, a_mid, w4 = _f64(f), _f64(a_mid), _f64(w4)
    n = f.shape[0]
    z = np.asarray(z)
    q, Bq, a, Ba = _update(f, _f64(Wu), form, a_mid)
    e1, Be1, e2, Be2 = _mlp_tail(a, Ba, _f64(W0), _f64(b0), _f64(W2), _f64(b2), act, form)
    e1, Be1 = _got(got, 'e1', e1, Be1)
    e2, Be2 = _got(got, 'e2', e2, Be2)
    if Be2 is None:
        Be2 = np.zeros_like(e2)
    b4 = float(np.asarray(b4).reshape(-1)[0])
    sc = np.ones(n) if scale is None else _f64(scale)[z]
    sh = np.zeros(n) if shift is None else _f64(shift)[z]
    av = D.act(act, e2)
    Bav = D.act_eval_err(e2) + slope(D.dact, act, e2, Be2) * Be2
    s = av @ w4
    Bs = (F + 2) * U * ((np.abs(av) + Bav) @ np.abs(w4)) + Bav @ np.abs(w4)
    ae = (s + b4) * sc + sh
    Bae = np.abs(sc) * Bs + 2 * U * (np.abs(sc) * (np.abs(s) + Bs + abs(b4)) + np.abs(sh))
    d = D.dact(act, e2)
    Bd = D.act_eval_err(e2) + slope(D.d2act, act, e2, Be2) * Be2
    ge = sc[:, None] * w4 * d
    Bge = np.abs(sc[:, None] * w4) * Bd + 3 * U * (np.abs(ge) + np.abs(sc[:, None] * w4) * Bd)
    _, _, ga, Bga = _mlp_adjoint(*_got(got, 'g_e2', ge, Bge), e1, Be1, _f64(W2T), _f64(W0T), act, form)
    gf, Bgf = _update_adjoint(*_got(got, 'g_a', ga, Bga), f, q, Bq, None, _f64(WuT), form)
    return {'a_out': (a, Ba, _all(n)), 'atom_energy': (ae, Bae, _all(n)), 'g_a': (ga, Bga, _all(n)), 'gf': (gf, Bgf, _all(n))}


def node_tan_fwd(df, f, q, da_mid, hn, Wu, W0, W2, act='silu', form=SPLIT, got=None):
    """got: {'da_out', 'T'} as stored.
    dq_k = df_k Wu^T; da_out = da_mid + sum_k (df_k q_k + f_k dq_k); T = da_out W0^T; Y = (T act'(hn)) W2^T"""
    df, f, q, da_mid, hn = (_f64(t) for t in (df, f, q, da_mid, hn))
    n = f.shape[0]
    dq, Bdq = np.empty_like(f), np.empty_like(f)
    for k in range(3):
        dq[:, k], Bdq[:, k] = D.product(df[:, k], _f64(Wu), form)
    a = da_mid + (df * q + f * dq).sum(axis=1)
    mag = np.abs(da_mid) + (np.abs(df * q) + np.abs(f) * (np.abs(dq) + Bdq)).sum(axis=1)
    Ba = (np.abs(f) * Bdq).sum(axis=1) + 7 * U * mag
    T, BT = _prod_got(_got(got, 'da_out', a, Ba), _f64(W0), form)
    g, Bg = mul(*_got(got, 'T', T, BT), D.dact(act, hn), D.act_eval_err(hn))
    Y, BY = D.product(g, _f64(W2), form, Bg)
    return {'dq': (dq, Bdq, _all(n)), 'da_out': (a, Ba, _all(n)), 'T': (T, BT, _all(n)), 'Y': (Y, BY, _all(n))}


def node_tan_bwd(dga, g_top=None, h_top=None, t2_top=None, hd_top=None, W2T=None, W0T=None, acc_dga=0, ga=None, f=None, df=None,
                 q=None, dq=None, dgf_in=None, WuT=None, act='silu', form=SPLIT, got=None):
    """got: {'G', 'dga', 'dgq'} as stored.
    part A (g_top given): dT = g_top W2T^T; G = dT act'(h) + t2 act''(h) hd; dga (+)= G W0T^T.
    part B (f given): gq_k = ga f_k; dgq_k = dga f_k + ga df_k; dgf_k = dgf_in,k + dga q_k + ga dq_k + dgq_k WuT^T"""
    dga = _f64(dga)
    n = dga.shape[0]
    z, z3 = np.zeros((n, F)), np.zeros((n, 3, F))
    out = {'G': (z, z, _none(n))}
    for k in ('gq', 'dgq', 'dgf'):
        out[k] = (z3, z3, _none(n))
    d, Bd = dga, None
    if g_top is not None:
        h = _f64(h_top)
        dT, BdT = D.product(_f64(g_top), _f64(W2T), form)
        G, BG = mul(dT, BdT, D.dact(act, h), D.act_eval_err(h))
        if t2_top is not None:
            th = _f64(t2_top) * _f64(hd_top)
            second = th * D.d2act(act, h)
            BG = BG + np.abs(th) * D.act_eval_err(h) + 2 * U * np.abs(second) + U * (np.abs(G) + np.abs(second))
            G = G + second
        d, Bd = _prod_got(_got(got, 'G', G, BG), _f64(W0T), form)
        if acc_dga:
            d = d + dga
            Bd = Bd + U * np.abs(d)
        out['G'] = (G, BG, _all(n))
        out['dga'] = (d, Bd, _all(n))
        d, Bd = _got(got, 'dga', d, Bd)
    else:
        out['dga'] = (dga, np.zeros_like(dga), _all(n))
    if f is not None:
        ga, f, df, q, dq = (_f64(t) for t in (ga, f, df, q, dq))
        gq, dgq, dgf = np.empty_like(f), np.empty_like(f), np.empty_like(f)
        Bgq, Bdgq, Bdgf = np.empty_like(f), np.empty_like(f), np.empty_like(f)
        for k in range(3):
            gq[:, k], Bgq[:, k] = mul(ga, None, f[:, k], None)
            p1, B1 = mul(d, Bd, f[:, k], None)
            p2 = ga * df[:, k]
            dgq[:, k] = p1 + p2
            Bdgq[:, k] = B1 + 2 * U * (np.abs(p1) + np.abs(p2))
            o, Bo = D.product(_f64(got['dgq'])[:, k], _f64(WuT), form) if got is not None and 'dgq' in got else \
                D.product(dgq[:, k], _f64(WuT), form, Bdgq[:, k])
            p3, B3 = mul(d, Bd, q[:, k], None)
            p4 = ga * dq[:, k]
            g0 = 0.0 if dgf_in is None else _f64(dgf_in)[:, k]
            dgf[:, k] = o + p3 + p4 + g0
            Bdgf[:, k] = Bo + B3 + 4 * U * (np.abs(o) + Bo + np.abs(p3) + B3 + np.abs(p4) + np.abs(g0))
        out['gq'], out['dgq'], out['dgf'] = (gq, Bgq, _all(n)), (dgq, Bdgq, _all(n)), (dgf, Bdgf, _all(n))
    return out


def update_tan_fwd(da_mid, f, df, q, dq):
    da_mid, f, df, q, dq = (_f64(t) for t in (da_mid, f, df, q, dq))
    a = da_mid + (df * q + f * dq).sum(axis=1)
    mag = np.abs(da_mid) + (np.abs(df * q) + np.abs(f * dq)).sum(axis=1)
    return {'da_out': (a, 7 * U * mag, _all(f.shape[0]))}


def update_tan_bwd(ga, dga, f, df, q, dq, dgf_in=None):
    ga, dga, f, df, q, dq = (_f64(t) for t in (ga, dga, f, df, q, dq))
    n = f.shape[0]
    a, d = ga[:, None], dga[:, None]
    gq = a * f
    dgq = d * f + a * df
    g0 = 0.0 if dgf_in is None else _f64(dgf_in)
    dgf = d * q + a * dq + g0
    return {'gq': (gq, U * np.abs(gq), _all(n)), 'dgq': (dgq, 2 * U * (np.abs(d * f) + np.abs(a * df)), _all(n)),
            'dgf': (dgf, 3 * U * (np.abs(d * q) + np.abs(a * dq) + np.abs(g0)), _all(n))}


def head_seed_tan(e2, de2, w4, b4, scale, z, batch, g_energy, act='silu'):
    """the seed of the tangent reverse sweep (csrc/train.hip: head_seed_tan_kernel), c = g_energy[batch], sc = scale[z] (NULL: 1):
         dg_e2 = sc w4 (c act'(e2) + act''(e2) de2);   w4row = sc (c act(e2) + act'(e2) de2);
         scal  = (c eps + deps, c, sc c, 0),  eps = <act(e2), w4> + b4,  deps = <act'(e2) de2, w4>
    act, act', act'' are evaluations at an input (dense_ref.act_eval_err each); the two dot products have n = 128 terms."""
    e2, de2, w = _f64(e2), _f64(de2), _f64(w4)
    n = e2.shape[0]
    b4 = float(np.asarray(b4).reshape(-1)[0])
    c = _f64(g_energy)[np.asarray(batch)][:, None]
    sc = (np.ones(n) if scale is None else _f64(scale)[np.asarray(z)])[:, None]
    a, b, cc, err = D.act(act, e2), D.dact(act, e2), D.d2act(act, e2), D.act_eval_err(e2)

    def seeded(v0, v1, lead):
        inner = c * v0 + v1 * de2
        Bin = (np.abs(c) + np.abs(de2)) * err + 2 * U * (np.abs(c * v0) + np.abs(v1 * de2))
        out = lead * inner
        return out, np.abs(lead) * Bin + 2 * U * np.abs(out)
    dg, Bdg = seeded(b, cc, sc * w)
    wr, Bwr = seeded(a, b, sc)
    eps = a @ w + b4
    Beps = (F + 2) * U * ((np.abs(a) + err) @ np.abs(w)) + err @ np.abs(w) + U * np.abs(eps)
    deps = (b * de2) @ w
    Bdeps = (F + 3) * U * ((np.abs(b * de2) + np.abs(de2) * err) @ np.abs(w)) + (np.abs(de2) * err) @ np.abs(w)
    c1, s1 = c[:, 0], sc[:, 0]
    scal = np.stack([c1 * eps + deps, c1, s1 * c1, np.zeros(n)], axis=1)
    Bscal = np.stack([np.abs(c1) * Beps + Bdeps + 2 * U * (np.abs(c1 * eps) + np.abs(deps)), np.zeros(n), U * np.abs(s1 * c1), np.zeros(n)], axis=1)
    return {'dg_e2': (dg, Bdg, _all(n)), 'w4row': (wr, Bwr, _all(n)), 'scal': (scal, Bscal, _all(n))}


def direct_force_tail(d, f, scale, z):
    """out[i][k] = scale[z_i] <d_i, f_i,k> (csrc/node128.hip: direct_force_tail_kernel; d = the head's third linear, which
    nnhip_direct_force leaves in its scratch): a 128-term dot product and one product"""
    d, f = _f64(d), _f64(f)
    n = d.shape[0]
    sc = (np.ones(n) if scale is None else _f64(scale)[np.asarray(z)])[:, None]
    s = np.einsum('if,ikf->ik', d, f)
    out = s * sc
    return {'out': (out, np.abs(sc) * (F + 2) * U * np.einsum('if,ikf->ik', np.abs(d), np.abs(f)) + U * np.abs(out), _all(n))}


def direct_force_adj(g_out, d3, f, scale, z):
    """the adjoint of the tail (csrc/heads.hip: direct_force_adj_kernel): g_d3 = sc sum_k g_k f_k; seed_f_k = (g_k sc) d3;
    sc4 = (sum_k g_k <d3, f_k>, 0, 0, 0)"""
    g, d, f = _f64(g_out), _f64(d3), _f64(f)
    n = d.shape[0]
    sc = (np.ones(n) if scale is None else _f64(scale)[np.asarray(z)])[:, None]
    gs = g * sc
    g_d3 = np.einsum('ik,ikf->if', gs, f)
    Bg = 4 * U * np.einsum('ik,ikf->if', np.abs(gs), np.abs(f))
    seed = gs[:, :, None] * d[:, None, :]
    s = np.einsum('if,ikf->ik', d, f)
    raw = (g * s).sum(axis=1)
    Braw = (np.abs(g) * (F + 2) * U * np.einsum('if,ikf->ik', np.abs(d), np.abs(f))).sum(axis=1) + 4 * U * np.abs(g * s).sum(axis=1)
    sc4, Bsc4 = np.zeros((n, 4)), np.zeros((n, 4))
    sc4[:, 0], Bsc4[:, 0] = raw, Braw
    return {'g_d3': (g_d3, Bg, _all(n)), 'seed_f': (seed, 2 * U * np.abs(seed), _all(n)), 'sc4': (sc4, Bsc4, _all(n))}


def direct_force_inputs(n, seed=0):
    rng = rng_for('direct force', n, seed)
    t = node_inputs(n, 'plain', seed)
    return dict(atom_node=_r(rng, n, F), f=t['f'], z=t['z'], scale=t['scale'], w0=t['W0'], b0=t['b0'], w2=t['W2'], b2=t['b2'], w4=t['Wu'],
                b4=_r(rng, F, scale=0.3), g_out=_r(rng, n, 3), d=_r(rng, n, F))


def restate_direct_force_tail(t, scale=True, mut=None):
    d, f = _pair(t['d']), t['f']
    sc = t['scale'][t['z']] if scale else np.ones(len(t['z']), f32)
    cols = []
    for k in range(3):
        fk = _pair(f[:, k])
        cols.append(wave_sum32(fma32(d[..., 0], fk[..., 0], d[..., 1] * fk[..., 1])) * sc)
    return {'out': np.stack(cols, axis=1)}


def restate_direct_force_adj(t, scale=True, mut=None):
    d, f, g = _pair(t['d']), t['f'], t['g_out']
    sc = t['scale'][t['z']] if scale else np.ones(len(t['z']), f32)
    acc = np.zeros_like(t['d'])
    raw = np.zeros(len(sc), f32)
    seed = []
    for k in range(3):
        gs = (g[:, k] * sc)[:, None]
        fk = _pair(f[:, k])
        acc = fma32(f[:, k], gs, acc)
        raw = fma32(g[:, k], wave_sum32(fma32(d[..., 0], fk[..., 0], d[..., 1] * fk[..., 1])), raw)
        seed.append(t['d'] * gs)
    sc4 = np.zeros((len(sc), 4), f32)
    sc4[:, 0] = raw
    return {'g_d3': acc, 'seed_f': np.stack(seed, axis=1), 'sc4': sc4}


def head_seed_inputs(n, seed=0):
    rng = rng_for('head seed', n, seed)
    t = node_inputs(n, 'plain', seed)
    nb = 3
    return dict(e2=_r(rng, n, F), de2=_r(rng, n, F), w4=t['w4'], b4=t['b4'], scale=t['scale'], z=t['z'],
                batch=np.sort(rng.integers(0, nb, n)).astype(np.int64), g_energy=_r(rng, nb))


def restate_head_seed_tan(t, act='silu', scale=True, mut=None):
    h, dh, w = _pair(t['e2']), _pair(t['de2']), _pair(t['w4'][None])
    c = t['g_energy'][t['batch']][:, None, None]
    sc = (t['scale'][t['z']] if scale else np.ones(len(t['z']), f32))[:, None, None]
    a, b, cc = (act32(act, h, k) for k in range(3))
    dg = sc * w * fma32(c, b, cc * dh)
    wr = sc * fma32(c, a, b * dh)
    eps = wave_sum32(fma32(a[..., 0], w[..., 0], a[..., 1] * w[..., 1])) + t['b4'][0]
    deps = wave_sum32(fma32(b[..., 0] * dh[..., 0], w[..., 0], b[..., 1] * dh[..., 1] * w[..., 1]))
    c1, s1 = c[:, 0, 0], sc[:, 0, 0]
    return {'dg_e2': dg.reshape(-1, F), 'w4row': wr.reshape(-1, F), 'scal': np.stack([fma32(c1, eps, deps), c1, s1 * c1, np.zeros_like(c1)], axis=1)}


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------
def _mean(t, Bt=None, k=9):
    """(mean over the row, bound): k u mean|t| for the wave sum and the 1 / F product, + the mean of the terms' own bounds"""
    m = t.mean(axis=1, keepdims=True)
    B = k * U * np.abs(t).mean(axis=1, keepdims=True)
    return m, B if Bt is None else B + (1 + k * U) * Bt.mean(axis=1, keepdims=True)


def layer_norm_fwd(x, gamma, beta, eps=EPS):
    x, gamma, beta = _f64(x), _f64(gamma), _f64(beta)
    n = x.shape[0]
    mean, Bmean = _mean(x)
    dx = x - mean
    Bdx = U * (np.abs(x) + np.abs(mean)) + Bmean
    var, Bvar = _mean(dx * dx, 2 * np.abs(dx) * Bdx + Bdx * Bdx + U * dx * dx, k=10)
    rs = 1.0 / np.sqrt(var + eps)
    Brs = rs * ((Bvar + U * (var + eps)) / (2 * (var + eps)) + 3 * U)
    xh = dx * rs
    Bxh = rs * Bdx + np.abs(dx) * Brs + Bdx * Brs + U * np.abs(xh)
    y = xh * gamma + beta
    By = np.abs(gamma) * Bxh + U * np.abs(y)
    return {'y': (y, By, _all(n)), 'xhat': (xh, Bxh, _all(n)), 'rstd': (rs[:, 0], Brs[:, 0], _all(n))}


def _ln_adjoint_parts(g, w, xh):
    gp, Bgp = mul(g, None, w, None)
    m1, Bm1 = _mean(gp, Bgp)
    p, Bp = mul(gp, Bgp, xh, None)
    c, Bc = _mean(p, Bp, k=10)
    xc, Bxc = mul(xh, None, c, Bc)
    A = gp - m1 - xc
    BA = Bgp + Bm1 + Bxc + 2 * U * (np.abs(gp) + np.abs(m1) + np.abs(xc))
    return gp, Bgp, m1, c, Bc, A, BA


def layer_norm_bwd(g, gamma, xhat, rstd):
    """dE/dx = rstd (g' - mean(g') - xhat mean(g' xhat)), g' = g gamma"""
    g, w, xh, rs = _f64(g), _f64(gamma), _f64(xhat), _f64(rstd)[:, None]
    *_, A, BA = _ln_adjoint_parts(g, w, xh)
    out, B = mul(rs, None, A, BA)
    return {'g_x': (out, B, _all(g.shape[0]))}


def layer_norm_tan_fwd(dx, xhat, rstd, gamma):
    """s = mean(xhat dx); dxhat = r (dx - mean(dx) - xhat s); dr = -r^2 s; dy = gamma dxhat"""
    dx, xh, r, w = _f64(dx), _f64(xhat), _f64(rstd)[:, None], _f64(gamma)
    n = dx.shape[0]
    md, Bmd = _mean(dx)
    p, Bp = mul(xh, None, dx, None)
    sm, Bsm = _mean(p, Bp, k=10)
    xs, Bxs = mul(xh, None, sm, Bsm)
    inner = dx - md - xs
    Bin = Bmd + Bxs + 2 * U * (np.abs(dx) + np.abs(md) + np.abs(xs))
    dxh, Bdxh = mul(r, None, inner, Bin)
    dy, Bdy = mul(w, None, dxh, Bdxh)
    dr = -r * r * sm
    Bdr = r * r * Bsm + 2 * U * np.abs(dr)
    return {'dy': (dy, Bdy, _all(n)), 'dxhat': (dxh, Bdxh, _all(n)), 'drstd': (dr[:, 0], Bdr[:, 0], _all(n))}


def layer_norm_tan_bwd(gy, dgy, xhat, rstd, dxhat, drstd, gamma):
    """dA = dg' - mean(dg') - dxhat c - xhat mean(dg' xhat + g' dxhat); dg_x = dr A + r dA; row_w = dg_y xhat + g_y dxhat; row_b = dg_y"""
    g, dg, xh, dxh, w = (_f64(t) for t in (gy, dgy, xhat, dxhat, gamma))
    r, dr = _f64(rstd)[:, None], _f64(drstd)[:, None]
    n = g.shape[0]
    gp, Bgp, m1, c, Bc, A, BA = _ln_adjoint_parts(g, w, xh)
    dgp, Bdgp = mul(dg, None, w, None)
    dm1, Bdm1 = _mean(dgp, Bdgp)
    p1, B1 = mul(dgp, Bdgp, xh, None)
    p2, B2 = mul(gp, Bgp, dxh, None)
    dc, Bdc = _mean(p1 + p2, B1 + B2 + U * (np.abs(p1) + np.abs(p2)), k=10)
    t1, Bt1 = mul(dxh, None, c, Bc)
    t2, Bt2 = mul(xh, None, dc, Bdc)
    dA = dgp - dm1 - t1 - t2
    BdA = Bdgp + Bdm1 + Bt1 + Bt2 + 3 * U * (np.abs(dgp) + np.abs(dm1) + np.abs(t1) + np.abs(t2))
    o1, Bo1 = mul(dr, None, A, BA)
    o2, Bo2 = mul(r, None, dA, BdA)
    out = o1 + o2
    rw = dg * xh + g * dxh
    return {'dg_x': (out, Bo1 + Bo2 + U * (np.abs(o1) + np.abs(o2)), _all(n)),
            'row_w': (rw, 2 * U * (np.abs(dg * xh) + np.abs(g * dxh)), _all(n)), 'row_b': (dg, np.zeros_like(dg), _all(n))}


# ---------------------------------------------------------------------------------------------------------------------------
# the cases: independent seeded random fp32 arrays, shared by the CPU tests of the bounds and the kernel tests
# ---------------------------------------------------------------------------------------------------------------------------
SPECIES = np.array([0, 1, 6, 7, 8, 17, 35, 118])
EDGES = ('plain', 'zero row', 'zero f', 'decades', 'big row', 'big weight')
LN_EDGES = ('plain', 'constant row', 'offset row', 'gamma zeros', 'small row')


def _r(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(f32)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def node_inputs(n, edge='plain', seed=0):
    """every array a node stage may take, for n rows.  The matrices are stored as the interface takes them: Wu, W0, W2 and the
    transposes WuT, W0T, W2T.
      zero row    row 2 (or the last) of every row input is zero;       zero f   f is zero everywhere
      decades     every row input spans 12 decades inside a row (the row scale of the split resolves the largest only)
      big row     row 7 of the leading input of a stage is 2^40 times its neighbours (a scale leaking across rows)
      big weight  one entry of every matrix is 2^20 above the rest"""
    rng = rng_for('node', n, edge, seed)
    s = 1.0 / np.sqrt(F)
    t = {k: _r(rng, n, 3, F, scale=0.5) for k in ('f', 'df', 'G_f', 'dq', 'dgf_in')}
    t.update({k: _r(rng, n, F) for k in ('a_mid', 'g_top', 'h_top', 'g_a', 'g_a_in', 'da_mid', 'hn', 't2_top', 'hd_top', 'dga', 'ga')})
    t.update({k: _r(rng, F, F, scale=s) for k in ('Wu', 'W0', 'W2')})
    t.update({k: _r(rng, F, scale=0.3) for k in ('b0', 'b2', 'w4')})
    t['b4'] = _r(rng, 1)
    t['scale'] = (1.0 + 0.5 * rng.random(N_ELEMENTS)).astype(f32)
    t['shift'] = _r(rng, N_ELEMENTS, scale=3.0)
    t['z'] = np.concatenate([SPECIES, rng.integers(0, N_ELEMENTS, max(n, len(SPECIES)))])[:n].astype(np.int64) if n else np.zeros(0, np.int64)
    rows = [k for k, v in t.items() if v.ndim >= 2 and v.shape[0] == n and k not in ('Wu', 'W0', 'W2')]
    lead = ('f', 'g_top', 'df')
    if n and edge == 'zero row':
        for k in rows:
            t[k][min(2, n - 1)] = 0
    elif edge == 'zero f':
        t['f'][:] = 0
    elif edge == 'decades':
        for k in rows:
            t[k] *= (10.0 ** rng.uniform(-12, 0, t[k].shape)).astype(f32)
    elif n and edge == 'big row':
        for k in lead:
            t[k][min(7, n - 1)] *= f32(2.0 ** 40)
    elif edge == 'big weight':
        for k in ('Wu', 'W0', 'W2'):
            t[k][int(rng.integers(F)), int(rng.integers(F))] *= f32(2.0 ** 20)
    for k in ('Wu', 'W0', 'W2'):
        t[k + 'T'] = np.ascontiguousarray(t[k].T)
    t['q'] = np.stack([(t['f'][:, k].astype(np.float64) @ t['Wu'].astype(np.float64).T) for k in range(3)], axis=1).astype(f32) \
        if n else np.zeros((0, 3, F), f32)
    return t


def ln_inputs(n, edge='plain', seed=0):
    """  constant row  variance 0;   offset row  mean 1e3, spread 1e-2;   gamma zeros;   small row  magnitude 1e-3"""
    rng = rng_for('ln', n, edge, seed)
    t = {k: _r(rng, n, F) for k in ('x', 'g', 'dx', 'gy', 'dgy')}
    t['gamma'] = (1.0 + 0.3 * rng.standard_normal(F)).astype(f32)
    t['beta'] = _r(rng, F, scale=0.3)
    r = min(1, n - 1)
    if n and edge == 'constant row':
        t['x'][r] = f32(0.75)
    elif n and edge == 'offset row':
        t['x'][r] = (1e3 + 1e-2 * rng.standard_normal(F)).astype(f32)
    elif edge == 'gamma zeros':
        t['gamma'][::5] = 0
    elif n and edge == 'small row':
        t['x'][r] *= f32(1e-3)
    # the adjoint / tangent kernels read what the forward kernel stored: the fp32 roundings of the float64 statement
    fw = layer_norm_fwd(t['x'], t['gamma'], t['beta'])
    t['xhat'], t['rstd'] = fw['xhat'][0].astype(f32), fw['rstd'][0].astype(f32)
    tf = layer_norm_tan_fwd(t['dx'], t['xhat'], t['rstd'], t['gamma'])
    t['dxhat'], t['drstd'] = tf['dxhat'][0].astype(f32), tf['drstd'][0].astype(f32)
    return t


# Variants of each stage: name -> keyword arguments of the statement (and of the launch); every one is a case of its own.
FWD_VARIANTS = {f'q={int(sq)} W0={int(w0)}': dict(store_q=sq, mlp=w0) for sq in (True, False) for w0 in (True, False)}
BWD_VARIANTS = {
    'mlp only': dict(mlp=True, upd=False), 'update only': dict(mlp=False, upd=True), 'both': dict(mlp=True, upd=True),
    'both acc': dict(mlp=True, upd=True, acc=1), 'mlp acc': dict(mlp=True, upd=False, acc=1),
    'both G_f': dict(mlp=True, upd=True, G_f=True), 'update G_f': dict(mlp=False, upd=True, G_f=True),
}
BWD_SPLIT_VARIANTS = {       # the members of the split-f16 kernel only
    'both T': dict(mlp=True, upd=True, T=True), 'both acc g_a_in=g_a': dict(mlp=True, upd=True, acc=1, g_a_in='same'),
    'both acc g_a_in': dict(mlp=True, upd=True, acc=1, g_a_in='other', T=True, G_f=True),
    'both recompute q': dict(mlp=True, upd=True, G_f=True, recompute=True), 'update recompute q': dict(mlp=False, upd=True, recompute=True),
}
TURN_VARIANTS = {f'scale={int(a)} shift={int(b)}': dict(scale=a, shift=b) for a in (True, False) for b in (True, False)}
TAN_BWD_VARIANTS = {
    'A only': dict(A=True, B=False), 'B only': dict(A=False, B=True), 'both': dict(A=True, B=True),
    'both no t2': dict(A=True, B=True, t2=False), 'both acc': dict(A=True, B=True, acc=1), 'A acc no t2': dict(A=True, B=False, acc=1, t2=False),
    'both dgf_in': dict(A=True, B=True, dgf_in=True),
}


def ref_node_fwd(t, act, form, store_q=True, mlp=True, got=None):
    w = dict(W0=t['W0'], b0=t['b0'], W2=t['W2'], b2=t['b2']) if mlp else {}
    return node_fwd(t['f'], t['a_mid'], t['Wu'], act=act, form=form, store_q=store_q, got=got, **w)


def ref_node_bwd(t, act, form, mlp=True, upd=True, acc=0, G_f=False, T=False, g_a_in=None, recompute=False, q=None, got=None):
    kw = dict(act=act, form=form, acc_ga=acc, want_T=T, got=got)
    if mlp:
        kw.update(g_top=t['g_top'], h_top=t['h_top'], W2T=t['W2T'], W0T=t['W0T'])
    if upd:
        kw.update(f=t['f'], q=None if recompute else (t['q'] if q is None else q), G_f=t['G_f'] if G_f else None, WuT=t['WuT'], Wu=t['Wu'])
    if g_a_in == 'other':
        kw['g_a_in'] = t['g_a_in']
    return node_bwd(t['g_a'], **kw)


def ref_node_turn(t, scale=True, shift=True, got=None):
    return node_turn(t['f'], t['a_mid'], t['Wu'], t['W0'], t['b0'], t['W2'], t['b2'], t['w4'], t['b4'], t['scale'] if scale else None,
                     t['shift'] if shift else None, t['z'], t['W2T'], t['W0T'], t['WuT'], got=got)


def ref_node_tan_fwd(t, got=None):
    return node_tan_fwd(t['df'], t['f'], t['q'], t['da_mid'], t['hn'], t['Wu'], t['W0'], t['W2'], got=got)


def ref_node_tan_bwd(t, A=True, B=True, t2=True, acc=0, dgf_in=False, got=None):
    kw = dict(acc_dga=acc, got=got)
    if A:
        kw.update(g_top=t['g_top'], h_top=t['h_top'], W2T=t['W2T'], W0T=t['W0T'])
        if t2:
            kw.update(t2_top=t['t2_top'], hd_top=t['hd_top'])
    if B:
        kw.update(ga=t['ga'], f=t['f'], df=t['df'], q=t['q'], dq=t['dq'], WuT=t['WuT'], dgf_in=t['dgf_in'] if dgf_in else None)
    return node_tan_bwd(t['dga'], **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the kernels' own order of operations (what check 3 of tests/test_node_ref_host.py holds to the bounds).
# `mut`: the name of a deliberately wrong kernel (MUTATIONS), None for the right one.
# ---------------------------------------------------------------------------------------------------------------------------
def pow2_scale(m):
    """csrc/mlp128s.hip:49-55: S = 2^(14 - floor(log2 m)) and 1 / S; (1, 1) below an exponent field of 40 and for non-finite m"""
    e = (np.asarray(m, f32).view(np.uint32) >> 23) & 0xff
    ok = (e >= 40) & (e < 255)
    ee = np.where(ok, e, 141).astype(np.int64)
    return np.ldexp(1.0, 141 - ee).astype(f32), np.ldexp(1.0, ee - 141).astype(f32)


def split16(v, S):
    """hi = f16(v S), lo = f16(v S - hi)"""
    with np.errstate(over='ignore', invalid='ignore'):
        s = (np.asarray(v, f32) * S).astype(f32)
        hi = s.astype(np.float16)
        lo = (s - hi.astype(f32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def gemm_split(X, W):
    """X W^T as the image kernels form it (csrc/node128s.hip: tile_commit, tile_gemm_s; weight_image_kernel): row scales of X, one
    scale of W, hi / lo f16 pieces, per 16 k-values the three partial products hi hi, hi lo, lo hi accumulated in fp32"""
    X, W = np.asarray(X, f32), np.asarray(W, f32)
    Sx, ix = pow2_scale(np.abs(X).max(axis=1, keepdims=True))
    Sw, iw = pow2_scale(np.abs(W).max())
    xh, xl = split16(X, Sx)
    wh, wl = split16(W, Sw)
    acc = np.zeros((X.shape[0], W.shape[0]), f32)
    with np.errstate(over='ignore', invalid='ignore'):
        for T in range(F // 16):
            k = slice(16 * T, 16 * T + 16)
            acc = (acc + xh[:, k] @ wh[:, k].T).astype(f32)
            acc = (acc + xl[:, k] @ wh[:, k].T).astype(f32)
            acc = (acc + xh[:, k] @ wl[:, k].T).astype(f32)
        return (acc * (ix * iw).astype(f32)).astype(f32)


def gemm_fp32(X, W):
    """X W^T on v_mfma_f32_32x32x2_f32: two k-values per step, fp32 accumulation"""
    X, W = np.asarray(X, f32).astype(np.float64), np.asarray(W, f32).astype(np.float64)
    acc = np.zeros((X.shape[0], W.shape[0]), f32)
    with np.errstate(over='ignore', invalid='ignore'):
        for k in range(0, F, 2):
            acc = (acc + X[:, k:k + 2] @ W[:, k:k + 2].T).astype(f32)
    return acc


def gemm(form):
    return gemm_split if form == SPLIT else gemm_fp32


def act32(name, x, order=0):
    """fp32 evaluation of act (order 0), act' (1), act'' (2): the float64 function rounded once, except SiLU, which the split
    kernels evaluate as x s, s (1 + x (1 - s)), s (1 - s) (2 + x (1 - 2 s)) with s = 1 / (1 + exp(-x)) in fp32"""
    x = np.asarray(x, f32)
    if name != 'silu':
        return (D.act, D.dact, D.d2act)[order](name, x).astype(f32)
    one = f32(1)
    with np.errstate(over='ignore', invalid='ignore'):
        s = (one / (one + np.exp(-x).astype(f32))).astype(f32)
        if order == 0:
            return x * s
        if order == 1:
            return s * (one + x * (one - s))
        return s * (one - s) * (f32(2) + x * (one - f32(2) * s))


def fma32(a, b, c):
    with np.errstate(over='ignore', invalid='ignore'):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def wave_sum32(v):
    """lane l holds the two features 2 l, 2 l + 1 already combined into v[..., l]; 64 lanes, a 6-level butterfly"""
    return tree_sum32(v)


def _pair(x):
    return np.asarray(x, f32).reshape(x.shape[0], 64, 2)


def _drop_last(out, mut, names):
    """the last row of a tile not written"""
    if mut == 'last row':
        for k in names:
            out[k] = out[k].copy()
            out[k][-1] = np.nan
    return out


def restate_node_fwd(t, act, form, store_q=True, mlp=True, mut=None):
    mm = gemm(form)
    f, Wu = t['f'], (t['WuT'] if mut == 'Wu transposed' else t['Wu'])
    q = np.stack([mm(f[:, k], Wu) for k in range(3)], axis=1)
    upd = np.zeros_like(t['a_mid'])
    for k in range(3):
        upd = fma32(f[:, k], q[:, (k + 1) % 3 if mut == 'wrong q' else k], upd)
    a = t['a_mid'] + upd
    out = {'a_out': a}
    if store_q:
        out['q'] = q
    if mlp:
        hn = mm(a, t['W0']) + t['b0']
        out['hn'] = hn
        out['m'] = mm(act32(act, hn), t['W2']) + t['b2']
    return _drop_last(out, mut, list(out))


def restate_node_bwd(t, act, form, mlp=True, upd=True, acc=0, G_f=False, T=False, g_a_in=None, recompute=False, q=None, mut=None):
    mm = gemm(form)
    out = {}
    ga = t['g_a']
    if mlp:
        tt = mm(t['g_top'], t['W2T'])
        if T:
            out['T'] = tt
        g = tt * act32(act, t['g_top'] if mut == "act' at the wrong place" else t['h_top'], 1)
        ga = mm(g, t['W0T'])
        if acc and mut != 'acc_ga ignored':
            ga = ga + (t['g_a_in'] if g_a_in == 'other' else t['g_a'])
    out['g_a'] = ga
    if upd:
        f = t['f']
        qq = [mm(f[:, k], t['Wu']) for k in range(3)] if recompute else [(t['q'] if q is None else q)[:, k] for k in range(3)]
        gf = []
        for k in range(3):
            o = mm(f[:, k] * ga, t['Wu'] if mut == 'Wu transposed' else t['WuT'])
            o = fma32(ga, qq[(k + 1) % 3 if mut == 'wrong q' else k], o)
            if G_f and mut != 'G_f dropped':
                o = o + t['G_f'][:, k]
            gf.append(o)
        out['gf'] = np.stack(gf, axis=1)
    return _drop_last(out, mut, [k for k in out if k != 'g_a' or mlp])


def restate_head_tail(e2, t, scale, shift, mut=None):
    a = _pair(act32('silu', e2))
    w = _pair(t['w4'][None])
    s = wave_sum32(fma32(a[..., 0], w[..., 0], a[..., 1] * w[..., 1]))
    sc = t['scale'][t['z']] if scale else np.ones(len(t['z']), f32)
    sh = t['shift'][t['z']] if shift and mut != 'shift missing' else np.zeros(len(t['z']), f32)
    return fma32(s + t['b4'][0], sc, sh), (sc[:, None] * t['w4']) * act32('silu', e2, 1)


def restate_node_turn(t, scale=True, shift=True, mut=None):
    fw = restate_node_fwd(t, 'silu', SPLIT, store_q=True, mlp=True, mut=mut if mut in ('wrong q',) else None)
    ae, ge = restate_head_tail(fw['m'], t, scale, shift, mut)
    t2 = dict(t, g_top=ge, h_top=fw['hn'], q=fw['q'])
    bw = restate_node_bwd(t2, 'silu', SPLIT, mut=mut if mut in ('Wu transposed', "act' at the wrong place") else None)
    out = _drop_last({'a_out': fw['a_out'], 'atom_energy': ae, 'g_a': bw['g_a'], 'gf': bw['gf']}, mut, ['a_out', 'atom_energy', 'g_a', 'gf'])
    out['_stored'] = {'a_out': fw['a_out'], 'e1': fw['hn'], 'e2': fw['m'], 'g_e2': ge, 'g_a': bw['g_a']}   # what the composition stores
    return out


def restate_node_tan_fwd(t, mut=None):
    dq = np.stack([gemm_split(t['df'][:, k], t['Wu']) for k in range(3)], axis=1)
    upd = np.zeros_like(t['da_mid'])
    for k in range(3):
        upd = fma32(t['df'][:, k], t['q'][:, k], fma32(t['f'][:, k], dq[:, k], upd))
    a = t['da_mid'] + upd
    T = gemm_split(a, t['W0'])
    Y = gemm_split(T * act32('silu', t['hn'], 1), t['W2'])
    return _drop_last({'dq': dq, 'da_out': a, 'T': T, 'Y': Y}, mut, ['dq', 'da_out', 'T', 'Y'])


def restate_node_tan_bwd(t, A=True, B=True, t2=True, acc=0, dgf_in=False, mut=None):
    out = {}
    d = t['dga']
    if A:
        g = gemm_split(t['g_top'], t['W2T'])
        if t2 and mut != "act'' dropped":
            g = fma32(g, act32('silu', t['h_top'], 1), t['t2_top'] * act32('silu', t['h_top'], 2) * t['hd_top'])
        else:
            g = g * act32('silu', t['h_top'], 1)
        out['G'] = g
        d = gemm_split(g, t['W0T'])
        if acc:
            d = d + t['dga']
    out['dga'] = d
    if B:
        ga = t['ga']
        gq, dgq, dgf = [], [], []
        for k in range(3):
            gq.append(ga * t['f'][:, k])
            v = fma32(d, t['f'][:, k], ga * t['df'][:, k])
            dgq.append(v)
            o = gemm_split(v, t['WuT']) + fma32(d, t['q'][:, k], ga * t['dq'][:, k])
            if dgf_in:
                o = o + t['dgf_in'][:, k]
            dgf.append(o)
        out.update(gq=np.stack(gq, 1), dgq=np.stack(dgq, 1), dgf=np.stack(dgf, 1))
    return _drop_last(out, mut, [k for k in out if k != 'dga' or A])


def restate_update_tan_fwd(t, mut=None):
    acc = t['da_mid']
    for k in range(3):
        acc = fma32(t['df'][:, k], t['q'][:, k], acc)
        acc = fma32(t['f'][:, k], t['dq'][:, k], acc)
    return {'da_out': acc}


def restate_update_tan_bwd(t, dgf_in=False, mut=None):
    a, d = t['ga'][:, None], t['dga'][:, None]
    o = fma32(d, t['q'], a * t['dq'])
    return {'gq': a * t['f'], 'dgq': fma32(d, t['f'], a * t['df']), 'dgf': o + t['dgf_in'] if dgf_in else o}


def restate_layer_norm_fwd(t, mut=None):
    x = _pair(t['x'])
    inv = f32(1.0 / F)
    mean = (wave_sum32(x[..., 0] + x[..., 1]) * inv)[:, None]
    dx, dy = x[..., 0] - mean, x[..., 1] - mean
    var = wave_sum32(fma32(dx, dx, dy * dy)) * inv
    with np.errstate(divide='ignore', invalid='ignore'):
        rs = (f32(1) / np.sqrt(var + (f32(0) if mut == 'eps missing' else f32(EPS)), dtype=f32)).astype(f32)
        xh = np.stack([dx * rs[:, None], dy * rs[:, None]], axis=-1).reshape(-1, F)
    return _drop_last({'y': fma32(xh, t['gamma'], t['beta']), 'xhat': xh, 'rstd': rs}, mut, ['y', 'xhat', 'rstd'])


def restate_layer_norm_bwd(t, mut=None):
    gp = _pair(t['g'] * t['gamma'])
    xh = _pair(t['xhat'])
    inv = f32(1.0 / F)
    m1 = (wave_sum32(gp[..., 0] + gp[..., 1]) * inv)[:, None, None]
    if mut == "mean(g') dropped":
        m1 = m1 * f32(0)
    m2 = (wave_sum32(fma32(gp[..., 0], xh[..., 0], gp[..., 1] * xh[..., 1])) * inv)[:, None, None]
    return {'g_x': (t['rstd'][:, None, None] * (gp - m1 - xh * m2)).reshape(-1, F)}


def restate_layer_norm_tan_fwd(t, mut=None):
    dx, xh = _pair(t['dx']), _pair(t['xhat'])
    inv = f32(1.0 / F)
    r = t['rstd']
    md = (wave_sum32(dx[..., 0] + dx[..., 1]) * inv)
    sm = (wave_sum32(fma32(xh[..., 0], dx[..., 0], xh[..., 1] * dx[..., 1])) * inv)
    dxh = (r[:, None, None] * (dx - md[:, None, None] - xh * sm[:, None, None])).reshape(-1, F)
    return {'dy': t['gamma'] * dxh, 'dxhat': dxh, 'drstd': -r * r * sm}


def restate_layer_norm_tan_bwd(t, mut=None):
    w = _pair(t['gamma'][None])
    g, dg, xh, dxh = (_pair(t[k]) for k in ('gy', 'dgy', 'xhat', 'dxhat'))
    r, dr = t['rstd'][:, None, None], t['drstd'][:, None, None]
    inv = f32(1.0 / F)
    gp, dgp = g * w, dg * w
    ws = lambda v: (wave_sum32(v) * inv)[:, None, None]  # noqa: E731
    m1 = ws(gp[..., 0] + gp[..., 1])
    c = ws(fma32(gp[..., 0], xh[..., 0], gp[..., 1] * xh[..., 1]))
    dm1 = ws(dgp[..., 0] + dgp[..., 1])
    dc = ws(fma32(dgp[..., 0], xh[..., 0], dgp[..., 1] * xh[..., 1]) + fma32(gp[..., 0], dxh[..., 0], gp[..., 1] * dxh[..., 1]))
    A = gp - m1 - xh * c
    dA = dgp - dm1 - dxh * c - xh * dc
    return {'dg_x': fma32(dr, A, r * dA).reshape(-1, F), 'row_w': fma32(dg, xh, g * dxh).reshape(-1, F), 'row_b': t['dgy']}


def ref_ln(stage, t):
    if stage == 'layer_norm_fwd':
        return layer_norm_fwd(t['x'], t['gamma'], t['beta'])
    if stage == 'layer_norm_bwd':
        return layer_norm_bwd(t['g'], t['gamma'], t['xhat'], t['rstd'])
    if stage == 'layer_norm_tan_fwd':
        return layer_norm_tan_fwd(t['dx'], t['xhat'], t['rstd'], t['gamma'])
    return layer_norm_tan_bwd(t['gy'], t['dgy'], t['xhat'], t['rstd'], t['dxhat'], t['drstd'], t['gamma'])


LN_STAGES = {'layer_norm_fwd': restate_layer_norm_fwd, 'layer_norm_bwd': restate_layer_norm_bwd,
             'layer_norm_tan_fwd': restate_layer_norm_tan_fwd, 'layer_norm_tan_bwd': restate_layer_norm_tan_bwd}


def node_cases():
    """(stage, form, activation, rows, data edge, variant name, variant) of every node-stage case of the kernel tests"""
    out = []
    for n in NODE_ROWS:
        for form in (SPLIT, FP32):
            for name, v in FWD_VARIANTS.items():
                out.append(('node_fwd', form, 'silu', n, 'plain', name, v))
            for name, v in {**BWD_VARIANTS, **(BWD_SPLIT_VARIANTS if form == SPLIT else {})}.items():
                out.append(('node_bwd', form, 'silu', n, 'plain', name, v))
        for name, v in TURN_VARIANTS.items():
            out.append(('node_turn', SPLIT, 'silu', n, 'plain', name, v))
        out.append(('node_tan_fwd', SPLIT, 'silu', n, 'plain', '', {}))
        for name, v in TAN_BWD_VARIANTS.items():
            out.append(('node_tan_bwd', SPLIT, 'silu', n, 'plain', name, v))
    for act in D.ACTIVATIONS[1:]:
        out.append(('node_fwd', FP32, act, 33, 'plain', 'q=1 W0=1', FWD_VARIANTS['q=1 W0=1']))
        out.append(('node_bwd', FP32, act, 33, 'plain', 'both G_f', BWD_VARIANTS['both G_f']))
    for edge in EDGES[1:]:
        for form in (SPLIT, FP32):
            out.append(('node_fwd', form, 'silu', 33, edge, 'q=1 W0=1', FWD_VARIANTS['q=1 W0=1']))
            out.append(('node_bwd', form, 'silu', 33, edge, 'both G_f', BWD_VARIANTS['both G_f']))
        out.append(('node_bwd', SPLIT, 'silu', 33, edge, 'both recompute q', BWD_SPLIT_VARIANTS['both recompute q']))
        out.append(('node_turn', SPLIT, 'silu', 33, edge, 'scale=1 shift=1', TURN_VARIANTS['scale=1 shift=1']))
        out.append(('node_tan_fwd', SPLIT, 'silu', 33, edge, '', {}))
        out.append(('node_tan_bwd', SPLIT, 'silu', 33, edge, 'both', TAN_BWD_VARIANTS['both']))
    return out


def node_ref(stage, form, act, t, v, got=None):
    if stage == 'node_fwd':
        return ref_node_fwd(t, act, form, got=got, **v)
    if stage == 'node_bwd':
        return ref_node_bwd(t, act, form, got=got, **v)
    if stage == 'node_turn':
        return ref_node_turn(t, got=got, **v)
    if stage == 'node_tan_fwd':
        return ref_node_tan_fwd(t, got=got)
    return ref_node_tan_bwd(t, got=got, **v)


def node_restate(stage, form, act, t, v, mut=None):
    if stage == 'node_fwd':
        return restate_node_fwd(t, act, form, mut=mut, **v)
    if stage == 'node_bwd':
        return restate_node_bwd(t, act, form, mut=mut, **v)
    if stage == 'node_turn':
        return restate_node_turn(t, mut=mut, **v)
    if stage == 'node_tan_fwd':
        return restate_node_tan_fwd(t, mut=mut)
    return restate_node_tan_bwd(t, mut=mut, **v)


def judge(stage, form, act, t, v, got, stored=None):
    """{output: worst |got - value| / bound}: each output against the CHAINED statement and against the statement that takes the
    stored intermediates in front of it as exact operands (`stored`: those of the three-launch composition for node_turn, the
    kernel's own outputs otherwise), the larger ratio of the two"""
    stored = {k: x for k, x in (got if stored is None else stored).items() if not k.startswith('_')}
    out = {}
    for ref in (node_ref(stage, form, act, t, v), node_ref(stage, form, act, t, v, got=stored)):
        for k, g in got.items():
            if not k.startswith('_'):
                out[k] = max(out.get(k, 0.0), worst_ratio(g, ref[k]))
    return out


def worst_ratio(got, ref):
    """largest |got - value| / bound over the defined entries of one output (inf where the bound is zero and the error is not)"""
    val, B, defined = ref
    d = np.broadcast_to(np.asarray(defined).reshape((-1,) + (1,) * (val.ndim - 1)), val.shape)
    if not d.any():
        return 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        err = np.abs(np.asarray(got, np.float64)[d] - val[d])
    err = np.where(np.isfinite(err), err, np.inf)
    Bd = B[d]
    return float(np.where(Bd > 0, err / np.where(Bd > 0, Bd, 1.0), np.where(err > 0, np.inf, 0.0)).max())
