"""The float64 statements of tests/edge_ref.py checked on the CPU: what tests/test_hip_edge_stages.py compares the HIP kernels with
must itself be right, its bounds must hold for the kernels' own order of operations in fp32, and they must still tell a wrong
kernel from a right one.  No GPU.

  * derivative structure: every *_bwd statement is the vector-Jacobian product of its *_fwd statement and every *_tan_* statement the
    Jacobian-vector product of the value statement, by torch float64 autograd, with the table replaced by a smooth filter that
    has the same value and derivative at the edge (eps_e(x) = eps_e + d eps_e (x - x_e));
  * chained over the layers of one small molecule the statements reproduce tests/trace.py and the tangent sweeps of
    tests/tangent_ref.py (the exact filter in place of the table);
  * the kernels' summation order restated in fp32 numpy (two edges per step, half-wave fold, the waves of a split row added in
    wave order, the molecule-resident kernels' single range) stays inside the bound on every graph of the kernel tests;
  * each of nine wrong kernels (MUTATIONS, mutated_view) leaves the bound by more than 10 x somewhere in every output it changes;
  * the graph builder's conventions; the XCD tile map is a bijection.
"""
import numpy as np
import pytest
import torch

from tests import dense_ref as D
from tests import edge_ref as R
from tests.test_dense_ref_host import TORCH_ACT

F = R.F


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max(initial=0.0) <= tol * max(1.0, np.abs(b).max(initial=0.0)), np.abs(a - b).max()


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


@pytest.fixture(scope='module')
def table():
    W, freq = R.filter_weights()
    return R.host_filter_table(W, freq)


@pytest.fixture(scope='module')
def graphs():
    return {name: make() for name, make in R.GRAPHS.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# graph builder, tile map
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(R.GRAPHS) + ['one atom', 'no atoms'])
def test_graph_builder_conventions(name):
    g = R.graph_trivial(1 if name == 'one atom' else 0) if name not in R.GRAPHS else R.GRAPHS[name]()
    N, E = g.N, g.E
    assert g.row_ptr[0] == 0 and g.row_ptr[-1] == E and E == 2 * g.P and g.mol_ptr[-1] == N
    e = np.arange(E)
    assert (g.rev[g.rev] == e).all() and (g.rev != e).all()
    assert (g.i[g.rev] == g.j).all() and (g.j[g.rev] == g.i).all() and (g.col == g.j).all()
    assert (g.pid == g.pid[g.rev]).all() and sorted(g.pid[g.own].tolist()) == list(range(g.P))
    upper = np.zeros(N, np.int64)
    np.add.at(upper, g.i[g.own], 1)
    assert (g.pair_ptr == np.concatenate([[0], np.cumsum(upper)])).all()
    for i in range(N):
        beg, end = g.row_ptr[i], g.row_ptr[i + 1]
        assert (np.diff(g.col[beg:end]) > 0).all()                                  # ascending, no pair twice
        mid = end - upper[i]
        assert (g.col[beg:mid] < i).all() and (g.col[mid:end] > i).all()            # the upper edges are the last ones ...
        assert (g.pid[mid:end] == g.pair_ptr[i] + np.arange(end - mid)).all()       # ... and own a contiguous run of pair rows
    assert (g.geo[:, :3] == -g.geo[g.rev, :3]).all() and (g.geo[:, 3] == g.geo[g.rev, 3]).all()
    assert np.allclose(np.linalg.norm(g.geo[:, :3].astype(np.float64), axis=1), 1.0, atol=1e-6) or E == 0
    assert (g.xg == g.xg[g.rev]).all() and (g.masked == g.masked[g.rev]).all()
    assert ((g.xg[:, 0] == R.FT_ZERO_ROW) == g.masked).all() and (g.xg[g.masked, 1] == 0).all()
    frac = np.ascontiguousarray(g.xg_live[:, 1]).view(np.float32)
    x = (g.xg_live[:, 0] + frac.astype(np.float64)) / R.FT_G
    assert np.allclose(x, g.geo[:, 3].astype(np.float64) / g.cutoff, atol=1e-7) and ((frac >= 0) & (frac < 1)).all()
    mol = np.searchsorted(g.mol_ptr, np.arange(N), side='right') - 1
    assert (mol[g.i] == mol[g.j]).all()


def test_the_graphs_have_the_shapes_the_kernel_tests_rely_on(graphs):
    g = graphs['degrees']
    deg = R.degrees(g)
    assert g.N == 37 and set(R.DEGREES_WANTED) <= set(deg.tolist()) and deg[36] == 0
    assert [-(-37 // (R.EDGE_ROWS // w)) for w in (1, 2, 4)] == [10, 19, 37]
    upper = np.diff(g.pair_ptr)
    assert ((upper == deg) & (deg > 0)).any() and ((upper == 0) & (deg > 0)).any()     # all above / all below
    g = graphs['wide row']
    deg = R.degrees(g)
    assert deg[67] == 130 and deg[20] == 65 and 64 < (g.col[g.row_ptr[67]:g.row_ptr[68]] < 67).sum() < 128
    g = graphs['molecules']
    sizes = np.diff(g.mol_ptr)
    assert tuple(sizes) == R.MOLECULE_SIZES and 8 * g.B <= g.N <= R.MOL_STAGE_MAX * g.B
    per_mol = np.diff(g.row_ptr[g.mol_ptr])
    assert per_mol[4] == 24 * 23 and per_mol[0] == 0 and (per_mol[sizes <= R.MOL_STAGE_MAX] <= 24 * 23).all()
    g = graphs['masked']
    deg, beg, end = R.degrees(g), g.row_ptr[:-1], g.row_ptr[1:]
    n_masked = np.add.reduceat(np.append(g.masked, False).astype(int), beg)[:g.N] * (deg > 0)
    assert 0.15 < g.masked.mean() < 0.4 and ((n_masked == deg) & (deg > 0)).any()
    assert any(deg[i] % 2 == 1 and g.masked[end[i] - 1] and not g.masked[beg[i]:end[i]].all() for i in range(g.N))


@pytest.mark.parametrize('n', (0, 1))
def test_statements_accept_graphs_without_edges(n, table):
    g = R.graph_trivial(n)
    d = R.stage_inputs(g)
    out = _statements(g, R.TableFilter(table, g.xg), d)
    _close(out['message_fwd.a_mid'][0], d['a_in'])
    _close(out['force_message_fwd.f_out'][0], d['f_in'])
    _close(out['force_message_bwd.g_fin'][0], d['gf'])
    assert not out['edge_embed_bwd.forces'][0].any() and not out['message_bwd.g_m'][0].any()
    assert out['message_fwd.msg'][0].shape == (0, F) and out['edge_embed_bwd.virial'][0].shape == (n, 3, 3)
    h = R.head_out(d['e2'], d['w4'], d['b4'], d['scale'], d['shift'], d['z'], g.mol_ptr)
    assert h['energy'][0].shape == (n,) and R.pair_rbf(g, d['rbf'], d['drbf'], d['tgeo'])['rb'][0].shape == (0, 64)
    assert R.edge_tangent_geom(g, d['v'], -1.0)['tgeo'][0].shape == (0, 4) and R.embed(d['z'], d['embedding'])['out'][0].shape == (n, F)


def test_xcd_tile_map_is_a_bijection():
    for n in range(1, 201):
        assert sorted(R.xcd_tile(b, n) for b in range(n)) == list(range(n)), n


# ---------------------------------------------------------------------------------------------------------------------------
# derivative structure (torch float64 autograd; a smooth filter with the table's value and derivative at every edge)
# ---------------------------------------------------------------------------------------------------------------------------
class Smooth:
    """one small graph with masked pairs, float64 inputs, and the value stages written in torch"""

    def __init__(self):
        rng = np.random.default_rng(11)
        n = 9
        pairs = [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < 0.55]
        und = sorted(pairs)
        self.g = g = R.stage_graph(pairs, [4, 5] if all((a < 4) == (b < 4) for a, b in pairs) else [n],
                                   masked_pairs=[und[1], und[4], und[7]], seed=4)
        gen = torch.Generator().manual_seed(12)
        r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
        self.eps_p, self.deps_p = r(g.P, F), r(g.P, F)
        live_p = torch.ones(g.P, 1, dtype=torch.float64)
        live_p[torch.as_tensor(g.pid[g.masked])] = 0.0
        self.live_p = live_p                                                 # a masked pair reads zero rows of the table
        self.eps_p, self.deps_p = self.eps_p * live_p, self.deps_p * live_p
        self.pid, self.i, self.j = (torch.as_tensor(np.asarray(a, np.int64)) for a in (g.pid, g.i, g.j))
        self.own = torch.as_tensor(g.own)
        self.live_e = live_p[self.pid]
        self.filt = R.ExactFilter(self.eps_p[self.pid].numpy(), self.deps_p[self.pid].numpy())
        self.d = {k: r(*v.shape) if v.dtype == np.float32 else v for k, v in R.stage_inputs(g).items()}
        self.u_e = _t(g.geo[:, :3])

    def np(self, *names):
        return [self.d[n].numpy() for n in names]

    # value statements in torch; x_p: the pair's x relative to where the filter was read
    def message_fwd(self, m, a_in, x_p, eps_p=None):
        eps = (self.eps_p if eps_p is None else eps_p) + self.deps_p * x_p[:, None]
        msg_p = eps * m[self.i[self.own]] * m[self.j[self.own]]             # row p: pid of the owner edges ascends with e
        msg_e = msg_p[self.pid]
        return msg_p, a_in + torch.zeros_like(a_in).index_add_(0, self.i, msg_e)

    def force_fwd(self, phi1, phi2, u_e, f_in, has_f=True):
        t = phi1[self.pid][:, None, :] * u_e[:, :, None]
        if has_f:
            t = t + phi2[self.pid][:, None, :] * f_in[self.j]
        t = t * self.live_e[:, :, None]
        base = f_in if has_f else torch.zeros(self.g.N, 3, F, dtype=torch.float64)
        return base + torch.zeros(self.g.N, 3, F, dtype=torch.float64).index_add_(0, self.i, t)


@pytest.fixture(scope='module')
def smooth():
    s = Smooth()
    assert (s.g.pid[s.g.own] == np.arange(s.g.P)).all() and s.g.masked.any()
    return s


def _leaf(t):
    return t.clone().requires_grad_(True)


@pytest.mark.parametrize('need_gm', (0, 1))
def test_message_bwd_is_the_vjp_of_message_fwd(smooth, need_gm):
    s, g = smooth, smooth.g
    m, a_in, g_msg, g_a = (s.d[k] for k in ('m', 'a_in', 'g_msg', 'g_a'))
    ref = R.message_fwd(g, s.filt, m.numpy(), a_in.numpy())
    ml, xl = _leaf(m), torch.zeros(g.P, dtype=torch.float64, requires_grad=True)
    msg_p, a_mid = s.message_fwd(ml, a_in, xl)
    _close(ref['msg'][0], msg_p.detach().numpy())
    _close(ref['a_mid'][0], a_mid.detach().numpy())
    gm, gx = torch.autograd.grad((msg_p * g_msg).sum() + (a_mid * g_a).sum(), (ml, xl))
    out = R.message_bwd(g, s.filt, g_msg.numpy(), g_a.numpy(), m.numpy(), need_gm)
    _close(out['g_m'][0], gm.numpy())
    _close(out['g_x_pair'][0], gx.numpy())
    assert out['g_m'][2].all() == bool(need_gm) and out['g_m'][2].any() == bool(need_gm)
    assert not out['g_x_pair'][0][g.pid[g.masked]].any() and not ref['msg'][0][g.pid[g.masked]].any()


@pytest.mark.parametrize('has_f', (False, True))
def test_force_message_bwd_is_the_vjp_of_force_message_fwd(smooth, has_f):
    s, g = smooth, smooth.g
    phi1, phi2, f_in, gf = (s.d[k] for k in ('phi1', 'phi2', 'f_in', 'gf'))
    fin = f_in.numpy() if has_f else None
    ref = R.force_message_fwd(g, phi1.numpy(), phi2.numpy(), fin)
    p1, p2, ue, fl = _leaf(phi1), _leaf(phi2), _leaf(s.u_e), _leaf(f_in)
    f_out = s.force_fwd(p1, p2, ue, fl, has_f)
    _close(ref['f_out'][0], f_out.detach().numpy())
    grads = torch.autograd.grad((f_out * gf).sum(), (p1, p2, ue, fl), allow_unused=True)
    out = R.force_message_bwd(g, gf.numpy(), phi1.numpy(), phi2.numpy(), fin)
    _close(out['g_h12'][0][:, :F], grads[0].numpy())
    _close(out['g_u'][0][:, :3], grads[2].numpy())
    assert not out['g_u'][0][:, 3].any() and not out['g_u'][0][g.masked].any() and not out['g_h12'][0][g.pid[g.masked]].any()
    if has_f:
        _close(out['g_h12'][0][:, F:], grads[1].numpy())
        _close(out['g_fin'][0], grads[3].numpy())
        assert out['g_h12'][2].all() and out['g_fin'][2].all()
    else:
        assert not out['g_h12'][2][:, F:].any() and out['g_h12'][2][:, :F].all() and not out['g_fin'][2].any()
    # xg = NULL: nothing is masked
    live, s.live_e = s.live_e, torch.ones_like(s.live_e)
    try:
        _close(R.force_message_fwd(g, phi1.numpy(), phi2.numpy(), fin, use_mask=False)['f_out'][0],
               s.force_fwd(phi1, phi2, s.u_e, f_in, has_f).numpy())
    finally:
        s.live_e = live


def _geometry(pos, i, j, cutoff):
    d = pos[i] - pos[j]
    r = d.norm(dim=1, keepdim=True)
    return d / r, r[:, 0] / cutoff, r[:, 0]


def test_edge_embed_bwd_is_minus_the_gradient_and_the_strain_derivative(smooth):
    s, g = smooth, smooth.g
    pos = s.d['pos']
    u, x, r = _geometry(pos, s.i, s.j, g.cutoff)
    gg = R.Graph(**dict(g.__dict__, geo=torch.cat([u, r[:, None]], dim=1).numpy()))    # (float64: |u| = 1 to 1e-16)
    g_x, g_u = s.d['g_x'], s.d['g_u']
    # dL/d(disp) of L = sum_l g_x x(disp) + g_u . u(disp) at disp = r u
    disp = _leaf(u * r[:, None])
    strain = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
    posl = _leaf(pos)
    dd = disp + (posl[s.i] - posl[s.j]) - (pos[s.i] - pos[s.j]) + (pos[s.i] - pos[s.j]) @ strain
    rr = dd.norm(dim=1)
    L = (g_x.sum(0) * rr / g.cutoff).sum() + (g_u.sum(0)[:, :3] * dd / rr[:, None]).sum()
    gd, gpos, gS = torch.autograd.grad(L, (disp, posl, strain))
    out = R.edge_embed_bwd(gg, g_x.numpy(), g_u.numpy(), pos.numpy(), want_virial=True)
    _close(out['g_d'][0][:, :3], gd.numpy(), 1e-9)
    _close(out['forces'][0], -gpos.numpy(), 1e-9)
    _close(out['virial'][0][0] if g.B == 1 else out['virial'][0].sum(0), -0.5 * (gS + gS.T).numpy(), 1e-9)
    assert not out['g_d'][0][:, 3].any()
    assert not R.edge_embed_bwd(gg, g_x.numpy(), g_u.numpy())['g_d'][2].any()


@pytest.mark.parametrize('act', D.ACTIVATIONS)
@pytest.mark.parametrize('tables', (False, True))
def test_head_out_against_torch(smooth, act, tables):
    s, g = smooth, smooth.g
    e2, w4, b4, scale, shift = (s.d[k] for k in ('e2', 'w4', 'b4', 'scale', 'shift'))
    z = torch.as_tensor(s.d['z'])
    el = _leaf(e2)
    ae = TORCH_ACT[act](el) @ w4 + b4
    if tables:
        ae = ae * scale[z] + shift[z]
    mol = torch.as_tensor(np.searchsorted(g.mol_ptr, np.arange(g.N), side='right') - 1)
    energy = torch.zeros(g.B, dtype=torch.float64).index_add_(0, mol, ae)
    ge, = torch.autograd.grad(energy.sum(), el)
    out = R.head_out(e2.numpy(), w4.numpy(), b4.numpy(), scale.numpy() if tables else None, shift.numpy() if tables else None,
                     s.d['z'], g.mol_ptr, act)
    _close(out['atom_energy'][0], ae.detach().numpy())
    _close(out['g_e2'][0], ge.numpy())
    _close(out['energy'][0], energy.detach().numpy())


def test_edge_tangent_geom_is_the_jvp_of_the_geometry(smooth):
    s, g = smooth, smooth.g
    pos, v = s.d['pos'], s.d['v']
    u, x, r = _geometry(pos, s.i, s.j, g.cutoff)
    gg = R.Graph(**dict(g.__dict__, geo=torch.cat([u, r[:, None]], dim=1).numpy()))
    for sign in (-1.0, 0.75):
        _, (du, dx) = torch.autograd.functional.jvp(lambda p: _geometry(p, s.i, s.j, g.cutoff)[:2], pos, sign * v)
        out = R.edge_tangent_geom(gg, v.numpy(), sign)['tgeo'][0]
        _close(out[:, :3], du.numpy())
        _close(out[:, 3], dx.numpy())


def _tgeo(s):
    """a tangent geometry that is consistent over a pair: du antisymmetric, dx shared"""
    t = s.d['tgeo'].clone()
    own, rev = torch.as_tensor(s.g.own), torch.as_tensor(np.asarray(s.g.rev, np.int64))
    t[~own, :3], t[~own, 3] = -t[rev[~own], :3], t[rev[~own], 3]
    return t


@pytest.mark.parametrize('has_dm', (False, True))
def test_message_tangents_are_jvps(smooth, has_dm):
    s, g = smooth, smooth.g
    tg = _tgeo(s)
    dx_p = tg[:, 3][s.own]
    m, a_in, g_msg, g_a = (s.d[k] for k in ('m', 'a_in', 'g_msg', 'g_a'))
    zero = torch.zeros_like(m)
    dm, da_in = (s.d['dm'], s.d['da_in']) if has_dm else (zero, zero)
    x0 = torch.zeros(g.P, dtype=torch.float64)
    _, (dmsg, da_mid) = torch.autograd.functional.jvp(lambda mm, aa, xx: s.message_fwd(mm, aa, xx), (m, a_in, x0), (dm, da_in, dx_p))
    out = R.message_tan_fwd(g, s.filt, m.numpy(), tg.numpy(), dm.numpy() if has_dm else None, da_in.numpy() if has_dm else None)
    _close(out['dmsg'][0], dmsg.numpy())
    _close(out['da_mid'][0], da_mid.numpy())
    # tangent of the adjoint: (g_m, g_eps) as functions of (g_msg, g_a, m, x), along (dg_msg, dga, dm, dx)
    dg_msg, dga = s.d['dg_msg'], s.d['dga']

    def bwd(gmsg, ga, mm, xx):
        ml, el = _leaf(mm) if not mm.requires_grad else mm, s.eps_p.clone().requires_grad_(True)
        msg_p, a_mid = s.message_fwd(ml, torch.zeros_like(a_in), xx, el)
        return torch.autograd.grad((msg_p * gmsg).sum() + (a_mid * ga).sum(), (ml, el), create_graph=True)
    (gm0, ge0), (dgm, dge) = torch.autograd.functional.jvp(bwd, (g_msg, g_a, m, x0), (dg_msg, dga, dm, dx_p))
    out = R.message_tan_bwd(g, s.filt, g_msg.numpy(), dg_msg.numpy(), g_a.numpy(), dga.numpy(), m.numpy(), tg.numpy(),
                            dm.numpy() if has_dm else None)
    _close(out['g_eps'][0], ge0.detach().numpy())
    _close(out['dg_m'][0], dgm.detach().numpy())
    _close(out['dg_eps'][0], dge.detach().numpy())
    _close(R.message_bwd(g, s.filt, g_msg.numpy(), g_a.numpy(), m.numpy())['g_m'][0], gm0.detach().numpy())


@pytest.mark.parametrize('has_f', (False, True))
def test_force_message_tangents_are_jvps(smooth, has_f):
    s, g = smooth, smooth.g
    tg = _tgeo(s)
    du = tg[:, :3]
    phi1, phi2, f_in, gf = (s.d[k] for k in ('phi1', 'phi2', 'f_in', 'gf'))
    dphi1, dphi2, df_in, dgf = (s.d[k] for k in ('dphi1', 'dphi2', 'df_in', 'dgf'))
    _, df_out = torch.autograd.functional.jvp(lambda a, b, c, d: s.force_fwd(a, b, c, d, has_f), (phi1, phi2, s.u_e, f_in),
                                              (dphi1, dphi2, du, df_in))
    fin, dfin = (f_in.numpy(), df_in.numpy()) if has_f else (None, None)
    out = R.force_message_tan_fwd(g, phi1.numpy(), dphi1.numpy(), phi2.numpy(), dphi2.numpy(), tg.numpy(), fin, dfin)
    _close(out['df_out'][0], df_out.numpy())

    def bwd(gff, p2, ue, ff):
        p1l, p2l, fl = _leaf(phi1), (p2 if p2.requires_grad else _leaf(p2)), (ff if ff.requires_grad else _leaf(ff))
        f_out = s.force_fwd(p1l, p2l, ue, fl, has_f)
        return torch.autograd.grad((f_out * gff).sum(), (p1l, p2l, fl) if has_f else (p1l,), create_graph=True)
    _, tang = torch.autograd.functional.jvp(bwd, (gf, phi2, s.u_e, f_in), (dgf, dphi2, du, df_in))
    out = R.force_message_tan_bwd(g, gf.numpy(), dgf.numpy(), phi2.numpy(), dphi2.numpy(), tg.numpy(), fin, dfin)
    _close(out['dg_h12'][0][:, :F], tang[0].detach().numpy())
    if has_f:
        _close(out['dg_h12'][0][:, F:], tang[1].detach().numpy())
        _close(out['dg_fin'][0], tang[2].detach().numpy())
    else:
        assert not out['dg_fin'][2].any() and not out['dg_h12'][2][:, F:].any()
    assert not out['dg_h12'][0][g.pid[g.masked]].any()


def test_pair_rbf_and_embed(smooth):
    s, g = smooth, smooth.g
    rbf, drbf, tg = s.d['rbf'].numpy(), s.d['drbf'].numpy(), _tgeo(s).numpy()
    rb = R.pair_rbf(g, rbf, drbf, tg)['rb'][0]
    nb = rbf.shape[1]
    for e in np.flatnonzero(g.own):
        assert (rb[g.pid[e], :nb] == rbf[e]).all() and (rb[g.pid[e], 32:32 + nb] == drbf[e] * tg[e, 3]).all()
    assert not rb[:, nb:32].any() and not rb[:, 32 + nb:].any()
    out, B, _ = R.embed(s.d['z'], s.d['embedding'].numpy())['out']
    assert (out == s.d['embedding'].numpy()[s.d['z']]).all() and not B.any()


# ---------------------------------------------------------------------------------------------------------------------------
# chained over the layers of one molecule: tests/trace.py
# ---------------------------------------------------------------------------------------------------------------------------
def test_chained_statements_reproduce_the_trace():
    """ethanol (9 atoms, 3 layers): the forward and reverse edge stages fed with the trace's own node-side tensors give the
    trace's messages, sums, geometry gradients and forces.  The exact filter W rbf(x) stands in for the table (whose own 1e-7 is
    tests/test_hip_parity.py::test_radial_filter_tables_against_float64); what is left is float64 rounding and the fp32 rounding of
    the geometry the statements read (geo is an fp32 array: 1e-7 relative), hence 1e-6 of each array's largest element."""
    from tests import trace as TR
    from tests import util
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand')
    keep = batch == 0
    z, pos, cell, batch = z[keep], pos[keep], cell[:1], batch[keep]
    sd = util.load_state('rand')
    T = TR.trace(sd, z, pos, cell, batch)
    ei = T['edge_index'].numpy()
    n, L = z.shape[0], 3
    g = R.stage_graph([(int(a), int(b)) for a, b in ei.T], [n])
    to_e = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(g.i, g.j))}
    perm = np.array([to_e[(int(a), int(b))] for a, b in ei.T])             # trace edge -> CSR edge
    inv = np.argsort(perm)                                                   # CSR edge -> trace edge
    g.geo = np.concatenate([T['u'].numpy()[inv], T['r'].numpy()[inv][:, None]], axis=1).astype(np.float32)
    g.cutoff = 5.0
    own = g.own
    tol = 1e-6
    gxs, gus = [], []
    for l in range(L):
        t = lambda k: T[f'{k}_{l}'].numpy()  # noqa: E731
        We = sd[f'interaction_layers.{l}.message_edgepart.weight'].numpy()
        eps = (T['rbf'].numpy() @ We.T)[inv]
        # d eps / dx by autograd of the same expression
        from oracle import newtonnet_ref as ref
        xl = T['x'].clone().requires_grad_(True)
        freq = sd['embedding_layers.edge_embedding.embedding.frequencies']
        rb = ref.poly_envelope(xl[:, None]) * torch.sin(freq * xl[:, None]) / xl[:, None]
        ee = rb @ torch.as_tensor(We).T
        deps = torch.stack([torch.autograd.grad(ee[:, c].sum(), xl, retain_graph=True)[0] for c in range(F)], dim=1).numpy()[inv]
        filt = R.ExactFilter(eps, deps)
        a_prev = T['a0'].numpy() if l == 0 else T[f'a_out_{l - 1}'].numpy()
        out = R.message_fwd(g, filt, t('m'), a_prev)
        _close(out['msg'][0][g.pid], t('msg')[inv], tol)
        _close(out['a_mid'][0], t('a_mid'), tol)
        f_prev = None if l == 0 else T[f'f_out_{l - 1}'].numpy()
        phi1, phi2 = np.zeros((g.P, F)), np.zeros((g.P, F))
        phi1[g.pid[own]], phi2[g.pid[own]] = t('phi1')[inv][own], t('phi2')[inv][own]
        _close(phi1[g.pid], t('phi1')[inv], 1e-9)                           # symmetric under i <-> j
        _close(R.force_message_fwd(g, phi1, phi2, f_prev)['f_out'][0], t('f_out'), tol)
        gf = t('g_f_out')
        out = R.force_message_bwd(g, gf, phi1, phi2, f_prev)
        _close(out['g_u'][0][:, :3], t('g_u')[inv], tol)
        gp1 = t('g_phi1')[inv]
        _close(out['g_h12'][0][g.pid[own], :F], (gp1 + gp1[g.rev])[own], tol)
        if l:
            gp2 = t('g_phi2')[inv]
            _close(out['g_h12'][0][g.pid[own], F:], (gp2 + gp2[g.rev])[own], tol)
        # the trace's g_msg is the TOTAL gradient of a directed edge's message; the kernel's g_msg[p] is the MLP side of the pair
        ga = t('g_a_mid')
        tot = t('g_msg')[inv]
        g_msg = np.zeros((g.P, F))
        g_msg[g.pid[own]] = ((tot + tot[g.rev]) - ga[g.i] - ga[g.j])[own]
        out = R.message_bwd(g, filt, g_msg, ga, t('m'))
        gx = T[f'g_x_{l}'].numpy()[inv]
        _close(out['g_x_pair'][0][g.pid[own]], (gx + gx[g.rev])[own], tol)
        if l:
            _close(out['g_m'][0], t('g_m'), tol)
        gxe = np.zeros(g.E)
        gxe[own] = out['g_x_pair'][0][g.pid[own]]
        gxs.append(gxe)
        gus.append(np.concatenate([T[f'g_u_{l}'].numpy()[inv], np.zeros((g.E, 1))], axis=1))
    out = R.edge_embed_bwd(g, np.stack(gxs), np.stack(gus))
    _close(out['forces'][0], T['forces'].numpy(), tol)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' order of operations in fp32 stays inside the bounds
# ---------------------------------------------------------------------------------------------------------------------------
def _ranges(g, i, split):
    beg, end = int(g.row_ptr[i]), int(g.row_ptr[i + 1])
    mid = end - int(g.pair_ptr[i + 1] - g.pair_ptr[i])
    return ((beg, mid), (mid, end)) if split else ((beg, end),)


def _inside(got, ref, what):
    val, B, defined = ref
    err = np.abs(np.asarray(got, np.float64) - val)
    assert (err <= B).all(), (what, float((err / np.where(B > 0, B, 1)).max()))
    return float((err / np.where(B > 0, B, np.inf)).max(initial=0.0))


FORMS = ((1, True), (2, True), (4, True), (1, False))        # (waves per row, two ranges); the last: force_fwd_mol's one range


@pytest.mark.parametrize('name', list(R.GRAPHS))
def test_the_bounds_hold_for_the_kernels_summation_order(name, graphs, table):
    g = graphs[name]
    d = R.stage_inputs(g)
    filt = R.TableFilter(table, g.xg)
    f32 = np.float32
    fl = {e: R.filter32(table, g.xg, e) for e in range(g.E)}
    m, a_in, g_msg, g_a, phi1, phi2, f_in, gf = (d[k] for k in ('m', 'a_in', 'g_msg', 'g_a', 'phi1', 'phi2', 'f_in', 'gf'))
    i_of, j_of, pid = g.i, g.j, g.pid
    worst = {}
    refs = dict(mf=R.message_fwd(g, filt, m, a_in), mb=R.message_bwd(g, filt, g_msg, g_a, m),
                ff=R.force_message_fwd(g, phi1, phi2, f_in), fb=R.force_message_bwd(g, gf, phi1, phi2, f_in))
    live = ~g.masked
    for wpr, split in FORMS:
        a_mid, g_m, f_out, g_fin = (np.zeros(s, f32) for s in ((g.N, F), (g.N, F), (g.N, 3 * F), (g.N, 3 * F)))
        for i in range(g.N):
            rg = _ranges(g, i, split)
            one = ((int(g.row_ptr[i]), int(g.row_ptr[i + 1])),)
            # msg_fwd_kernel: one range, v = (eps m_i) m_j added; a_in last
            acc = R.row_sum32(one, wpr, lambda acc, e: acc + (fl[e][0] * m[i]) * m[j_of[e]], F)
            a_mid[i] = a_in[i] + acc

            def gm_step(acc, e):          # msg_bwd_kernel: G = (g_msg + ga_i) + ga_j; acc = fma(G eps, m_j, acc)
                G = (g_msg[pid[e]] + g_a[i]) + g_a[j_of[e]]
                return R.fma32(G * (fl[e][1] if j_of[e] > i else fl[e][0]), m[j_of[e]], acc)
            g_m[i] = R.row_sum32(_ranges(g, i, True), wpr, gm_step, F)

            def ff_step(acc, e):          # force_fwd_kernel: three phi1 u_k, then three phi2 f_j[k]
                if not live[e]:
                    return acc
                acc = np.concatenate([R.fma32(phi1[pid[e]], g.geo[e, k], acc[k * F:(k + 1) * F]) for k in range(3)])
                return R.fma32(np.tile(phi2[pid[e]], 3), f_in[j_of[e]].reshape(-1), acc)
            f_out[i] = R.row_sum32(rg, wpr, ff_step, 3 * F, first=f_in[i].reshape(-1))

            def fb_step(acc, e):          # force_bwd_kernel: acc = fma(phi2, gf_j, acc)
                return R.fma32(np.tile(phi2[pid[e]], 3), gf[j_of[e]].reshape(-1), acc) if live[e] else acc
            g_fin[i] = R.row_sum32(_ranges(g, i, True), wpr, fb_step, 3 * F, first=gf[i].reshape(-1))
        tag = f'{wpr} waves, {"two ranges" if split else "one range"}'
        worst[tag] = (_inside(a_mid, refs['mf']['a_mid'], 'a_mid ' + tag), _inside(g_m, refs['mb']['g_m'], 'g_m ' + tag),
                      _inside(f_out.reshape(g.N, 3, F), refs['ff']['f_out'], 'f_out ' + tag),
                      _inside(g_fin.reshape(g.N, 3, F), refs['fb']['g_fin'], 'g_fin ' + tag))
    # the pair rows and the 128-term dot products (one form each)
    own = np.flatnonzero(g.own)
    msg, gh, gx = np.zeros((g.P, F), f32), np.zeros((g.P, 2 * F), f32), np.zeros(g.P, f32)
    gu = np.zeros((g.E, 4), f32)
    for e in range(g.E):
        i, j, p = i_of[e], j_of[e], pid[e]
        if live[e]:
            gu[e, :3] = [R.tree_sum32(gf[i, k] * phi1[p]) for k in range(3)]
        if j < i:
            continue
        msg[p] = (fl[e][0] * m[i]) * m[j]
        G = (g_msg[p] + g_a[i]) + g_a[j]
        gx[p] = R.tree_sum32(((G * m[i]) * m[j]) * fl[e][2])
        if live[e]:
            a = (gf[i, 0] - gf[j, 0]) * g.geo[e, 0]
            for k in (1, 2):
                a = R.fma32(gf[i, k] - gf[j, k], g.geo[e, k], a)
            b = np.zeros(F, f32)
            for k in range(3):
                b = R.fma32(gf[j, k], f_in[i, k], R.fma32(gf[i, k], f_in[j, k], b))
            gh[p] = np.concatenate([a, b])
    worst['pair rows'] = (_inside(msg, refs['mf']['msg'], 'msg'), _inside(gx, refs['mb']['g_x_pair'], 'g_x'),
                          _inside(gh, refs['fb']['g_h12'], 'g_h12'), _inside(gu, refs['fb']['g_u'], 'g_u'))
    # the geometry adjoint: gd_of_edge, then 16 lanes stride the row and a butterfly adds them
    g_x, g_u = d['g_x'], d['g_u']
    inv_rc = f32(1.0) / f32(g.cutoff)
    gd = np.zeros((g.E, 4), f32)
    for e in range(g.E):
        sx, su = f32(0), np.zeros(3, f32)
        for l in range(g_x.shape[0]):
            sx, su = sx + g_x[l, e], su + g_u[l, e, :3]
        u, ir = g.geo[e, :3], f32(1.0) / g.geo[e, 3]
        dot = (su[0] * u[0] + su[1] * u[1]) + su[2] * u[2]
        a = sx * inv_rc - dot * ir
        gd[e, :3] = R.fma32(a, u, su * ir)
    forces = np.zeros((g.N, 3), f32)
    for i in range(g.N):
        lanes = np.zeros((16, 3), f32)
        for e in range(g.row_ptr[i], g.row_ptr[i + 1]):
            lanes[(e - g.row_ptr[i]) % 16] -= gd[e, :3] - gd[g.rev[e], :3]
        o = 8
        while o:
            lanes[:o] = lanes[:o] + lanes[o:2 * o]
            o //= 2
        forces[i] = lanes[0]
    ref = R.edge_embed_bwd(g, g_x, g_u, d['pos'], want_virial=True)
    seq = np.zeros((g.N, 3), f32)               # force_out_kernel (the two-launch path): one thread walks the row in order
    for i in range(g.N):
        for e in range(g.row_ptr[i], g.row_ptr[i + 1]):
            seq[i] -= gd[e, :3] - gd[g.rev[e], :3]
    # virial_kernel: float64 sums of the fp32 g_d, rounded once
    pos64 = d['pos'].astype(np.float64)
    s9 = np.zeros((g.B, 3, 3))
    mol = np.searchsorted(g.mol_ptr, g.i, side='right') - 1
    np.add.at(s9, mol, (pos64[g.i] - pos64[g.j])[:, :, None] * gd[:, None, :3].astype(np.float64))
    vir = (-0.5 * (s9 + s9.transpose(0, 2, 1))).astype(f32)
    worst['geometry adjoint'] = (_inside(gd, ref['g_d'], 'g_d'), _inside(forces, ref['forces'], 'forces'),
                                 _inside(seq, ref['forces'], 'forces, in order'), _inside(vir, ref['virial'], 'virial'))
    print('\nEDGE-REF-RATIO', name, {k: tuple(round(x, 3) for x in v) for k, v in worst.items()})
    assert all(0 < x <= 1 for v in worst.values() for x in v) or g.E == 0


@pytest.mark.parametrize('name', list(R.GRAPHS))
def test_the_bounds_hold_for_the_tangent_kernels_order(name, graphs, table):
    """csrc/train.hip: one wave per row, one range, every edge through the Hermite form; the pair rows from the owner's edge"""
    g = graphs[name]
    d = R.stage_inputs(g)
    filt = R.TableFilter(table, g.xg)
    fl = {e: R.filter32(table, g.xg, e) for e in range(g.E)}
    f32 = np.float32
    m, dm, da_in, tg = d['m'], d['dm'], d['da_in'], d['tgeo']
    g_msg, dg_msg, ga, dga = d['g_msg'], d['dg_msg'], d['g_a'], d['dga']
    phi1, dphi1, phi2, dphi2, f_in, df_in, gf, dgf = (d[k] for k in ('phi1', 'dphi1', 'phi2', 'dphi2', 'f_in', 'df_in', 'gf', 'dgf'))
    j_of, pid, live = g.j, g.pid, ~g.masked
    da_mid, dg_m = np.zeros((g.N, F), f32), np.zeros((g.N, F), f32)
    df_out, dg_fin = np.zeros((g.N, 3 * F), f32), np.zeros((g.N, 3 * F), f32)
    for i in range(g.N):
        one = ((int(g.row_ptr[i]), int(g.row_ptr[i + 1])),)

        def tf(acc, e):
            j = j_of[e]
            v = ((fl[e][2] * tg[e, 3]) * m[i]) * m[j]
            return acc + R.fma32(fl[e][1], R.fma32(dm[i], m[j], m[i] * dm[j]), v)
        da_mid[i] = R.row_sum32(one, 1, tf, F) + da_in[i]

        def tb(acc, e):
            j, p = j_of[e], pid[e]
            G, dG = (g_msg[p] + ga[i]) + ga[j], (dg_msg[p] + dga[i]) + dga[j]
            t = R.fma32(dG, fl[e][1], (G * fl[e][2]) * tg[e, 3])
            return R.fma32(G * fl[e][1], dm[j], R.fma32(t, m[j], acc))
        dg_m[i] = R.row_sum32(one, 1, tb, F)

        def ft(acc, e):
            if not live[e]:
                return acc
            p, j = pid[e], j_of[e]
            acc = np.concatenate([R.fma32(dphi1[p], g.geo[e, k], R.fma32(phi1[p], tg[e, k], acc[k * F:(k + 1) * F])) for k in range(3)])
            acc = R.fma32(np.tile(dphi2[p], 3), f_in[j].reshape(-1), acc)
            return R.fma32(np.tile(phi2[p], 3), df_in[j].reshape(-1), acc)
        df_out[i] = R.row_sum32(one, 1, ft, 3 * F, first=df_in[i].reshape(-1))

        def fb(acc, e):
            if not live[e]:
                return acc
            p, j = pid[e], j_of[e]
            return R.fma32(np.tile(phi2[p], 3), dgf[j].reshape(-1), R.fma32(np.tile(dphi2[p], 3), gf[j].reshape(-1), acc))
        dg_fin[i] = R.row_sum32(_ranges(g, i, True), 1, fb, 3 * F, first=dgf[i].reshape(-1))
    r1 = R.message_tan_fwd(g, filt, m, tg, dm, da_in)
    r2 = R.message_tan_bwd(g, filt, g_msg, dg_msg, ga, dga, m, tg, dm)
    r3 = R.force_message_tan_fwd(g, phi1, dphi1, phi2, dphi2, tg, f_in, df_in)
    r4 = R.force_message_tan_bwd(g, gf, dgf, phi2, dphi2, tg, f_in, df_in)
    dmsg, g_eps, dg_eps, dg_h12 = (np.zeros((g.P, w), f32) for w in (F, F, F, 2 * F))
    for e in np.flatnonzero(g.own):
        i, j, p = g.i[e], j_of[e], pid[e]
        v = ((fl[e][2] * tg[e, 3]) * m[i]) * m[j]
        dmsg[p] = R.fma32(fl[e][1], R.fma32(dm[i], m[j], m[i] * dm[j]), v)
        G, dG, mm = (g_msg[p] + ga[i]) + ga[j], (dg_msg[p] + dga[i]) + dga[j], m[i] * m[j]
        g_eps[p] = G * mm
        dg_eps[p] = R.fma32(G, R.fma32(dm[i], m[j], m[i] * dm[j]), dG * mm)
        if live[e]:
            a = (dgf[i, 0] - dgf[j, 0]) * g.geo[e, 0]
            for k in (1, 2):
                a = R.fma32(dgf[i, k] - dgf[j, k], g.geo[e, k], a)
            for k in range(3):
                a = R.fma32(gf[i, k] - gf[j, k], tg[e, k], a)
            b = np.zeros(F, f32)
            for k in range(3):
                b = R.fma32(dgf[i, k], f_in[j, k], b)
                b = R.fma32(gf[i, k], df_in[j, k], b)
                b = R.fma32(dgf[j, k], f_in[i, k], b)
                b = R.fma32(gf[j, k], df_in[i, k], b)
            dg_h12[p] = np.concatenate([a, b])
    worst = (_inside(da_mid, r1['da_mid'], 'da_mid'), _inside(dg_m, r2['dg_m'], 'dg_m'),
             _inside(df_out.reshape(g.N, 3, F), r3['df_out'], 'df_out'), _inside(dg_fin.reshape(g.N, 3, F), r4['dg_fin'], 'dg_fin'),
             _inside(dmsg, r1['dmsg'], 'dmsg'), _inside(g_eps, r2['g_eps'], 'g_eps'), _inside(dg_eps, r2['dg_eps'], 'dg_eps'),
             _inside(dg_h12, r4['dg_h12'], 'dg_h12'))
    print('\nEDGE-REF-RATIO tangent', name, tuple(round(x, 3) for x in worst))
    assert all(0 < x <= 1 for x in worst)


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds still discriminate
# ---------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ('drop_last_odd', 'twice_last_odd', 'upper_half_col', 'swap_phi', 'ignore_mask', 'own_upper', 'ga_i_only', 'rev_u_sign',
             'skip_first_row')


def mutated_view(g, mut):
    """the view of a WRONG kernel (edge_ref.View holds what a right one reads); swap_phi is an exchange of arguments (_statements)"""
    v = R.View(g)
    last = g.row_ptr[1:][R.degrees(g) % 2 == 1] - 1
    if mut == 'drop_last_odd':             # the last edge of a row of odd degree is not added ...
        v.w[last] = 0
    elif mut == 'twice_last_odd':          # ... or added twice (the clamped odd half-wave not masked off)
        v.w[last] = 2
    elif mut == 'upper_half_col':          # the upper half-wave gathers the sender of the lower half-wave's edge
        k = np.arange(g.E) - g.row_ptr[v.i]
        v.j = np.where(k % 2 == 1, g.j[np.maximum(np.arange(g.E) - 1, 0)], g.j)
    elif mut == 'ignore_mask':             # masked candidates treated as edges inside the cutoff
        v.live[:] = True
        v.xg = g.xg_live
    elif mut == 'own_upper':               # i >= j instead of i < j: the pair rows come from the upper endpoint's edge
        v.owner = ~g.own
    elif mut == 'ga_i_only':               # G = g_msg + g_a[i]
        v.ga_j = 0.0
    elif mut == 'rev_u_sign':              # the reverse edge reads the owner's direction: u is no longer antisymmetric
        v.u = np.where(g.own[:, None], v.u, -v.u)
        v.pair_sign = -1.0
    elif mut == 'skip_first_row':          # the first row of every molecule is never computed
        v.skip[g.mol_ptr[:-1][np.diff(g.mol_ptr) > 0]] = True
    else:
        assert mut in (None, 'swap_phi'), mut
    return v


def _statements(g, filt, d, mut=None):
    """every output of every statement that takes a graph, keyed 'stage.output'"""
    k = dict(view=mutated_view(g, mut)) if mut else {}
    one, two = ('2', '1') if mut == 'swap_phi' else ('1', '2')
    phi1, phi2, dphi1, dphi2 = d['phi' + one], d['phi' + two], d['dphi' + one], d['dphi' + two]
    out = {}

    def put(stage, res):
        for name, v in res.items():
            out[f'{stage}.{name}'] = v
    put('message_fwd', R.message_fwd(g, filt, d['m'], d['a_in'], **k))
    put('message_bwd', R.message_bwd(g, filt, d['g_msg'], d['g_a'], d['m'], **k))
    put('force_message_fwd', R.force_message_fwd(g, phi1, phi2, d['f_in'], **k))
    put('force_message_bwd', R.force_message_bwd(g, d['gf'], phi1, phi2, d['f_in'], **k))
    put('edge_embed_bwd', R.edge_embed_bwd(g, d['g_x'], d['g_u'], d['pos'], True, **k))
    put('message_tan_fwd', R.message_tan_fwd(g, filt, d['m'], d['tgeo'], d['dm'], d['da_in'], **k))
    put('message_tan_bwd', R.message_tan_bwd(g, filt, d['g_msg'], d['dg_msg'], d['g_a'], d['dga'], d['m'], d['tgeo'], d['dm'], **k))
    put('force_message_tan_fwd', R.force_message_tan_fwd(g, phi1, dphi1, phi2, dphi2, d['tgeo'], d['f_in'], d['df_in'], **k))
    put('force_message_tan_bwd', R.force_message_tan_bwd(g, d['gf'], d['dgf'], phi2, dphi2, d['tgeo'], d['f_in'], d['df_in'], **k))
    put('pair_rbf', R.pair_rbf(g, d['rbf'], d['drbf'], d['tgeo'], **k))
    return out


ROW_SUMS = ('message_fwd.a_mid', 'message_bwd.g_m', 'force_message_fwd.f_out', 'force_message_bwd.g_fin', 'edge_embed_bwd.forces',
            'message_tan_fwd.da_mid', 'message_tan_bwd.dg_m', 'force_message_tan_fwd.df_out', 'force_message_tan_bwd.dg_fin')
# which outputs a mutation must change (an output that does not read what the mutation spoils cannot see it; whatever else it
# changes -- a wrong sender also spoils the pair rows -- is held to the same factor):
#   the row sums see an edge dropped / counted twice, the lower half-wave's sender, a skipped row;
#   phi1 <-> phi2: whatever reads both;  the mask: whatever a masked edge would otherwise feed;
#   g_a[i] alone in G: whatever reads G;  +u on the reverse edge: whatever reads u of a non-owner edge or adds both directions;
#   the virial and g_d follow the forces' inputs but are formed per edge, not per row.
APPLIES = {
    'drop_last_odd': ROW_SUMS, 'twice_last_odd': ROW_SUMS, 'upper_half_col': tuple(r for r in ROW_SUMS if r != 'edge_embed_bwd.forces'),
    'skip_first_row': ROW_SUMS + ('message_bwd.g_x_pair', 'force_message_bwd.g_u'),
    'swap_phi': ('force_message_fwd.f_out', 'force_message_bwd.g_u', 'force_message_bwd.g_fin', 'force_message_tan_fwd.df_out'),
    'ignore_mask': ('message_fwd.msg', 'message_fwd.a_mid', 'message_bwd.g_m', 'message_bwd.g_x_pair', 'force_message_fwd.f_out',
                    'force_message_bwd.g_h12', 'force_message_bwd.g_u', 'force_message_bwd.g_fin', 'message_tan_fwd.dmsg',
                    'message_tan_fwd.da_mid', 'message_tan_bwd.dg_m', 'force_message_tan_fwd.df_out',
                    'force_message_tan_bwd.dg_h12', 'force_message_tan_bwd.dg_fin'),
    # the owner matters where a pair row is formed from a per-directed-edge input: dx_e, du_e, rbf_e, drbf_e (edge_ref: Ownership)
    'own_upper': ('message_tan_fwd.dmsg', 'force_message_tan_bwd.dg_h12', 'pair_rbf.rb'),
    'ga_i_only': ('message_bwd.g_m', 'message_bwd.g_x_pair', 'message_tan_bwd.dg_m', 'message_tan_bwd.g_eps', 'message_tan_bwd.dg_eps'),
    'rev_u_sign': ('force_message_fwd.f_out', 'force_message_bwd.g_h12', 'edge_embed_bwd.g_d', 'edge_embed_bwd.forces',
                   'edge_embed_bwd.virial', 'force_message_tan_fwd.df_out', 'force_message_tan_bwd.dg_h12'),
}


@pytest.mark.parametrize('name', list(R.GRAPHS))
def test_every_mutation_leaves_the_bound_by_ten_times(name, graphs, table):
    g = graphs[name]
    d = R.stage_inputs(g)
    filt = R.TableFilter(table, g.xg)
    ref = _statements(g, filt, d)
    assert set(APPLIES) == set(MUTATIONS) and all(k in ref for ks in APPLIES.values() for k in ks)
    seen = set()
    for mut in MUTATIONS:
        if mut == 'ignore_mask' and not g.masked.any():
            continue
        got = _statements(g, filt, d, mut)
        for key, (val, B, _) in ref.items():
            err = np.abs(got[key][0] - val)
            changed = bool((err > 1e-6 * B).any())       # (float64 rounding of a reordered sum is no change)
            assert changed or key not in APPLIES[mut], f'{name}: {mut} does not change {key}'
            if changed:                      # whatever the mutation moves at all, it moves far outside the bound
                ratio = np.where(B > 0, err / np.where(B > 0, B, 1.0), np.where(err > 0, np.inf, 0.0))
                assert ratio.max() > 10.0, f'{name}: {mut} moves {key} by only {ratio.max():.3g} x its bound'
                seen.add(key)
    assert seen >= set(ROW_SUMS)


def test_chained_tangent_statements_reproduce_the_tangent_reference():
    """the same molecule through tests/tangent_ref.py (sweeps 3 and 4 of training): the tangent statements fed with its node-side
    tensors give its per-edge tangents (pair rows: the sum of the two directed edges' rows where the reference keeps both)"""
    from tests import tangent_ref as TG
    from tests import util
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand')
    keep = batch == 0
    z, pos, cell, batch = z[keep], pos[keep], cell[:1], batch[keep]
    sd = util.load_state('rand')
    gen = torch.Generator().manual_seed(5)
    g_energy, g_forces = torch.randn(1, generator=gen, dtype=torch.float64), torch.randn(z.shape[0], 3, generator=gen, dtype=torch.float64)
    _, _, _, S = TG.train_grads(sd, z, pos, cell, batch, g_energy, g_forces, keep=True)
    ei = S['edge_index'].numpy()
    n, Ls = z.shape[0], S['layers']
    g = R.stage_graph([(int(a), int(b)) for a, b in ei.T], [n])
    to_e = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(g.i, g.j))}
    inv = np.argsort(np.array([to_e[(int(a), int(b))] for a, b in ei.T]))       # CSR edge -> reference edge
    r = (pos[ei[0]] - pos[ei[1]]).norm(dim=1, keepdim=True)
    g.geo = np.concatenate([S['u'].numpy(), r.numpy()], axis=1)[inv]            # (float64)
    own, rev, pid = g.own, g.rev, g.pid
    tgeo = np.concatenate([S['du'].numpy(), S['dx'].numpy()], axis=1)[inv]
    _close(R.edge_tangent_geom(g, S['v'].numpy(), 1.0)['tgeo'][0], tgeo)
    tol = 1e-10

    def pair(x):                       # a symmetric per-edge array of the reference as pair rows
        x = x.numpy()[inv]
        _close(x, x[rev], 1e-9)
        out = np.zeros((g.P,) + x.shape[1:])
        out[pid[own]] = x[own]
        return out

    def both(x):                       # the two directed edges' rows added, as pair rows
        x = x.numpy()[inv]
        out = np.zeros((g.P,) + x.shape[1:])
        out[pid[own]] = (x + x[rev])[own]
        return out
    W = lambda l, k: sd[f'interaction_layers.{l}.{k}']  # noqa: E731
    dGA = S['dg_e1'] @ sd['output_layers.0.layers.0.weight']
    for l in range(len(Ls) - 1, -1, -1):
        st = Ls[l]
        first = l == 0
        filt = R.ExactFilter(st['eps'].numpy()[inv], st['deps'].numpy()[inv])
        nn = lambda k: st[k].numpy()  # noqa: E731
        out = R.message_tan_fwd(g, filt, nn('m'), tgeo, None if first else nn('dm'), None if first else nn('da_in'))
        _close(out['dmsg'][0], pair(st['dmsg']), tol)
        _close(out['da_mid'][0], (st['da_in'] + TG._scat(st['dmsg'], S['edge_index'][0], n)).numpy(), tol)
        fin, dfin = (None, None) if first else (nn('f_in'), nn('df_in'))
        out = R.force_message_tan_fwd(g, pair(st['phi1']), pair(st['dphi1']), pair(st['phi2']), pair(st['dphi2']), tgeo, fin, dfin)
        _close(out['df_out'][0], nn('df_out'), tol)
        out = R.force_message_tan_bwd(g, nn('gf'), nn('dgf'), pair(st['phi2']), pair(st['dphi2']), tgeo, fin, dfin)
        _close(out['dg_h12'][0][:, :F], both(st['dg_phi1']), tol)
        if not first:
            _close(out['dg_h12'][0][:, F:], both(st['dg_phi2']), tol)
            i_, j_ = S['edge_index']
            fin_ref = st['dgf'] + TG._scat(st['dphi2'].unsqueeze(1) * st['gf'][i_] + st['phi2'].unsqueeze(1) * st['dgf'][i_], j_, n)
            _close(out['dg_fin'][0], fin_ref.numpy(), tol)
        # the reference's G / dG are per directed edge (MLP side of that edge + GA_i); the kernel's pair rows hold the MLP side of both
        GA = st['GA']
        dg_msg_e = sum(st[f'dg_h{k}'] @ W(l, f'equiv_message{k}.0.weight') for k in (1, 2))
        i_ = S['edge_index'][0]
        g_msg = both(st['G'] - GA[i_])
        dg_msg = both(dg_msg_e)
        out = R.message_tan_bwd(g, filt, g_msg, dg_msg, GA.numpy(), dGA.numpy(), nn('m'), tgeo, None if first else nn('dm'))
        _close(out['dg_m'][0], nn('dg_m'), tol)
        _close(out['g_eps'][0], both(st['g_eps']), tol)
        _close(out['dg_eps'][0], both(st['dg_eps']), tol)
        _close(R.message_bwd(g, filt, g_msg, GA.numpy(), nn('m'))['g_m'][0], nn('g_m'), tol)
        rb = R.pair_rbf(g, S['rbf'].numpy()[inv], S['drbf'].numpy()[inv], tgeo)['rb'][0]
        nb = S['rbf'].shape[1]
        _close(rb[:, :nb], pair(S['rbf']))
        _close(rb[:, 32:32 + nb], pair(S['drbf'] * S['dx']))
        dGA = dGA + st['dg_hn'] @ W(l, 'message_nodepart.0.weight')


@pytest.mark.parametrize('act', ('silu', 'tanh', 'relu'))
def test_the_bounds_hold_for_the_heads_order(act, graphs):
    """head_out_kernel in fp32: lane l holds features 2l, 2l + 1 (one fused product pair), the 64 lanes are added as a tree, the
    atom energy is one fused multiply-add, the molecule sums are float64 sums of the fp32 atom energies rounded once"""
    g = graphs['molecules']
    d = R.stage_inputs(g)
    f32 = np.float32
    e2, w4, b4, sc, sh = d['e2'], d['w4'], d['b4'][0], d['scale'][d['z']], d['shift'][d['z']]
    one = f32(1)
    sig = one / (one + np.exp(-e2))
    a, da = {'silu': (e2 * sig, sig * (one + e2 * (one - sig))), 'tanh': (np.tanh(e2), one - np.tanh(e2) * np.tanh(e2)),
             'relu': (np.maximum(e2, 0), (e2 > 0).astype(f32))}[act]
    assert a.dtype == f32 and da.dtype == f32
    s = R.tree_sum32(R.fma32(a[:, 0::2], w4[0::2], a[:, 1::2] * w4[1::2]))
    ae = R.fma32(s + b4, sc, sh)
    ge = (sc[:, None] * w4) * da
    mol = np.searchsorted(g.mol_ptr, np.arange(g.N), side='right') - 1
    E = np.zeros(g.B)
    np.add.at(E, mol, ae.astype(np.float64))
    ref = R.head_out(e2, w4, d['b4'], d['scale'], d['shift'], d['z'], g.mol_ptr, act)
    worst = (_inside(ae, ref['atom_energy'], 'atom_energy'), _inside(ge, ref['g_e2'], 'g_e2'), _inside(E.astype(f32), ref['energy'], 'energy'))
    print('\nEDGE-REF-RATIO head', act, tuple(round(x, 3) for x in worst))
    assert all(x <= 1 for x in worst) and worst[0] > 0
