"""CPU-side checks of tests/hvp_ref.py, the float64 statements and bounds the kernel test of the Hessian and strain tail
(tests/test_hip_hvp_stages.py) compares against:
  * every statement is the JVP, by torch float64 autograd, of the value statement of tests/edge_ref.py it is the tangent of;
  * the analytic second derivative of the basis agrees with mpmath's numerical differentiation (longdouble central differences
    where mpmath is missing);
  * chained after the sweeps of tests/tangent_ref.py the statements give a column of the oracle's Hessian and the second strain
    derivatives of elastic_ref.StrainedOracle;
  * an fp32 restatement of each kernel's own order of operations stays inside the bound on every case of the kernel test
    (`RESTATED-RATIO` lines);
  * fourteen wrong kernels, applied to the statements, leave the bound by more than ten times in every output they change."""
import numpy as np
import pytest
import torch

from tests import edge_ref as R
from tests import elastic_ref
from tests import hessian_ref
from tests import hvp_ref as H
from tests import tangent_ref
from tests import util

f64 = np.float64
JVP_TOL = 1e-11


def _close(got, want, tol, what):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    top = max(float(np.abs(want).max()), 1e-300) if want.size else 1.0
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= tol * top, f'{what}: {err:.3g} against {tol:g} x {top:.3g}'


def _t(a):
    return torch.from_numpy(np.asarray(a, f64))


def _jvp(fn, primals, tangents):
    out, tan = torch.autograd.functional.jvp(fn, tuple(_t(p) for p in primals), tuple(_t(t) for t in tangents))
    return out.numpy(), tan.numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. JVPs of the value statements
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,use_mask', [('degrees', True), ('masked', True), ('masked', False), ('molecules', True)])
def test_dg_u_is_the_jvp_of_g_u(name, use_mask):
    g, d = H.dgu_inputs(name)
    s = R.stage_inputs(g)
    i, pid, live = torch.from_numpy(g.i), torch.from_numpy(g.pid.astype(np.int64)), _t(~g.masked if use_mask else np.ones(g.E))

    def g_u(gf, phi1):
        return (gf[i] * phi1[pid][:, None, :]).sum(2) * live[:, None]
    val, tan = _jvp(g_u, (d['gf'], d['phi1']), (d['dgf'], d['dphi1']))
    _close(val, R.force_message_bwd(g, d['gf'], d['phi1'], s['phi2'], use_mask=use_mask)['g_u'][0][:, :3], 1e-13, 'g_u in torch')
    ref = H.hvp_dgu(g, **d, use_mask=use_mask)['dg_u'][0]
    _close(ref[:, :3], tan, JVP_TOL, 'dg_u')
    assert not ref[:, 3].any() and (not use_mask or not ref[g.masked].any())


def _torch_envelope(x, env):
    if env == H.ENV_COSINE:
        return 0.5 * (1 + torch.cos(np.pi * x))
    p = env if env > 0 else 9
    return 1 - 0.5 * (p + 1) * (p + 2) * x ** p + p * (p + 2) * x ** (p + 1) - 0.5 * p * (p + 1) * x ** (p + 2)


@pytest.mark.parametrize('env', (0,) + H.ENVELOPES)
@pytest.mark.parametrize('name', ('degrees', 'masked'))
def test_dg_x_is_the_jvp_of_g_x(name, env):
    g, d = H.dgx_inputs(name, 20, False)
    W, w = _t(d['W']), _t(d['freq'])
    own = np.flatnonzero(g.own)
    x0 = H.x_of(g)

    def eps(x):                                           # [n][F] of x [n]
        return (_torch_envelope(x, env)[:, None] * torch.sin(w * x[:, None]) / x[:, None]) @ W.T

    def deps(x):
        return torch.autograd.functional.jvp(eps, x, torch.ones_like(x), create_graph=True)[1]    # row n depends on x[n] alone
    # the value statement: message_bwd's g_x on the owner's edge with G m_i m_j = g_eps (m = 1, g_a = 0, g_msg = g_eps)
    d1 = deps(_t(x0)).detach().numpy()
    filt = R.ExactFilter(eps(_t(x0)).numpy(), d1)
    ones, zeros = np.ones((g.N, R.F)), np.zeros((g.N, R.F))
    gx_pair = R.message_bwd(g, filt, d['g_eps'], zeros, ones)['g_x_pair'][0]
    pid = torch.from_numpy(g.pid[own].astype(np.int64))

    def g_x(g_eps, x):
        return (g_eps[pid] * deps(x)).sum(1)
    val, tan = _jvp(g_x, (d['g_eps'], x0[own]), (d['dg_eps'], d['tgeo'][own, 3]))
    _close(val, gx_pair[g.pid[own]], 1e-13, 'g_x in torch')
    ref = H.hvp_dgx(g, d['tgeo'], d['g_eps'], d['dg_eps'], d['W'], d['freq'], env)['dg_x'][0]
    live = ~g.masked[own]
    _close(ref[own][live], tan[live], JVP_TOL, 'dg_x')
    assert not ref[~g.own].any() and not ref[g.masked].any()


@pytest.mark.parametrize('name,L', (('degrees', 3), ('wide row', 1), ('molecules', 8)))
def test_dg_d_and_hv_are_the_jvp_of_the_geometry_adjoint(name, L):
    g = H.graph(name)
    rng = H._rng('jvp out', name)
    d = dict(g_x=H._r(rng, L, g.E), g_u=H._r(rng, L, g.E, 4), dg_x=H._r(rng, L, g.E), dg_u=H._r(rng, L, g.E, 4), tgeo=H._r(rng, g.E, 4))
    i, rev, rc = torch.from_numpy(g.i), torch.from_numpy(g.rev.astype(np.int64)), g.cutoff

    def g_d(g_x, g_u, u, r):
        gx, gu = g_x.sum(0)[:, None], g_u.sum(0)
        return (gx / rc - (gu * u).sum(1, keepdim=True) / r) * u + gu / r

    def forces(g_x, g_u, u, r):
        gd = g_d(g_x, g_u, u, r)
        return -torch.zeros(g.N, 3, dtype=torch.float64).index_add_(0, i, gd - gd[rev])
    geo = g.geo.astype(f64)
    primals = (d['g_x'], d['g_u'][..., :3], geo[:, :3], geo[:, 3:4])
    tangents = (d['dg_x'], d['dg_u'][..., :3], d['tgeo'][:, :3], d['tgeo'][:, 3:4].astype(f64) * rc)
    value = R.edge_embed_bwd(g, d['g_x'], d['g_u'])
    ref = H.hvp_out(g, **d)
    val, tan = _jvp(g_d, primals, tangents)
    _close(val, value['g_d'][0][:, :3], 1e-13, 'g_d in torch')
    _close(ref['dg_d'][0][:, :3], tan, JVP_TOL, 'dg_d')
    val, tan = _jvp(forces, primals, tangents)
    _close(val, value['forces'][0], 1e-13, 'forces in torch')
    _close(ref['hv'][0], -tan, JVP_TOL, 'hv')
    assert not ref['dg_d'][0][:, 3].any()


def test_strain_seed_is_the_jvp_of_the_strained_geometry():
    g, batch, eta6 = H.strain_inputs()
    geo = g.geo.astype(f64)
    geo[:, :3] /= np.linalg.norm(geo[:, :3], axis=1, keepdims=True)       # (the statement takes u as a unit vector, as the kernel does)
    g = R.Graph(**dict(g.__dict__, geo=geo))
    d0 = _t(geo[:, 3:4] * geo[:, :3])
    eta = torch.stack([elastic_ref.voigt_matrix(_t(e)) for e in eta6])[torch.from_numpy(batch[g.i])]

    def geom(t):
        d = d0 + t * torch.bmm(eta, d0.unsqueeze(-1)).squeeze(-1)
        r = d.norm(dim=1, keepdim=True)
        return torch.cat([d / r, r / g.cutoff], dim=1)
    _, tan = torch.autograd.functional.jvp(geom, torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64))
    _close(H.strain_tan_geom(g, batch, eta6)['tgeo'][0], tan.numpy(), JVP_TOL, 'strain tgeo')


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the basis derivatives
# ---------------------------------------------------------------------------------------------------------------------------
X_POINTS = (0.02, 0.5, 0.9, 1.0 - 2.0 ** -20)


@pytest.mark.parametrize('env', H.ENVELOPES)
def test_basis_second_derivatives(env):
    freq = (np.array([1, 8, 20, 32]) * np.pi).astype(np.float32)
    x = np.array(X_POINTS)
    r1, r2, A1, A2 = H.rbf_d12(x, freq, env)
    e0, e1, e2 = (np.asarray(t, f64) for t in H.envelope_d012(x, env))
    try:
        import mpmath as mp
    except ImportError:
        mp = None
    for a, xa in enumerate(x):
        for n, wn in enumerate(freq.astype(f64)):
            if mp is not None:
                mp.mp.dps = 50
                p = env if env > 0 else 9
                fe = (lambda y: (1 + mp.cos(mp.pi * y)) / 2) if env == H.ENV_COSINE else (
                    lambda y: 1 - mp.mpf((p + 1) * (p + 2)) / 2 * y ** p + p * (p + 2) * y ** (p + 1) - mp.mpf(p * (p + 1)) / 2 * y ** (p + 2))
                fr = lambda y: fe(y) * mp.sin(mp.mpf(float(wn)) * y) / y  # noqa: E731
                xm = mp.mpf(float(xa))
                want1, want2, wenv2 = float(mp.diff(fr, xm, 1)), float(mp.diff(fr, xm, 2)), float(mp.diff(fe, xm, 2))
                tol = 1e-13
            else:
                LD = np.longdouble
                h = LD(2.0) ** -16

                def fr(y):
                    e = 0.5 * (1 + np.cos(H.PI_LD * y)) if env == H.ENV_COSINE else H.envelope_d012(y, env)[0]
                    return e * np.sin(LD(wn) * y) / y
                xl = LD(xa)
                want1 = float((fr(xl + h) - fr(xl - h)) / (2 * h))
                want2 = float((fr(xl + h) - 2 * fr(xl) + fr(xl - h)) / (h * h))
                wenv2 = e2[a]
                tol = 1e-6
            assert abs(r1[a, n] - want1) <= tol * A1[a, n], (env, xa, wn, r1[a, n], want1)
            assert abs(r2[a, n] - want2) <= tol * A2[a, n], (env, xa, wn, r2[a, n], want2)
            assert abs(e2[a] - wenv2) <= 1e-13 * max(abs(wenv2), 1.0), (env, xa, e2[a], wenv2)    # (term by term: its terms reach 1e4)
    # the envelope and its first derivative vanish at the cutoff, and the factored forms of the polynomial say the same
    last = x[-1]
    assert abs(e0[-1]) < 10 * (1 - last) ** 2 and abs(e1[-1]) < 10 * (1 - last)
    if env != H.ENV_COSINE:
        p = float(env)
        K = 0.5 * p * (p + 1) * (p + 2)
        _close(e1, -K * x ** (p - 1) * (1 - x) ** 2, 1e-12, "env'")
        assert abs(e2[-1] - 2 * K * (1 - last)) < 1e-3 * abs(e2[-1])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. and 4. chained with the sweeps of tangent_ref
# ---------------------------------------------------------------------------------------------------------------------------
def oracle_graph(S, n_atoms, mol_ptr, cutoff=5.0):
    """(graph, order): the directed edges of a tangent_ref run sorted by receiver, every edge with a pair row of its own"""
    ei = S['edge_index'].numpy()
    order = np.lexsort((ei[1], ei[0]))
    i, j = ei[0][order], ei[1][order]
    E = i.size
    disp = S['disp'].numpy()[order]
    where = {}
    for e in range(E):
        where.setdefault((int(i[e]), int(j[e])), []).append(e)
    rev = np.zeros(E, np.int64)
    for e in range(E):                                    # periodic images: the reverse edge is the one with the opposite vector
        cand = where[(int(j[e]), int(i[e]))]
        rev[e] = cand[int(np.argmin([np.abs(disp[c] + disp[e]).max() for c in cand]))]
        assert np.abs(disp[rev[e]] + disp[e]).max() < 1e-9
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n_atoms))]).astype(np.int32)
    geo = np.concatenate([S['u'].numpy()[order], S['r'].numpy()[order]], axis=1)
    own = (i < j) | ((i == j) & (np.arange(E) < rev))
    g = R.Graph(N=n_atoms, E=E, P=E, B=len(mol_ptr) - 1, row_ptr=row_ptr, col=j.astype(np.int32), rev=rev, pid=np.arange(E, dtype=np.int32),
                mol_ptr=np.asarray(mol_ptr, np.int32), edge_index=np.stack([i, j]), geo=geo, xg=np.zeros((E, 2), np.int32),
                masked=np.zeros(E, bool), cutoff=float(cutoff), x_exact=S['x'].numpy()[order, 0])
    return g, order, own


def chained_tail(sd, S, g, order, own, envelope=9):
    """the statements of hvp_ref on the intermediates of tangent_ref: (dg_d, hv)"""
    Ls = S['layers']
    freq = sd['embedding_layers.edge_embedding.embedding.frequencies'].numpy()
    tgeo = np.concatenate([S['du'].numpy(), S['dx'].numpy()], axis=1)[order]
    view = R.View(g)
    view.owner = own
    g_x, g_u, dg_x, dg_u = [], [], [], []
    for l, st in enumerate(Ls):
        e = {k: st[k].numpy() for k in ('gf', 'dgf')}
        pe = {k: st[k].numpy()[order] for k in ('phi1', 'dphi1', 'g_eps', 'dg_eps', 'g_x', 'g_u')}
        W = sd[f'interaction_layers.{l}.message_edgepart.weight'].numpy()
        pair = lambda a: a + a[g.rev]  # noqa: E731  (a pair row is the sum of the two directions' rows of the per-edge model)
        dg_u.append(H.hvp_dgu(g, e['gf'], e['dgf'], pe['phi1'], pe['dphi1'])['dg_u'][0])
        dg_x.append(H.hvp_dgx(g, tgeo, pair(pe['g_eps']), pair(pe['dg_eps']), W, freq, envelope, view=view)['dg_x'][0])
        g_x.append(pe['g_x'][:, 0])
        g_u.append(np.concatenate([pe['g_u'], np.zeros((g.E, 1))], axis=1))
    out = H.hvp_out(g, np.stack(g_x), np.stack(g_u), np.stack(dg_x), np.stack(dg_u), tgeo)
    return out['dg_d'][0], out['hv'][0]


def test_chained_statements_reproduce_a_hessian_column():
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand')
    keep = batch == 0
    z, pos, cell, batch = z[keep], pos[keep], cell[:1], batch[keep]
    sd = util.load_state('rand')
    n = z.shape[0]
    for col in (1, 3 * (n - 1) + 2):
        v = torch.zeros(n, 3, dtype=torch.float64)
        v.view(-1)[col] = 1.0
        S = tangent_ref.train_grads(sd, z, pos, cell, batch, torch.zeros(1, dtype=torch.float64), -v, keep=True)[3]
        g, order, own = oracle_graph(S, n, [0, n])
        _, hv = chained_tail(sd, S, g, order, own)
        want = hessian_ref.oracle_hessian_columns(sd, z, pos, cell, batch, [col])[0].numpy()
        _close(hv, want, 1e-9, f'H e_{col}')


def test_chained_statements_reproduce_the_strain_derivatives():
    z, pos, cell, batch = elastic_ref.supercell(0)
    sd = util.load_state('rand')
    n = z.shape[0]
    eta = torch.tensor([[0.3, -0.2, 0.5, 0.7, -0.4, 0.6]], dtype=torch.float64)
    oracle = elastic_ref.StrainedOracle(sd, z, pos, cell, batch)
    dgrad, d2 = oracle.strain_tangent(eta)
    dd = (elastic_ref.voigt_matrix(eta[0]) @ oracle.disp.T).T
    zero = torch.zeros(n, 3, dtype=torch.float64)
    S = tangent_ref.train_grads(sd, z, pos, cell, batch, torch.zeros(1, dtype=torch.float64), zero, keep=True, edge_dd=dd)[3]
    assert torch.equal(S['edge_index'], oracle.edge_index)
    g, order, own = oracle_graph(S, n, [0, n])
    seed = H.strain_tan_geom(g, batch.numpy(), eta.numpy())['tgeo'][0]
    _close(seed, np.concatenate([S['du'].numpy(), S['dx'].numpy()], axis=1)[order], 1e-12, 'strain seed')
    dg_d, hv = chained_tail(sd, S, g, order, own)
    _close(hv, dgrad.numpy(), 1e-9, 'd(dE/dpos)/d eta')
    born = H.strain_born(dg_d, g.geo, g.row_ptr, g.mol_ptr, dtype=f64)['d2'][0]
    _close(born, d2.numpy(), 1e-9, 'd(dE/de)/d eta')


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the kernels' own order of operations in fp32 stays inside the bounds, on the cases of the kernel test
# ---------------------------------------------------------------------------------------------------------------------------
def _restated(stage, what, got, ref):
    r = H.ratio(got, ref)
    print(f'RESTATED-RATIO {stage} {what}: {r:.3f}')
    assert r <= 1.0, (stage, what, r)
    return r


def test_restatements_stay_inside_the_bounds():
    worst = {}

    def put(stage, what, got, ref):
        worst[stage] = max(worst.get(stage, 0.0), _restated(stage, what, got, ref))
    for name, m in H.DGU_CASES:
        g, d = H.dgu_inputs(name)
        put('hvp_dgu dg_u', f'{name}, mask {m}', H.dgu32(g, **d, use_mask=m), H.hvp_dgu(g, **d, use_mask=m)['dg_u'])
    for name, nb, env, m, own in H.DGX_CASES:
        g, d = H.dgx_inputs(name, nb, own)
        a = (g, d['tgeo'], d['g_eps'], d['dg_eps'], d['W'], d['freq'], env)
        put('hvp_dgx dg_x', f'{name}, nb {nb}, env {env}, mask {m}, own rows {own}', H.dgx32(*a, use_mask=m), H.hvp_dgx(*a, use_mask=m)['dg_x'])
    for name, L in H.OUT_CASES:
        g, d = H.out_inputs(name, L)
        ref = H.hvp_out(g, **d)
        gd, hv = H.out32(g, **d)
        put('hvp_out dg_d', f'{name}, {L} layers', gd, ref['dg_d'])
        put('hvp_out hv', f'{name}, {L} layers', hv, ref['hv'])
        assert not gd[:, 3].any()
    g, batch, eta6 = H.strain_inputs()
    for n in H.STRAIN_EDGES:
        put('strain_tan_geom tgeo', f'E = {n}', H.strain_tan32(g, batch, eta6, n), H.strain_tan_geom(g, batch, eta6, n)['tgeo'])
    for swap in (False, True):
        g, dg_d, geo = H.born_inputs(swap)
        put('strain_born d2', f'swap {swap}', H.born64(dg_d, geo, g.row_ptr, g.mol_ptr), H.strain_born(dg_d, geo, g.row_ptr, g.mol_ptr)['d2'])
    for stage, r in sorted(worst.items()):
        print(f'RESTATED-RATIO {stage}: worst {r:.3f}')


def test_the_cases_have_the_shapes_the_kernel_test_relies_on():
    assert H.graph('complete').E == 9120 > 8192
    assert sorted({H.graph(n).N for n, _ in H.DGU_CASES})[:5] == [1, 3, 4, 5, 33]
    deg = R.degrees(H.graph('wide row'))
    assert deg.max() == 130 and 65 in deg and 0 in R.degrees(H.graph('degrees'))
    g = H.edges_graph()
    inside, outside = H.last_r_inside(g.cutoff)
    x = lambda r: f64(r) * f64(np.float32(1) / np.float32(g.cutoff))  # noqa: E731
    assert x(inside) < 1.0 <= x(outside) and outside == np.nextafter(inside, np.float32(np.inf))
    for name, L in H.OUT_CASES:
        g, d = H.out_inputs(name, L)
        assert np.isnan(d['g_u'][..., 3]).all() and np.isnan(d['dg_u'][..., 3]).all() and np.isfinite(d['tgeo']).all()
    assert [H.out_inputs(n, L)[0].E for n, L in H.OUT_CASES[:3]] == [255, 256, 257]
    g, batch, eta6 = H.strain_inputs()
    assert g.E == 404 and batch.dtype == np.int64
    g, dg_d, geo = H.born_inputs()
    assert tuple(np.diff(g.mol_ptr)) == H.BORN_SIZES and (R.degrees(g)[g.mol_ptr[5] + 64:] > 0).any()
    for n_rep in H.HESS_REPS:                              # the replica scheme writes every block element exactly once
        batch, mol_ptr, blk_ptr, n_mol0, n_blk = H.hess_inputs(n_rep)
        passes, _ = hessian_ref.pass_count(3 * max(H.HESS_SIZES), n_rep)
        count = np.zeros(n_blk, int)
        for k in range(passes):
            idx, val = H.hess_scatter(H.hess_hv(batch.size, k), batch, mol_ptr, blk_ptr, k, n_rep, n_mol0)
            np.add.at(count, idx, 1)
            v = H.hess_dirs(batch, mol_ptr, k, n_rep, n_mol0)
            live = np.flatnonzero(v.any(axis=1))               # one unit entry per molecule whose column this pass writes
            assert idx.size == 3 * int(np.diff(mol_ptr)[batch[live]].sum()) and (v.sum(axis=1)[live] == 1).all()
        assert (count == 1).all()
        assert H.hess_scatter(H.hess_hv(batch.size, passes), batch, mol_ptr, blk_ptr, passes, n_rep, n_mol0)[0].size == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 6. wrong kernels leave the bounds
# ---------------------------------------------------------------------------------------------------------------------------
def _dgu_mut(mut):
    for name, m in H.DGU_CASES:
        g, d = H.dgu_inputs(name)
        v = R.View(g, m)
        v.live[:] = True
        yield f'{name} {m}', H.hvp_dgu(g, **d, use_mask=m), H.hvp_dgu(g, **d, view=v)


def _dgx_mut(mut):
    for name, nb, env, m, own in H.DGX_CASES:
        if name == 'complete':
            continue
        g, d = H.dgx_inputs(name, nb, own)
        a = (g, d['tgeo'], d['g_eps'], d['dg_eps'], d['W'], d['freq'], env)
        v = R.View(g, m)
        if mut == 'owner_gt':
            v.owner = g.i > g.j
        if mut == 'dgx_nomask':
            v.live[:] = True
        yield f'{name} {nb} {env} {m} {own}', H.hvp_dgx(*a, use_mask=m), H.hvp_dgx(*a, view=v, mut=(mut,))


def _out_mut(mut):
    for name, L in H.OUT_CASES:
        g, d = H.out_inputs(name, L)
        yield f'{name} {L}', H.hvp_out(g, **d), H.hvp_out(g, **d, mut=(mut,))


def _strain_mut(mut):
    g, batch, eta6 = H.strain_inputs()
    for n in H.STRAIN_EDGES:
        yield f'E = {n}', H.strain_tan_geom(g, batch, eta6, n), H.strain_tan_geom(g, batch, eta6, n, mut=(mut,))


def _born_mut(mut):
    g, dg_d, geo = H.born_inputs()
    yield 'born', H.strain_born(dg_d, geo, g.row_ptr, g.mol_ptr), H.strain_born(dg_d, geo, g.row_ptr, g.mol_ptr, mut=(mut,))


MUTATIONS = {
    'no_eps2': _dgx_mut,            # the eps'' term dropped
    'env_b_factor1': _dgx_mut,      # 2 env' b' with factor 1
    'p1_as_p2': _dgx_mut,           # the p = 1 branch replaced by the general formula at p = 2
    'owner_gt': _dgx_mut,           # owner taken as i > j
    'dgu_nomask': _dgu_mut,         # mask ignored in dg_u
    'dgx_nomask': _dgx_mut,         # mask ignored in dg_x
    'sign_gdu_dr': _out_mut,        # the sign of (g_u.u) dr / r^2
    'no_gu_du': _out_mut,           # g_u.du dropped
    'last_layer_out': _out_mut,     # the last layer left out of the layer sums
    'rev_as_e': _out_mut,           # rev[e] read as e
    'born_lane64': _born_mut,       # atoms at lane index 64 and above dropped
    'voigt_no_half': _strain_mut,   # shear factor 1/2 dropped in voigt_matrix
    's5_twice': _born_mut,          # s5 + s7 replaced by 2 s5
}


@pytest.mark.parametrize('mut', sorted(MUTATIONS))
def test_every_mutation_leaves_the_bound_by_ten_times(mut):
    changed = 0
    for what, right, wrong in MUTATIONS[mut](mut):
        for k, (val, B, _) in right.items():
            w = wrong[k][0]
            moved = w != val
            if not moved.any():
                continue
            changed += 1
            r = H.ratio(w, right[k])
            print(f'MUTATION {mut} {what} {k}: {int(moved.sum())} elements moved, worst ratio {r:.3g}')
            assert r > 10.0, (mut, what, k, r)
    assert changed, f'{mut} changes no output of any case'


def test_the_scatter_without_its_modulus_leaves_the_blocks():
    """b % n_mol0 dropped: a replica's columns land at the offsets of molecules the original batch does not have"""
    for n_rep in (2, 3, 5):
        batch, mol_ptr, blk_ptr, n_mol0, n_blk = H.hess_inputs(n_rep)
        sizes = np.diff(mol_ptr).astype(np.int64)
        wide = np.concatenate([[0], np.cumsum(9 * sizes * sizes)])[:-1]        # what such a kernel would read behind blk_ptr
        idx, val = H.hess_scatter(H.hess_hv(batch.size, 0), batch, mol_ptr, blk_ptr, 0, n_rep, n_mol0)
        bad, _ = H.hess_scatter(H.hess_hv(batch.size, 0), batch, mol_ptr, wide, 0, n_rep, n_mol0, mut=('scatter_no_mod',))
        assert idx.max() < n_blk <= bad.max() and not np.array_equal(idx, bad)
    batch, mol_ptr, blk_ptr, n_mol0, n_blk = H.hess_inputs(1)                # one replica: the modulus is the identity
    a = H.hess_scatter(H.hess_hv(batch.size, 0), batch, mol_ptr, blk_ptr, 0, 1, n_mol0)
    b = H.hess_scatter(H.hess_hv(batch.size, 0), batch, mol_ptr, blk_ptr, 0, 1, n_mol0, mut=('scatter_no_mod',))
    assert np.array_equal(a[0], b[0])


# ---------------------------------------------------------------------------------------------------------------------------
# the entry points: declared, exported, and refusing bad arguments before any launch (no GPU is touched: no pointer is followed)
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_stage_entry_points_are_exported_and_check_their_arguments():
    from newtonnet_amd import abi, hip
    names = ('nnhip_hvp_dgu', 'nnhip_hvp_dgx', 'nnhip_hvp_out', 'nnhip_hess_dirs', 'nnhip_hess_scatter', 'nnhip_strain_tan_geom',
             'nnhip_strain_born')
    L = hip.lib()
    for name in names:
        assert name in abi.FUNCTIONS and name in hip.EXPORTED_SYMBOLS and hasattr(L, name), name
    OK, E_INVALID, E_UNSUPPORTED = 0, 1, 2
    p = 0x7f0000001000                        # stands for any device array
    assert abi.CONSTANTS['NNHIP_MAX_NB'] == H.MAX_NB and abi.CONSTANTS['NNHIP_MAX_LAYERS'] == H.MAX_LAYERS
    assert abi.CONSTANTS['NNHIP_ENVELOPE_COSINE'] == H.ENV_COSINE

    def refused(rc, who, needle, code=E_INVALID):
        assert rc == code, (who, rc)
        msg = L.nnhip_last_error().decode()
        assert msg.startswith(who) and needle in msg, msg
    dgu = lambda n=5, gf=p, out=p: L.nnhip_hvp_dgu(gf, p, p, p, p, p, None, n, out, None)  # noqa: E731
    refused(dgu(n=-1), 'nnhip_hvp_dgu', 'n_atoms >= 0')
    refused(dgu(gf=None), 'nnhip_hvp_dgu', 'gf')
    refused(dgu(out=None), 'nnhip_hvp_dgu', 'dg_u')
    assert dgu(n=0, gf=None, out=None) == OK
    dgx = lambda nb=20, env=9, rc=5.0, n=8, w=p: L.nnhip_hvp_dgx(p, p, p, p, None, p, p, w, p, nb, env, rc, n, p, None)  # noqa: E731
    for nb in (0, 33, -1):
        refused(dgx(nb=nb), 'nnhip_hvp_dgx', 'n_basis', E_UNSUPPORTED)
    refused(dgx(rc=0.0), 'nnhip_hvp_dgx', 'cutoff > 0.f')
    refused(dgx(n=-1), 'nnhip_hvp_dgx', 'n_edges >= 0')
    refused(dgx(env=-2), 'nnhip_hvp_dgx', 'envelope')
    refused(dgx(w=None), 'nnhip_hvp_dgx', 'edge_w')
    assert dgx(n=0) == OK
    out = lambda n=4, e=8, layers=3, rc=5.0, hv=p: L.nnhip_hvp_out(p, p, p, p, p, p, p, p, n, e, layers, rc, p, hv, None)  # noqa: E731
    for layers in (0, 9, -1):
        refused(out(layers=layers), 'nnhip_hvp_out', 'n_layers')
    refused(out(rc=-1.0), 'nnhip_hvp_out', 'cutoff > 0.f')
    refused(out(n=0), 'nnhip_hvp_out', 'n_atoms > 0')
    refused(out(hv=None), 'nnhip_hvp_out', 'hv')
    assert out(n=0, e=0) == OK
    dirs = lambda n=4, k=0, rep=1, mol0=1: L.nnhip_hess_dirs(p, p, n, k, rep, mol0, p, None)  # noqa: E731
    scat = lambda n=4, k=0, rep=1, mol0=1: L.nnhip_hess_scatter(p, p, p, p, n, k, rep, mol0, p, None)  # noqa: E731
    for f, who in ((dirs, 'nnhip_hess_dirs'), (scat, 'nnhip_hess_scatter')):
        refused(f(n=-1), who, 'n_atoms >= 0')
        refused(f(k=-1), who, 'k >= 0')
        refused(f(rep=0), who, 'n_rep >= 1')
        refused(f(mol0=0), who, 'n_mol0 >= 1')
        assert f(n=0) == OK
    refused(L.nnhip_strain_tan_geom(p, p, p, p, 8, 0.0, p, None), 'nnhip_strain_tan_geom', 'cutoff > 0.f')
    refused(L.nnhip_strain_tan_geom(p, None, p, p, 8, 5.0, p, None), 'nnhip_strain_tan_geom', 'batch')
    assert L.nnhip_strain_tan_geom(None, None, None, None, 0, 5.0, None, None) == OK
    refused(L.nnhip_strain_born(p, p, p, p, -1, p, None), 'nnhip_strain_born', 'n_mol >= 0')
    refused(L.nnhip_strain_born(p, p, p, None, 3, p, None), 'nnhip_strain_born', 'mol_ptr')
    assert L.nnhip_strain_born(None, None, None, None, 0, None, None) == OK
