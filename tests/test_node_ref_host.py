"""tests/node_ref.py on the CPU: what tests/test_edge_ref_host.py is to tests/edge_ref.py.

  1. derivative structure: every *_bwd statement is the vector-Jacobian product of its forward statement and every tangent
     statement the Jacobian-vector product, by torch float64 autograd, to 1e-11 of the array's largest element;
  2. chained over the layers of one small molecule the statements reproduce tests/trace.py and tests/tangent_ref.py;
  3. the fp32 numpy restatement of each kernel's own order of operations (node_ref.restate_*: for the image kernels the power-of-two
     row and matrix scales, the hi + lo f16 split, the three partial products and fp32 accumulation; for the others the wave sums
     over two features per lane) stays inside the bound on every case of the kernel tests -- the worst ratio per stage is printed;
  4. each wrong kernel of MUTATIONS leaves the bound by more than 10 x somewhere in every output it changes."""
import numpy as np
import pytest
import torch

from tests import dense_ref as D
from tests import node_ref as R

F = R.F
f64 = torch.float64


def T(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def close(got, want, what, tol=1e-11):
    got, want = np.asarray(got, np.float64), np.asarray(want.detach().numpy() if torch.is_tensor(want) else want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(np.abs(want).max(), 1e-300)
    assert np.abs(got - want).max() <= tol * scale, f'{what}: {np.abs(got - want).max() / scale:.3e}'


def tact(name, x):
    if name == 'silu':
        return torch.nn.functional.silu(x)
    return {'tanh': torch.tanh, 'softplus': torch.nn.functional.softplus, 'gelu': torch.nn.functional.gelu,
            'sigmoid': torch.sigmoid, 'elu': torch.nn.functional.elu}[name](x)


def fwd_torch(f, a_mid, t, act):
    Wu, W0, W2 = T(t['Wu']), T(t['W0']), T(t['W2'])
    q = f @ Wu.T
    a = a_mid + (f * q).sum(1)
    hn = a @ W0.T + T(t['b0'])
    return q, a, hn, tact(act, hn) @ W2.T + T(t['b2'])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. derivative structure
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ('silu', 'tanh', 'gelu', 'softplus'))
def test_node_statements_are_the_derivatives_of_node_fwd(act):
    n = 5
    t = R.node_inputs(n)
    f, a_mid = T(t['f']).requires_grad_(True), T(t['a_mid']).requires_grad_(True)
    q, a, hn, m = fwd_torch(f, a_mid, t, act)
    fw = R.ref_node_fwd(t, act, R.FP32)
    for k, v in (('q', q), ('a_out', a), ('hn', hn), ('m', m)):
        close(fw[k][0], v, k)
    # node_bwd = VJP: cotangents g_top on m, g_a on a_out, G_f on f
    L = (m * T(t['g_top'])).sum() + (a * T(t['g_a'])).sum() + (f * T(t['G_f'])).sum()
    gf, ga = torch.autograd.grad(L, (f, a_mid))
    tt = dict(t, h_top=hn.detach().numpy(), q=q.detach().numpy())
    for form in (R.FP32, R.SPLIT):
        bw = R.ref_node_bwd(tt, act, form, mlp=True, upd=True, acc=1, G_f=True, T=True)
        close(bw['g_a'][0], ga, 'g_a')
        close(bw['gf'][0], gf, 'gf')
        close(bw['T'][0], T(t['g_top']) @ T(t['W2']), 'T')
        close(R.ref_node_bwd(tt, act, form, mlp=True, upd=True, acc=1, G_f=True, recompute=True)['gf'][0], gf, 'gf (q formed again)')
        other = R.ref_node_bwd(tt, act, form, mlp=True, upd=False, acc=1, g_a_in='other')
        close(other['g_a'][0], ga - T(t['g_a']) + T(t['g_a_in']), 'g_a from g_a_in')
        assert not other['gf'][2].any() and not other['T'][2].any()
        upd = R.ref_node_bwd(dict(tt, g_a=ga.numpy()), act, form, mlp=False, upd=True, G_f=True)
        close(upd['gf'][0], gf, 'gf (update part alone)')
    if act != 'silu':
        return
    # node_tan_fwd = JVP in the direction (df, da_mid)
    _, (dq, da, dhn, dm) = torch.autograd.functional.jvp(lambda x, y: fwd_torch(x, y, t, act), (f.detach(), a_mid.detach()),
                                                         (T(t['df']), T(t['da_mid'])))
    tf = R.ref_node_tan_fwd(dict(tt, hn=hn.detach().numpy()))
    for k, v in (('dq', dq), ('da_out', da), ('T', dhn), ('Y', dm)):
        close(tf[k][0], v, 'tan_fwd ' + k)
    # node_tan_bwd = JVP of node_bwd: part A in (g_top, h_top), part B in (g_a, f, q)
    W2, W0, Wu = T(t['W2']), T(t['W0']), T(t['Wu'])

    def part_a(g, h):
        ghn = (g @ W2) * torch.autograd.grad(tact(act, h).sum(), h, create_graph=True)[0]
        return ghn, ghn @ W0

    h0 = hn.detach().requires_grad_(True)
    _, (G, dga) = torch.autograd.functional.jvp(part_a, (T(t['g_a']), h0), (T(t['g_top']), T(t['hd_top'])), create_graph=True)
    ta = dict(tt, t2_top=(T(t['g_a']) @ W2).numpy())            # t2 = the value sweep's hidden product of the point (g_a, h)
    A = R.ref_node_tan_bwd(ta, A=True, B=False, acc=1)
    close(A['G'][0], G.detach(), 'tan_bwd G')
    close(A['dga'][0], dga.detach() + T(t['dga']), 'tan_bwd dga')
    close(R.ref_node_tan_bwd(ta, A=True, B=False, t2=False)['G'][0], (T(t['g_top']) @ W2) * T(D.dact(act, tt['h_top'])), 'G, no t2')

    def part_b(gav, fv, qv):
        return gav.unsqueeze(1) * fv, gav.unsqueeze(1) * qv + (gav.unsqueeze(1) * fv) @ Wu

    (gq, _), (dgq, dgf) = torch.autograd.functional.jvp(part_b, (T(t['ga']), f.detach(), q.detach()), (T(t['dga']), T(t['df']), T(t['dq'])))
    B = R.ref_node_tan_bwd(tt, A=False, B=True, dgf_in=True)
    close(B['gq'][0], gq, 'gq')
    close(B['dgq'][0], dgq, 'dgq')
    close(B['dgf'][0], dgf + T(t['dgf_in']), 'dgf')
    ub = R.update_tan_bwd(t['ga'], t['dga'], t['f'], t['df'], tt['q'], t['dq'], t['dgf_in'])
    close(ub['dgf'][0] + (ub['dgq'][0] @ t['WuT'].astype(np.float64).T), dgf + T(t['dgf_in']), 'update_tan_bwd + the linear')
    close(ub['gq'][0], gq, 'update gq')
    close(R.update_tan_fwd(t['da_mid'], t['f'], t['df'], tt['q'], dq.numpy())['da_out'][0], da, 'update_tan_fwd')


def test_direct_force_adjoint_is_the_gradient_of_the_tail():
    t = R.direct_force_inputs(5)
    d, f = T(t['d']).requires_grad_(True), T(t['f']).requires_grad_(True)
    sc = T(t['scale'])[torch.from_numpy(t['z'])]
    raw = torch.einsum('if,ikf->ik', d, f)
    out = raw * sc[:, None]
    close(R.direct_force_tail(t['d'], t['f'], t['scale'], t['z'])['out'][0], out, 'out')
    gd, gf = torch.autograd.grad((out * T(t['g_out'])).sum(), (d, f))
    adj = R.direct_force_adj(t['g_out'], t['d'], t['f'], t['scale'], t['z'])
    close(adj['g_d3'][0], gd, 'g_d3')
    close(adj['seed_f'][0], gf, 'seed_f')
    close(adj['sc4'][0][:, 0], (raw.detach() * T(t['g_out'])).sum(1), 'dL/dscale rows')      # d out / d scale = raw


@pytest.mark.parametrize('scale,shift', ((True, True), (False, False)))
def test_node_turn_is_the_head_and_its_gradient(scale, shift):
    n = 9
    t = R.node_inputs(n)
    f, a_mid = T(t['f']).requires_grad_(True), T(t['a_mid']).requires_grad_(True)
    _, a, _, e2 = fwd_torch(f, a_mid, t, 'silu')
    z = torch.from_numpy(t['z'])
    sc = T(t['scale'])[z] if scale else 1.0
    sh = T(t['shift'])[z] if shift else 0.0
    ae = (torch.nn.functional.silu(e2) @ T(t['w4']) + float(t['b4'][0])) * sc + sh
    gf, ga = torch.autograd.grad(ae.sum(), (f, a_mid))
    out = R.ref_node_turn(t, scale=scale, shift=shift)
    for k, v in (('a_out', a), ('atom_energy', ae), ('g_a', ga), ('gf', gf)):
        close(out[k][0], v, k)


def ln_torch(x, t):
    y = torch.nn.functional.layer_norm(x, (F,), T(t['gamma']), T(t['beta']), eps=R.EPS)
    rs = 1.0 / torch.sqrt(x.var(dim=1, unbiased=False) + R.EPS)
    return y, (x - x.mean(1, keepdim=True)) * rs[:, None], rs


@pytest.mark.parametrize('edge', [e for e in R.LN_EDGES if e != 'offset row'])     # (autograd itself loses the offset row's digits)
def test_layer_norm_statements_are_the_derivatives_of_layer_norm(edge):
    t = R.ln_inputs(5, edge)
    x = T(t['x']).requires_grad_(True)
    y, xh, rs = ln_torch(x, t)
    fw = R.layer_norm_fwd(t['x'], t['gamma'], t['beta'])
    for k, v in (('y', y), ('xhat', xh), ('rstd', rs)):
        close(fw[k][0], v, k, 1e-11)
    e = dict(t, xhat=xh.detach().numpy(), rstd=rs.detach().numpy())
    gx, = torch.autograd.grad((y * T(t['g'])).sum(), x)
    close(R.ref_ln('layer_norm_bwd', e)['g_x'][0], gx, 'g_x', 1e-11)
    _, (dy, dxh, drs) = torch.autograd.functional.jvp(lambda v: ln_torch(v, t), x.detach(), T(t['dx']))
    tf = R.ref_ln('layer_norm_tan_fwd', e)
    for k, v in (('dy', dy), ('dxhat', dxh), ('drstd', drs)):
        close(tf[k][0], v, k, 1e-11)
    e.update(dxhat=dxh.numpy(), drstd=drs.numpy())

    def adjoint(gy, xhv, rv):
        gp = gy * T(t['gamma'])
        return rv[:, None] * (gp - gp.mean(1, keepdim=True) - xhv * (gp * xhv).mean(1, keepdim=True))

    _, dgx = torch.autograd.functional.jvp(adjoint, (T(t['gy']), xh.detach(), rs.detach()), (T(t['dgy']), dxh, drs))
    tb = R.ref_ln('layer_norm_tan_bwd', e)
    close(tb['dg_x'][0], dgx, 'dg_x', 1e-11)
    close(tb['row_w'][0], T(t['dgy']) * xh.detach() + T(t['gy']) * dxh, 'row_w')
    close(tb['row_b'][0], T(t['dgy']), 'row_b')


# ---------------------------------------------------------------------------------------------------------------------------
# 2. chained over the layers of one molecule
# ---------------------------------------------------------------------------------------------------------------------------
def _molecule():
    from tests import util
    z, pos, cell, batch, _ = util.case_inputs('ethanol4_rand')
    keep = batch == 0
    return util.load_state('rand'), z[keep], pos[keep], cell[:1], batch[keep]


def _mats(sd, l, L):
    """Wu of layer l and the MLP behind it: the next layer's message_nodepart, or the first two linears of the head"""
    p = f'interaction_layers.{l + 1}.message_nodepart.' if l + 1 < L else 'output_layers.0.layers.'
    w = {k: sd[p + k].numpy() for k in ('0.weight', '0.bias', '2.weight', '2.bias')}
    Wu = sd[f'interaction_layers.{l}.equiv_update.weight'].numpy()
    return dict(Wu=Wu, W0=w['0.weight'], b0=w['0.bias'], W2=w['2.weight'], b2=w['2.bias'], WuT=Wu.T, W0T=w['0.weight'].T, W2T=w['2.weight'].T)


def test_chained_statements_reproduce_the_trace():
    from tests import trace as TR
    sd, z, pos, cell, batch = _molecule()
    tr = TR.trace(sd, z, pos, cell, batch)
    L = 3
    for l in range(L):
        w = _mats(sd, l, L)
        t = dict(w, f=tr[f'f_out_{l}'].numpy(), a_mid=tr[f'a_mid_{l}'].numpy())
        fw = R.ref_node_fwd(t, 'silu', R.FP32)
        close(fw['q'][0], tr[f'q_{l}'], f'q {l}')
        close(fw['a_out'][0], tr[f'a_out_{l}'], f'a_out {l}')
        if l + 1 < L:
            close(fw['hn'][0], tr[f'hn_{l + 1}'], f'hn {l + 1}')
            close(fw['m'][0], tr[f'm_{l + 1}'], f'm {l + 1}')
            # dE/d a_out_l = what reaches it through a_mid_{l+1} (the running g_a) + the adjoint of message_nodepart
            t.update(g_top=tr[f'g_m_{l + 1}'].numpy(), h_top=tr[f'hn_{l + 1}'].numpy(), g_a=tr[f'g_a_mid_{l + 1}'].numpy())
            bw = R.ref_node_bwd(t, 'silu', R.SPLIT, mlp=True, upd=False, acc=1)
            close(bw['g_a'][0], tr[f'g_a_out_{l}'], f'g_a {l}', 1e-9)
    w = _mats(sd, L - 1, L)
    t = dict(w, f=tr[f'f_out_{L - 1}'].numpy(), a_mid=tr[f'a_mid_{L - 1}'].numpy(), z=z.numpy(),
             w4=sd['output_layers.0.layers.4.weight'].numpy().reshape(-1), b4=sd['output_layers.0.layers.4.bias'].numpy(),
             scale=sd['scalers.0.scale.weight'].numpy().reshape(-1), shift=sd['scalers.0.shift.weight'].numpy().reshape(-1))
    turn = R.ref_node_turn(t)
    close(turn['atom_energy'][0], tr['atom_energy'], 'atom_energy', 1e-9)
    close(turn['g_a'][0], tr[f'g_a_out_{L - 1}'], 'g_a of the last layer', 1e-9)
    close(turn['gf'][0], tr[f'g_f_out_{L - 1}'], 'gf of the last layer', 1e-9)
    # one layer down: the update adjoint with what comes from above = the total minus the update's own part
    l = L - 2
    w = _mats(sd, l, L)
    ga, f, q = tr[f'g_a_out_{l}'], tr[f'f_out_{l}'], tr[f'q_{l}']
    own = ga.unsqueeze(1) * q + (ga.unsqueeze(1) * f) @ sd[f'interaction_layers.{l}.equiv_update.weight']
    t = dict(w, g_a=ga.numpy(), f=f.numpy(), q=q.numpy(), G_f=(tr[f'g_f_out_{l}'] - own).numpy())
    close(R.ref_node_bwd(t, 'silu', R.FP32, mlp=False, upd=True, G_f=True)['gf'][0], tr[f'g_f_out_{l}'], f'gf {l}', 1e-9)


def test_chained_tangent_statements_reproduce_the_tangent_reference():
    from tests import tangent_ref as TG
    sd, z, pos, cell, batch = _molecule()
    gen = torch.Generator().manual_seed(5)
    g_energy, g_forces = torch.randn(1, generator=gen, dtype=f64), torch.randn(z.shape[0], 3, generator=gen, dtype=f64)
    _, _, _, S = TG.train_grads(sd, z, pos, cell, batch, g_energy, g_forces, keep=True)
    Ls, L = S['layers'], 3
    for l in range(L):
        st, w = Ls[l], _mats(sd, l, L)
        da_mid = st['da_out'] - (st['df_out'] * st['q'] + st['f_out'] * st['dq']).sum(1)
        hn = Ls[l + 1]['hn'] if l + 1 < L else S['e1']
        t = dict(w, df=st['df_out'].numpy(), f=st['f_out'].numpy(), q=st['q'].numpy(), da_mid=da_mid.numpy(), hn=hn.numpy())
        tf = R.ref_node_tan_fwd(t)
        close(tf['dq'][0], st['dq'], f'dq {l}', 1e-9)
        close(tf['da_out'][0], st['da_out'], f'da_out {l}', 1e-9)
        close(tf['T'][0], Ls[l + 1]['dhn'] if l + 1 < L else S['de1'], f'T {l}', 1e-9)
        close(tf['Y'][0], Ls[l + 1]['dm'] if l + 1 < L else S['de2'], f'Y {l}', 1e-9)
        close(R.update_tan_fwd(t['da_mid'], t['f'], t['df'], t['q'], st['dq'].numpy())['da_out'][0], st['da_out'], f'update_tan_fwd {l}', 1e-9)
    # the head's adjoint tangent and the last layer's update-adjoint tangent
    st, w = Ls[L - 1], _mats(sd, L - 1, L)
    t_e1 = S['g_e2'] @ sd['output_layers.0.layers.2.weight']
    t = dict(w, dga=np.zeros((z.shape[0], F)), g_top=S['dg_e2'].numpy(), h_top=S['e1'].numpy(), t2_top=t_e1.numpy(), hd_top=S['de1'].numpy(),
             ga=st['GA'].numpy(), f=st['f_out'].numpy(), df=st['df_out'].numpy(), q=st['q'].numpy(), dq=st['dq'].numpy())
    tb = R.ref_node_tan_bwd(t, A=True, B=True)
    close(tb['G'][0], S['dg_e1'], 'dg_e1', 1e-9)
    close(tb['dga'][0], S['dg_e1'] @ sd['output_layers.0.layers.0.weight'], 'dGA at the head', 1e-9)
    close(tb['dgf'][0], st['dgf'], 'dgf of the last layer', 1e-9)
    hs = R.head_seed_tan(S['e2'].numpy(), S['de2'].numpy(), sd['output_layers.0.layers.4.weight'].numpy().reshape(-1),
                         sd['output_layers.0.layers.4.bias'].numpy(), sd['scalers.0.scale.weight'].numpy().reshape(-1), z.numpy(),
                         batch.numpy(), g_energy.numpy())
    close(hs['dg_e2'][0], S['dg_e2'], 'dg_e2', 1e-9)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the fp32 restatements stay inside the bounds on every case of the kernel tests
# ---------------------------------------------------------------------------------------------------------------------------
def _ratios(ref, got, worst, key):
    for k, g in got.items():
        r = R.worst_ratio(g, ref[k])
        worst[key + (k,)] = max(worst.get(key + (k,), 0.0), r)


def test_fp32_restatements_stay_inside_the_bounds():
    worst, per_stage = {}, {}
    for stage, form, act, n, edge, name, v in R.node_cases():
        t = R.node_inputs(n, edge)
        got = R.node_restate(stage, form, act, t, v)
        for k, r in R.judge(stage, form, act, t, v, got, got.get('_stored')).items():
            worst[(stage, form, act, n, edge, name, k)] = r
    for n in R.WAVE_ROWS:
        for edge in R.LN_EDGES if n == 33 else ('plain',):
            t = R.ln_inputs(n, edge)
            for stage, fn in R.LN_STAGES.items():
                _ratios(R.ref_ln(stage, t), fn(t), worst, (stage, R.FP32, '', n, edge, ''))
        t = R.node_inputs(n)
        _ratios(R.update_tan_fwd(t['da_mid'], t['f'], t['df'], t['q'], t['dq']), R.restate_update_tan_fwd(t), worst,
                ('update_tan_fwd', R.FP32, '', n, 'plain', ''))
        for gin in (False, True):
            _ratios(R.update_tan_bwd(t['ga'], t['dga'], t['f'], t['df'], t['q'], t['dq'], t['dgf_in'] if gin else None),
                    R.restate_update_tan_bwd(t, gin), worst, ('update_tan_bwd', R.FP32, '', n, 'plain', f'dgf_in={int(gin)}'))
        for act in (D.ACTIVATIONS if n == 33 else ('silu',)):
            for sc in (True, False):
                t = R.head_seed_inputs(n)
                ref = R.head_seed_tan(t['e2'], t['de2'], t['w4'], t['b4'], t['scale'] if sc else None, t['z'], t['batch'], t['g_energy'], act)
                _ratios(ref, R.restate_head_seed_tan(t, act, sc), worst, ('head_seed_tan', R.FP32, act, n, 'plain', f'scale={int(sc)}'))
        t = R.direct_force_inputs(n)
        for sc in (True, False):
            _ratios(R.direct_force_tail(t['d'], t['f'], t['scale'] if sc else None, t['z']), R.restate_direct_force_tail(t, sc), worst,
                    ('direct_force tail', R.FP32, '', n, 'plain', f'scale={int(sc)}'))
            _ratios(R.direct_force_adj(t['g_out'], t['d'], t['f'], t['scale'] if sc else None, t['z']), R.restate_direct_force_adj(t, sc),
                    worst, ('direct_force_bwd tail', R.FP32, '', n, 'plain', f'scale={int(sc)}'))
    for key, r in worst.items():
        sk = key[:2]
        if r > per_stage.get(sk, (-1.0,))[0]:
            per_stage[sk] = (r, key)
    for (stage, form), (r, key) in sorted(per_stage.items()):
        print(f'RESTATED-RATIO {stage} [{form}]: {r:.3f} at {key[2:]}')
    bad = {k: r for k, r in worst.items() if not r <= 1.0}
    assert not bad, f'{len(bad)} outputs outside their bound, e.g. {sorted(bad.items(), key=lambda kv: -kv[1])[:5]}'


# ---------------------------------------------------------------------------------------------------------------------------
# 4. wrong kernels leave the bounds
# ---------------------------------------------------------------------------------------------------------------------------
NODE_MUT = {          # mutation -> (stage, variant dict, outputs that must change)
    'G_f dropped': [('node_bwd', R.BWD_VARIANTS['both G_f'], ('gf',))],
    'wrong q': [('node_fwd', R.FWD_VARIANTS['q=1 W0=1'], ('a_out', 'hn', 'm')), ('node_bwd', R.BWD_VARIANTS['both'], ('gf',)),
                ('node_turn', R.TURN_VARIANTS['scale=1 shift=1'], ('a_out', 'atom_energy', 'g_a', 'gf'))],
    "act' at the wrong place": [('node_bwd', R.BWD_VARIANTS['both'], ('g_a', 'gf'))],
    'acc_ga ignored': [('node_bwd', R.BWD_VARIANTS['both acc'], ('g_a', 'gf'))],
    'Wu transposed': [('node_fwd', R.FWD_VARIANTS['q=1 W0=1'], ('q', 'a_out', 'hn', 'm')), ('node_bwd', R.BWD_VARIANTS['both'], ('gf',))],
    'shift missing': [('node_turn', R.TURN_VARIANTS['scale=1 shift=1'], ('atom_energy',))],
    "act'' dropped": [('node_tan_bwd', R.TAN_BWD_VARIANTS['both'], ('G', 'dga', 'dgq', 'dgf'))],
    'last row': [('node_fwd', R.FWD_VARIANTS['q=1 W0=1'], ('q', 'a_out', 'hn', 'm')), ('node_bwd', R.BWD_VARIANTS['both'], ('g_a', 'gf')),
                 ('node_turn', R.TURN_VARIANTS['scale=1 shift=1'], ('a_out', 'atom_energy', 'g_a', 'gf')),
                 ('node_tan_fwd', {}, ('dq', 'da_out', 'T', 'Y')), ('node_tan_bwd', R.TAN_BWD_VARIANTS['both'], ('G', 'dga', 'gq', 'dgq', 'dgf'))],
}
LN_MUT = {'eps missing': ('layer_norm_fwd', ('y', 'xhat', 'rstd')), "mean(g') dropped": ('layer_norm_bwd', ('g_x',)),
          'last row': ('layer_norm_fwd', ('y', 'xhat', 'rstd'))}
MUTATIONS = tuple(NODE_MUT) + tuple(k for k in LN_MUT if k not in NODE_MUT)


def _changed(right, wrong):
    return {k for k in right if not np.array_equal(np.asarray(right[k]).view(np.int32), np.asarray(wrong[k], np.float32).view(np.int32))}


@pytest.mark.parametrize('mut', MUTATIONS)
def test_wrong_kernels_leave_the_bounds(mut):
    for stage, v, must in NODE_MUT.get(mut, ()):
        for form in ((R.SPLIT, R.FP32) if stage in ('node_fwd', 'node_bwd') else (R.SPLIT,)):
            for n in (33, 97):
                t = R.node_inputs(n)
                right, wrong = R.node_restate(stage, form, 'silu', t, v), R.node_restate(stage, form, 'silu', t, v, mut=mut)
                stored = right.pop('_stored', None)                   # node_turn: what the (right) three-launch composition stores
                wrong.pop('_stored', None)
                changed = _changed(right, wrong)
                assert set(must) <= changed, (mut, stage, form, n, must, changed)
                ratios = R.judge(stage, form, 'silu', t, v, wrong, stored)
                for k in changed:
                    r = ratios[k]
                    print(f'MUTATION {mut} | {stage} [{form}] N={n} | {k}: {r:.3g}')
                    assert r > 10.0, f'{mut}: {stage} [{form}] N={n} output {k} stays within {r:.3g} x its bound'
    if mut in LN_MUT:
        stage, must = LN_MUT[mut]
        best, seen = {}, set()
        for edge in R.LN_EDGES:
            t = R.ln_inputs(33, edge)
            ref, right, wrong = R.ref_ln(stage, t), R.LN_STAGES[stage](t), R.LN_STAGES[stage](t, mut=mut)
            for k in _changed(right, wrong):
                seen.add(k)
                best[k] = max(best.get(k, 0.0), R.worst_ratio(wrong[k], ref[k]))
        assert set(must) <= seen, (mut, must, seen)
        for k, r in best.items():
            print(f'MUTATION {mut} | {stage} | {k}: {r:.3g}')
            assert r > 10.0, f'{mut}: {stage} output {k} stays within {r:.3g} x its bound'
