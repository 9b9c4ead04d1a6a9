"""The float64 references of tests/dense_ref.py checked against torch.autograd / torch.optim / torch.nn in float64: what the
kernel tests (tests/test_hip_dense_stages.py) compare the HIP kernels with must itself be right.  No GPU."""
import numpy as np
import pytest
import torch

from tests import dense_ref as R

TORCH_ACT = {
    'silu': torch.nn.functional.silu, 'relu': torch.relu, 'elu': torch.nn.functional.elu,
    'leaky_relu': torch.nn.functional.leaky_relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid,
    'softplus': torch.nn.functional.softplus, 'gelu': torch.nn.functional.gelu,
    'ssp': lambda x: torch.nn.functional.softplus(x) - np.log(2.0),
}


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


@pytest.mark.parametrize('name', R.ACTIVATIONS)
def test_activation_derivatives(name):
    x = torch.linspace(-6, 6, 241, dtype=torch.float64)
    x = x[x != 0].clone().requires_grad_(True)        # (the kinks of relu / leaky_relu / elu are not differentiated at 0)
    y = TORCH_ACT[name](x)
    d1, = torch.autograd.grad(y.sum(), x, create_graph=True)
    _close(R.act(name, x.detach().numpy()), y.detach().numpy())
    _close(R.dact(name, x.detach().numpy()), d1.detach().numpy())
    d2 = torch.autograd.grad(d1.sum(), x, allow_unused=True)[0] if d1.requires_grad else None
    _close(R.d2act(name, x.detach().numpy()), np.zeros(x.shape) if d2 is None else d2.numpy())


@pytest.mark.parametrize('name', R.ACTIVATIONS)
def test_mlp_modes_are_the_derivatives_of_forward(name):
    """BWD = the vector-Jacobian product of FWD, TAN = its Jacobian-vector product, TAN2 = the Jacobian-vector product of BWD."""
    M = 7
    X, W1, W2 = _rand(1, M, 128), _rand(2, 128, 128) / 11, _rand(3, 128, 128) / 11
    b1, b2 = _rand(4, 128), _rand(5, 128)
    act = TORCH_ACT[name]
    fwd = lambda x: act(x @ W1.T + b1) @ W2.T + b2  # noqa: E731
    out = R.mlp(R.MODE_FWD, X.numpy(), W1.numpy(), W2.numpy(), name, b1=b1.numpy(), b2=b2.numpy())
    H = X @ W1.T + b1
    _close(out['H'][0], H.numpy())
    _close(out['Y'][0], fwd(X).numpy())
    # BWD: the adjoint runs with the transposed weights swapped (X = gY, W1 = W2^T, W2 = W1^T): gX = ((gY W2) act'(H)) W1
    gY, Y0 = _rand(6, M, 128), _rand(7, M, 128)
    Xr = X.clone().requires_grad_(True)
    vjp, = torch.autograd.grad(fwd(Xr), Xr, gY)
    W1a, W2a = W2.T.contiguous().numpy(), W1.T.contiguous().numpy()
    out = R.mlp(R.MODE_BWD, gY.numpy(), W1a, W2a, name, H=H.numpy())
    _close(out['Y'][0], vjp.numpy())
    out = R.mlp(R.MODE_BWD, gY.numpy(), W1a, W2a, name, H=H.numpy(), Y0=Y0.numpy())
    _close(out['Y'][0], (vjp + Y0).numpy())
    # TAN: the tangent of FWD along dX (T = dH, Y = dY)
    dX = _rand(8, M, 128)
    _, jvp = torch.autograd.functional.jvp(fwd, X, dX)
    out = R.mlp(R.MODE_TAN, dX.numpy(), W1.numpy(), W2.numpy(), name, H=H.numpy())
    _close(out['T'][0], (dX @ W1.T).numpy())
    _close(out['Y'][0], jvp.numpy())
    # TAN2: the tangent of BWD (as a function of gY and H) along (dgY, Hd); T2 = gY W2 is BWD's own hidden product
    dgY, Hd = _rand(9, M, 128), _rand(10, M, 128)

    def bwd_fn(g, h):      # act' through autograd, so that jvp differentiates it once more
        da, = torch.autograd.grad(act(h).sum(), h, create_graph=True)
        return ((g @ W2) * da) @ W1
    _, jvp2 = torch.autograd.functional.jvp(bwd_fn, (gY, H.detach()), (dgY, Hd))
    T2 = (gY @ W2).numpy()
    out = R.mlp(R.MODE_TAN2, dgY.numpy(), W1a, W2a, name, H=H.numpy(), T2=T2, Hd=Hd.numpy())
    _close(out['Y'][0], jvp2.numpy())
    G = (dgY @ W2) * torch.as_tensor(R.dact(name, H.numpy())) + (gY @ W2) * torch.as_tensor(R.d2act(name, H.numpy())) * Hd
    _close(out['G'][0], G.numpy())


def test_product_bound_holds_for_fp32_and_rounded_operands():
    """the bound really bounds: an fp32 product chain, and operands rounded to bf16 / to 22 bits of the row maximum"""
    A, W = _rand(11, 33, 128).float(), (_rand(12, 128, 128) / 11).float()
    C, B = R.product(A.numpy(), W.numpy(), R.FP32)
    got = (A @ W.T).double().numpy()                     # an fp32 chain of 128 products
    assert (np.abs(got - C) <= B).all() and (B < 2e-5 * np.abs(A.double().numpy()) @ np.abs(W.double().numpy()).T).all()
    C, B = R.product(A.numpy(), W.numpy(), R.BF16)
    got = (A.bfloat16().double() @ W.bfloat16().double().T).numpy()
    assert (np.abs(got - C) <= B).all()
    C, B = R.product(A.numpy(), W.numpy(), R.SPLIT)
    q = lambda t, s: torch.round(t.double() / s * 2 ** 22) / 2 ** 22 * s  # noqa: E731
    got = (q(A, A.abs().amax(1, keepdim=True).double()) @ q(W, W.abs().max().double()).T).numpy()
    assert (np.abs(got - C) <= B).all()
    # a dropped k-term is far outside the bound
    Cd = A[:, :127].double().numpy() @ W[:, :127].double().numpy().T
    assert (np.abs(Cd - R.product(A.numpy(), W.numpy(), R.FP32)[0]) > R.product(A.numpy(), W.numpy(), R.FP32)[1]).mean() > 0.99


@pytest.mark.parametrize('name', ('silu', 'tanh', 'ssp'))
@pytest.mark.parametrize('typ,two', [(0, False), (0, True), (1, False), (1, True), (2, False), (2, True)])
def test_weight_gradient_types(typ, two, name):
    """types 0, 1, 2 = torch.autograd.grad of the two-layer expression each one differentiates"""
    M = 19
    act = TORCH_ACT[name]
    A1, A2 = _rand(20, M, 128), _rand(21, M, 128)
    Wt = torch.zeros(128, 128, dtype=torch.float64, requires_grad=True)
    if typ == 0:
        B1, B2 = _rand(22, M, 128), _rand(23, M, 128)
        expr = (A1 * (B1 @ Wt.T)).sum() + ((A2 * (B2 @ Wt.T)).sum() if two else 0.0)
        got, _ = R.wgrad(0, A1.numpy(), B1.numpy(), A2.numpy() if two else None, B2.numpy() if two else None)
    elif typ == 1:   # d/dW of sum A1 (act(h) W^T) [+ the tangent term A2 ((act'(h) dh) W^T)]
        hB, dhB = _rand(24, M, 128), _rand(25, M, 128)
        hr = hB.clone().requires_grad_(True)
        a = act(hr)
        expr = (A1 * (a @ Wt.T)).sum()
        if two:
            da, = torch.autograd.grad(a.sum(), hr, create_graph=True)
            expr = expr + (A2 * ((da * dhB).detach() @ Wt.T)).sum()
        got, _ = R.wgrad(1, A1.numpy(), None, A2.numpy() if two else None, None, hB=hB.numpy(), dhB=dhB.numpy() if two else None,
                         activation=name)
    else:            # d/dW of sum A1 (B1 W^T) + (A2 act'(hA)) (B2 W^T)
        B1, B2, hA = _rand(26, M, 128), _rand(27, M, 128), _rand(28, M, 128)
        hr = hA.clone().requires_grad_(True)
        da, = torch.autograd.grad(act(hr).sum(), hr)
        expr = (A1 * (B1 @ Wt.T)).sum() + (((A2 * da) * (B2 @ Wt.T)).sum() if two else 0.0)
        got, _ = R.wgrad(2, A1.numpy(), B1.numpy(), A2.numpy() if two else None, B2.numpy() if two else None,
                         hA=hA.numpy() if two else None, activation=name)
    want, = torch.autograd.grad(expr, Wt)
    _close(got, want.numpy())


def test_reductions():
    x = _rand(30, 301, 128)
    s, B = R.colsum(x.numpy())
    _close(s, x.sum(0).numpy())
    assert (np.abs(x.float().sum(0).double().numpy() - s) <= B).all()
    z = torch.tensor([0, 1, 6, 7, 8, 118])[torch.randint(0, 6, (301,), generator=torch.Generator().manual_seed(31))]
    out, B = R.species_sum(x.numpy(), z.numpy(), 3, 40)
    want = torch.zeros(119, 40, dtype=torch.float64).index_add_(0, z, x[:, 3:43])
    _close(out, want.numpy())
    assert not out[[2, 3, 4, 5, 9, 117]].any() and not B[[2, 3, 4, 5, 9, 117]].any()


def _species_fp32(x, z, c_total):
    """nnhip_species_sum's summation order (csrc/train.hip) in fp32 on the host: (table [119][width], total)"""
    f = np.float32
    n, width = x.shape
    chunks, per = R.species_layout(n)
    if not chunks:                                   # species_direct_kernel: two waves list strided halves, lists added in order
        out = np.zeros((R.N_ELEMENTS, width), f)
        for zz in np.unique(z):
            idx = np.flatnonzero(z == zz)
            for w in (0, 1):
                for i in idx[(idx // 64) % 2 == w]:
                    out[zz] += x[i]
        sh = np.zeros(128, f)
        for i in range(n):
            sh[i % 128] += x[i, c_total]
        o = 64
        while o:
            sh[:o] += sh[o:2 * o]
            o //= 2
        return out, sh[0]
    part = np.zeros((chunks, R.N_ELEMENTS, width), f)
    for i in range(n):
        part[i // per, z[i]] += x[i]
    grp = np.zeros((8, R.N_ELEMENTS, width), f)
    for k in range(chunks):
        grp[k % 8] += part[k]
    out = grp[0].copy()
    for q in range(1, 8):
        out += grp[q]
    flat = part[:, :, c_total].ravel()
    sh = np.zeros(1024, f)
    for k in range(flat.size):
        sh[k % 1024] += flat[k]
    o = 512
    while o:
        sh[:o] += sh[o:2 * o]
        o //= 2
    return out, sh[0]


@pytest.mark.parametrize('n', (129, 1024, 1025, 16385))
def test_species_bounds_hold_for_the_kernels_summation_order(n):
    """the kernels' order of additions in fp32 stays inside species_sum's / species_total's bounds in both layouts, and a
    dropped atom does not"""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 5), dtype=np.float32)
    z = np.array([0, 1, 6, 7, 8, 118])[rng.integers(0, 6, n)]
    assert R.species_layout(n) == {129: (0, 0), 1024: (0, 0), 1025: (17, 61), 16385: (256, 65)}[n]
    got, tot = _species_fp32(x, z, 4)
    ref, B = R.species_sum(x, z, 0, 5)
    assert (np.abs(got - ref) <= B).all()
    t_ref, t_B = R.species_total(x[:, 4], z)
    assert abs(float(tot) - t_ref) <= t_B
    assert abs(float(tot) - t_ref) > 0 or n < 1024
    i = int(np.abs(x).min(axis=1).argmax())                          # an atom of ordinary size in every column, dropped
    keep = np.arange(n) != i
    ref1, _ = R.species_sum(x[keep], z[keep], 0, 5)
    assert (np.abs(ref1 - ref)[z[i]] > 10 * B[z[i]]).all() and abs(x[keep, 4].astype(np.float64).sum() - t_ref) > 10 * t_B


@pytest.mark.parametrize('mode_e', (0, 1, 2))
@pytest.mark.parametrize('mode_f', (0, 1, 2))
def test_losses(mode_e, mode_f):
    """nn.MSELoss / nn.L1Loss / nn.HuberLoss(delta), mean reduction, with residuals exactly at 0 and +-delta"""
    de_, df_ = 0.5, 0.25
    mk = lambda m, d: (torch.nn.MSELoss(), torch.nn.L1Loss(), torch.nn.HuberLoss(delta=d))[m]  # noqa: E731
    e_lab, f_lab = _rand(40, 9).float(), _rand(41, 30).float()
    re, rf = _rand(42, 9).float(), _rand(43, 30).float()
    re[:3], rf[:3] = torch.tensor([0.0, de_, -de_]), torch.tensor([0.0, df_, -df_])
    e, f = (e_lab + re), (f_lab + rf)
    re, rf = (e - e_lab), (f - f_lab)                   # the fp32 residuals as formed
    er, fr = e.double().requires_grad_(True), f.double().requires_grad_(True)
    w_e, w_f = 1.0, 50.0
    # (labels shifted so that the float64 residual equals the fp32 one exactly: the elements at 0 / +-delta stay there)
    loss = w_e * mk(mode_e, de_)(er, e.double() - re.double()) + w_f * mk(mode_f, df_)(fr, f.double() - rf.double())
    ge, gf = torch.autograd.grad(loss, (er, fr))
    got = R.loss_grad(e.numpy(), e_lab.numpy(), f.numpy(), f_lab.numpy(), (w_e / 9, w_f / 30), mode_e, mode_f, de_, df_)
    _close(got[0], loss.item())
    _close(got[2], ge.numpy())
    _close(got[3], gf.numpy())


@pytest.mark.parametrize('max_norm', (0.5, 1e6, 0.0))
def test_clip_adam_against_torch(max_norm):
    n = 1000
    p0, g_all = _rand(50, n), _rand(51, 5, n)
    prm = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([prm], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    p, m, v = p0.numpy(), np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        prm.grad = g_all[t - 1].clone()
        want_norm = prm.grad.norm().item()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([prm], max_norm)
        opt.step()
        p, m, v, norm = R.clip_adam_step(p, g_all[t - 1].numpy(), m, v, t, 1e-3, 0.9, 0.999, 1e-8, max_norm)
        _close(norm, want_norm)
        _close(p, prm.detach().numpy())
        _close(m, opt.state[prm]['exp_avg'].numpy())
        _close(v, opt.state[prm]['exp_avg_sq'].numpy())
    # frozen elements: out of the norm, never updated
    mask = (np.arange(n) % 3 != 0).astype(np.uint8)
    p2, m2, v2, norm = R.clip_adam_step(p0.numpy(), g_all[0].numpy(), np.zeros(n), np.zeros(n), 1, 1e-3, 0.9, 0.999, 1e-8, 0.5, mask)
    assert (p2[mask == 0] == p0.numpy()[mask == 0]).all() and not m2[mask == 0].any()
    _close(norm, g_all[0][torch.as_tensor(mask != 0)].norm().item())
