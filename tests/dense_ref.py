"""Float64 statements of the dense and reduction stages the C interface exports one by one (include/newtonnet_hip.h:
nnhip_linear128, nnhip_mlp128_ex, nnhip_mlp128_pair_ex, nnhip_wgrad_batch, nnhip_colsum_batch, nnhip_species_sum,
nnhip_loss_grad, nnhip_clip_adam), each with a COMPONENTWISE error bound computed in float64 from the magnitudes, so that the
kernel tests (tests/test_hip_dense_stages.py) assert |got - ref| <= B element by element instead of a norm.

The bound of a product C = A . W^T summed over n terms, u = 2^-24:
    accumulation       (n + 2) u (|A| . |W|^T)                    (any summation order of n fp32 products)
    operand rounding   sum_k |a_k| dw_k + da_k |w_k| (+ da_k dw_k)    da / dw = what the product form does to its operands:
        FP32   none  (v_mfma_f32_32x32x2_f32)
        SPLIT  da = 2^-22 max|row of A|, dw = 2^-22 max|W|         csrc/mlp128s.hip:6-9,17-19 (hi + lo f16 pieces scaled by the
               row's / matrix's largest element; the dropped lo_a lo_b term is the da dw-sized third term, kept here as
               n 2^-22 max|row| max|W|)
        BF16   da = 2^-9 |a|, dw = 2^-9 |w|                        the bf16 compute mode of the MLPs (precision = 1): K = 128
               rounded operands per output
        BF16_RN da = 2^-8 |a|, dw = 2^-8 |w|                       bf16's unit roundoff: 8 significant bits, round to nearest
               (csrc/train.hip: pack_bf16, `(__bf16)lo`) can move ONE operand by up to 2^-8 relative -- 0.2528647 -> 0.251953 is
               3.6e-3.  A weight gradient over M = 1 row is a single product of two such operands: it reaches
               1.84 x the 2^-9 bound with a correctly rounding kernel, so nnhip_wgrad_batch's bf16_operands = 1 form is
               held to the format's own bound
        SPLIT3 da = 2^-24 |a|, dw = 2^-24 |w|                      ("24 significant bits", header at nnhip_wgrad_batch)
    input error        dA . |W|^T for an A that is itself a computed quantity with elementwise bound dA (chained products)
Elementwise factors evaluated on the device (act, act', act'') are fp32 evaluations of exp-based formulas; ACT_EVAL bounds
their absolute error by 4 u (1 + |x|)^2: the argument reduction of exp(-x) loses about |x| u relative, the sigmoid a few u more,
and the polynomial in x around it multiplies by up to (1 + |x|)."""
import numpy as np

U = 2.0 ** -24
FP32, SPLIT, BF16, BF16_RN, SPLIT3 = 'fp32', 'split-f16', 'bf16', 'bf16 unit roundoff', 'split-bf16x3'
ROW_TOL = 2e-6          # worst row of a device-activated output, fp32-grade forms (test_split_f16_products_are_fp32_grade)
ROW_TOL_BF16 = 2e-2     # the bf16 compute mode
ACTIVATIONS = ('silu', 'relu', 'elu', 'leaky_relu', 'tanh', 'sigmoid', 'softplus', 'gelu', 'ssp')
MODE_FWD, MODE_BWD, MODE_TAN, MODE_TAN2 = 0, 1, 2, 3


def _sig(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def _pdf(x):
    return np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def _cdf(x):
    from math import erf
    return 0.5 * (1.0 + np.vectorize(erf)(x / np.sqrt(2.0))) if np.size(x) else np.zeros_like(x)


def act(name, x):
    """the factory's activations (torch defaults: ELU alpha 1, LeakyReLU 0.01, Softplus beta 1, exact-erf GELU) in float64"""
    x = np.asarray(x, np.float64)
    if name in ('silu', 'swish'):
        return x * _sig(x)
    if name == 'relu':
        return np.maximum(x, 0.0)
    if name == 'elu':
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    if name == 'leaky_relu':
        return np.where(x > 0, x, 0.01 * x)
    if name == 'tanh':
        return np.tanh(x)
    if name == 'sigmoid':
        return _sig(x)
    if name in ('softplus', 'ssp'):
        return np.logaddexp(0.0, x) - (np.log(2.0) if name == 'ssp' else 0.0)
    if name == 'gelu':
        return x * _cdf(x)
    raise KeyError(name)


def dact(name, x):
    x = np.asarray(x, np.float64)
    if name in ('silu', 'swish'):
        s = _sig(x)
        return s * (1.0 + x * (1.0 - s))
    if name == 'relu':
        return (x > 0).astype(np.float64)
    if name == 'elu':
        return np.where(x > 0, 1.0, np.exp(np.minimum(x, 0.0)))
    if name == 'leaky_relu':
        return np.where(x > 0, 1.0, 0.01)
    if name == 'tanh':
        return 1.0 - np.tanh(x) ** 2
    if name == 'sigmoid':
        s = _sig(x)
        return s * (1.0 - s)
    if name in ('softplus', 'ssp'):
        return _sig(x)
    if name == 'gelu':
        return _cdf(x) + x * _pdf(x)
    raise KeyError(name)


def d2act(name, x):
    x = np.asarray(x, np.float64)
    if name in ('silu', 'swish'):
        s = _sig(x)
        return s * (1.0 - s) * (2.0 + x * (1.0 - 2.0 * s))
    if name in ('relu', 'leaky_relu'):
        return np.zeros_like(x)
    if name == 'elu':
        return np.where(x > 0, 0.0, np.exp(np.minimum(x, 0.0)))
    if name == 'tanh':
        t = np.tanh(x)
        return -2.0 * t * (1.0 - t * t)
    if name == 'sigmoid':
        s = _sig(x)
        return s * (1.0 - s) * (1.0 - 2.0 * s)
    if name in ('softplus', 'ssp'):
        s = _sig(x)
        return s * (1.0 - s)
    if name == 'gelu':
        return (2.0 - x * x) * _pdf(x)
    raise KeyError(name)


def act_eval_err(x):
    """absolute error bound of one fp32 evaluation of act / act' / act'' at x (module docstring)"""
    return 4.0 * U * (1.0 + np.abs(x)) ** 2


def operand_rounding(form, A, W):
    """(dA, dW): elementwise absolute bounds of what the product form does to its operands before multiplying"""
    A, W = np.abs(A), np.abs(W)
    if form == FP32:
        return np.zeros_like(A), np.zeros_like(W)
    if form == SPLIT:
        return (2.0 ** -22 * A.max(axis=1, keepdims=True) * np.ones_like(A) if A.size else np.zeros_like(A),
                2.0 ** -22 * (W.max() if W.size else 0.0) * np.ones_like(W))
    if form == BF16:
        return 2.0 ** -9 * A, 2.0 ** -9 * W
    if form == BF16_RN:
        return 2.0 ** -8 * A, 2.0 ** -8 * W
    if form == SPLIT3:
        return U * A, U * W
    raise KeyError(form)


def product(A, W, form=FP32, dA_in=None):
    """C = A . W^T in float64 and its componentwise bound.  A [M][K], W [N][K]; dA_in: elementwise bound of the error A itself
    carries (a computed operand).  n = K."""
    A, W = np.asarray(A, np.float64), np.asarray(W, np.float64)
    n = A.shape[1]
    aA, aW = np.abs(A), np.abs(W)
    dA, dW = operand_rounding(form, A, W)
    if dA_in is not None:
        aA = aA + dA_in                       # the device multiplies its own (perturbed) operand
        dA = dA + dA_in + (operand_rounding(form, dA_in, W)[0] if form != FP32 else 0.0)
    B = (n + 2) * U * (aA @ aW.T) + aA @ dW.T + dA @ aW.T + dA @ dW.T
    return A @ W.T, B


def linear128(A, W, bias=None, H=None, C0=None, prologue=0, epilogue=0, activation='silu'):
    """nnhip_linear128 (fp32 MFMA): C = epilogue(prologue(A) . W^T); prologue 1 = act(A); epilogue 1 + bias, 2 * act'(H), 3 C0 +"""
    A = np.asarray(A, np.float64)
    dA = None
    if prologue == 1:
        dA = act_eval_err(A)
        A = act(activation, A)
    C, B = product(A, W, FP32, dA)
    if epilogue == 1:
        C = C + bias
        B = B + U * np.abs(C)
    elif epilogue == 2:
        d = dact(activation, H)
        B = B * np.abs(d) + np.abs(C) * act_eval_err(H)
        C = C * d
        B = B + U * np.abs(C)
    elif epilogue == 3:
        C = C + C0
        B = B + U * np.abs(C)
    return C, B


def mlp(mode, X, W1, W2, activation='silu', form=FP32, H=None, b1=None, b2=None, T2=None, Hd=None, Y0=None, H_got=None,
        T_got=None, G_got=None):
    """nnhip_mlp128_ex in float64: dict of (value, bound) per output.
      FWD : 'H' = X W1^T + b1; 'Y' = act(H_got) W2^T + b2 with H_got the kernel's own stored H (the second product is judged
            alone; H_got None: the reference's H)
      BWD : 'Y' = Y0 + ((X W1^T) act'(H)) W2^T            TAN: the same and 'T' = X W1^T
      TAN2: 'G' = (X W1^T) act'(H) + T2 act''(H) Hd;  'Y' = Y0 + G W2^T
    T_got (TAN) / G_got (TAN2): the kernel's own stored hidden product; with it 'Y' is formed from what the kernel stored, so the
    second product is judged alone there too (the first one is judged by 'T' / 'G').  BWD stores nothing in between: its 'Y'
    carries the first product's bound through act' and |W2|."""
    X = np.asarray(X, np.float64)
    out = {}
    T, BT = product(X, W1, form)
    if mode == MODE_FWD:
        if b1 is not None:
            T = T + b1
            BT = BT + U * np.abs(T)
        out['H'] = (T, BT)
        Hs = T if H_got is None else np.asarray(H_got, np.float64)
        Y, BY = product(act(activation, Hs), W2, form, act_eval_err(Hs))
        if b2 is not None:
            Y = Y + b2
            BY = BY + U * np.abs(Y)
        out['Y'] = (Y, BY)
        return out
    H = np.asarray(H, np.float64)
    d1 = dact(activation, H)
    if mode == MODE_TAN:
        out['T'] = (T, BT)
    G = T * d1
    BG = BT * np.abs(d1) + np.abs(T) * act_eval_err(H) + U * np.abs(G)
    if mode == MODE_TAN2:
        d2 = d2act(activation, H)
        second = np.asarray(T2, np.float64) * d2 * np.asarray(Hd, np.float64)
        BG = BG + np.abs(np.asarray(T2, np.float64) * np.asarray(Hd, np.float64)) * act_eval_err(H) + 3 * U * np.abs(second)
        G = G + second
        BG = BG + U * np.abs(G)
        out['G'] = (G, BG)
    if mode == MODE_TAN and T_got is not None:
        Tg = np.asarray(T_got, np.float64)
        G = Tg * d1
        BG = np.abs(Tg) * act_eval_err(H) + U * np.abs(G)
    if mode == MODE_TAN2 and G_got is not None:
        G, BG = np.asarray(G_got, np.float64), None
    Y, BY = product(G, W2, form, BG)
    if Y0 is not None:
        Y = Y + Y0
        BY = BY + U * np.abs(Y)
    out['Y'] = (Y, BY)
    return out


def row_errors(got, ref):
    """||got_r - ref_r|| / ||ref_r|| per row, and min ||ref_r|| / median ||ref_r|| (the case must keep its rows away from zero)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nr = np.linalg.norm(ref, axis=1)
    rel = np.linalg.norm(got - ref, axis=1) / nr
    return rel, (nr.min() / np.median(nr) if nr.size else 1.0)


def wgrad(typ, A1, B1=None, A2=None, B2=None, hA=None, hB=None, dhB=None, activation='silu', form=FP32):
    """nnhip_wgrad_batch, one problem: dW[o][i] = sum_r A1[r][o] B1[r][i] + A2[r][o] B2[r][i] (n = M rows).
    type 1: B1 = act(hB), B2 = act'(hB) dhB; type 2: A2 = A2 act'(hA).  Returns (dW, bound)."""
    f = lambda t: None if t is None else np.asarray(t, np.float64)  # noqa: E731
    A1, B1, A2, B2, hA, hB, dhB = (f(t) for t in (A1, B1, A2, B2, hA, hB, dhB))
    dB1 = dB2 = dA2 = None
    if typ == 1:
        B1, dB1 = act(activation, hB), act_eval_err(hB)
        if A2 is not None:
            B2 = dact(activation, hB) * dhB
            dB2 = np.abs(dhB) * act_eval_err(hB) + U * np.abs(B2)
    elif typ == 2 and A2 is not None:
        A2s = A2 * dact(activation, hA)
        dA2 = np.abs(A2) * act_eval_err(hA) + U * np.abs(A2s)
        A2 = A2s
    M = A1.shape[0]

    def term(A, B, dA, dB):                 # sum over rows: A^T . B, the operands' own errors dA, dB
        aA, aB = np.abs(A) + (0 if dA is None else dA), np.abs(B) + (0 if dB is None else dB)
        rA, rB = operand_rounding(form, A.T, B.T)
        rA, rB = rA.T + (0 if dA is None else dA), rB.T + (0 if dB is None else dB)
        return A.T @ B, aA.T @ rB + rA.T @ aB + rA.T @ rB, aA.T @ aB
    V, Bd, mag = term(A1, B1, None, dB1)
    if A2 is not None:
        V2, Bd2, mag2 = term(A2, B2, dA2, dB2)
        V, Bd, mag = V + V2, Bd + Bd2, mag + mag2
    n = M * (2 if A2 is not None else 1)
    return V, Bd + (n + 2) * U * mag


def colsum(src):
    src = np.asarray(src, np.float64)
    return src.sum(axis=0), (src.shape[0] + 2) * U * np.abs(src).sum(axis=0)


N_ELEMENTS = 119


SP_DIRECT_MAX_ATOMS, SP_ATOMS, SP_CHUNKS = 1024, 64, 256      # csrc/train.hip: the layouts of nnhip_species_sum


def species_layout(n):
    """(chunks, atoms per chunk) of the two-pass form; (0, 0): the single launch serves n atoms"""
    if n <= SP_DIRECT_MAX_ATOMS:
        return 0, 0
    chunks = min(SP_CHUNKS, -(-n // SP_ATOMS))
    return chunks, -(-n // chunks)


def species_chains(z):
    """(n' per element, n' of the total): the largest number of fp32 additions of NON-ZERO terms any input passes through, read
    off the summation order of csrc/train.hip for this z (adding an exact zero rounds nothing).
      single launch: an element's list is added in order (its count); the total takes 128 strided sums and a 7-level tree.
      two passes: species_partial_kernel adds an element's atoms of one chunk in order (the largest count in a chunk);
        species_final_kernel: 8 groups walk the chunks 8 apart (the non-empty chunks of a group), then the 8 group sums;
        species_total_kernel: 1024 threads walk the chunks x elements table 1024 apart (the non-empty entries of a thread), then
        a 10-level tree."""
    z = np.asarray(z)
    n = z.shape[0]
    cnt = np.bincount(z, minlength=N_ELEMENTS).astype(np.float64)
    chunks, per = species_layout(n)
    if not chunks:
        return cnt, float(-(-n // 128) + 7)
    table = np.zeros((chunks, N_ELEMENTS))
    np.add.at(table, (np.arange(n) // per, z), 1.0)
    filled = table > 0
    groups = np.stack([filled[g::8].sum(axis=0) for g in range(8)])
    elem = table.max(axis=0) + groups.max(axis=0) + 8
    per_thread = np.bincount(np.flatnonzero(filled.ravel()) % 1024, minlength=1024)
    return elem, float(table.max() + per_thread.max() + 10)


def species_sum(x, z, c0, cols):
    """out[zz][0:cols] = sum_{i: z_i = zz} x[i][c0:c0+cols] and its bound (n' + 2) u sum |x| per element and column, n' from
    species_chains.  What is left between the errors seen and this bound at many atoms (ratios of 0.01 at 16 385) is the
    worst case itself: n' roundings of one sign, each relative to sum |x| where the partial sums of mixed signs are smaller
    by sqrt(count).  A dropped atom of ordinary size (|x_i| about 1) still moves the sum by about 100 times this bound at
    16 385 atoms and by more at fewer (tests/test_dense_ref_host.py)."""
    x, z = np.asarray(x, np.float64), np.asarray(z)
    out, mag = np.zeros((N_ELEMENTS, cols)), np.zeros((N_ELEMENTS, cols))
    np.add.at(out, z, x[:, c0:c0 + cols])
    np.add.at(mag, z, np.abs(x[:, c0:c0 + cols]))
    return out, (species_chains(z)[0][:, None] + 2) * U * mag


def species_total(col, z):
    """total = sum_i x[i][c_total] and its bound (n' + 2) u sum |x| (species_chains)"""
    col = np.asarray(col, np.float64)
    return col.sum(), (species_chains(z)[1] + 2) * U * np.abs(col).sum()


LOSS_MSE, LOSS_MAE, LOSS_HUBER = 0, 1, 2


def loss_term(d, mode, delta):
    d = np.asarray(d, np.float64)
    if mode == LOSS_MAE:
        return np.abs(d), np.sign(d)
    if mode == LOSS_HUBER:
        small = np.abs(d) <= delta
        return np.where(small, 0.5 * d * d, delta * (np.abs(d) - 0.5 * delta)), np.where(small, d, delta * np.sign(d))
    return d * d, 2.0 * d


def loss_grad(e, e_lab, f, f_lab, w, mode_e, mode_f, delta_e, delta_f):
    """nnhip_loss_grad: (loss, bound, g_e, g_f).  The residuals are the fp32 differences the kernel forms (exact inputs to the
    loss terms: a residual exactly at 0 or +-delta stays there); bound: each term rounded a few times in fp32 (4 u each) before
    the fp64 sum, whose result is rounded to fp32 once."""
    de = (np.asarray(e, np.float32) - np.asarray(e_lab, np.float32)).astype(np.float64)
    df = (np.asarray(f, np.float32) - np.asarray(f_lab, np.float32)).astype(np.float64)
    le, ge = loss_term(de, mode_e, delta_e)
    lf, gf = loss_term(df, mode_f, delta_f)
    loss = w[0] * le.sum() + w[1] * lf.sum()
    mag = abs(w[0]) * np.abs(le).sum() + abs(w[1]) * np.abs(lf).sum()
    return loss, 4 * U * mag + U * abs(loss), w[0] * ge, w[1] * gf


OPT_BLOCKS = 256        # csrc/train.hip: the two-pass layout of the gradient norm


def grad_norm_rel_bound():
    """(n' + 2) u: the squares are summed in fp64 inside a workgroup and across the OPT_BLOCKS partials; each partial is rounded
    to fp32 ONCE in between, so the longest fp32 chain has n' = 1 link (then sqrt and the store round once more each)."""
    return (1 + 2) * U


def clip_adam_step(p, g, m, v, t, lr, b1, b2, eps, max_norm, mask=None):
    """one clip_grad_norm_ + Adam step in float64 (torch.optim.Adam defaults); returns (p, m, v, norm).  mask == 0: frozen."""
    p, g, m, v = (np.array(a, np.float64) for a in (p, g, m, v))
    live = np.ones(p.shape, bool) if mask is None else np.asarray(mask) != 0
    norm = np.sqrt((g[live] ** 2).sum())
    clip = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    gc = g * clip
    m2, v2 = b1 * m + (1 - b1) * gc, b2 * v + (1 - b2) * gc * gc
    step = lr / (1 - b1 ** t) * m2 / (np.sqrt(v2) / np.sqrt(1 - b2 ** t) + eps)
    return np.where(live, p - step, p), np.where(live, m2, m), np.where(live, v2, v), norm
