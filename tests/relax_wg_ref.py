"""What the tests of the workgroup-per-system L-BFGS form (nnhip_lbfgs_step_wg, nnhip_cell_lbfgs_step_wg; csrc/lbfgs_chain.h:
BlockTeam) add to tests/relax_ref.py and tests/cellrelax_ref.py (numpy only).

The workgroup form computes the same chain as the wave form; only its reductions are ordered differently: thread t of 1024 sums
its rows t, t + 1024, ... in row order, each wave folds its 64 values by the butterfly 32 .. 1, and the 16 wave results are folded
as  for d in 8, 4, 2, 1: p[i] += p[i + d].  A term of a dot product over n rows therefore passes through
    wg_dot_depth(n) = 3 (product, two fmas) + ceil(n / 1024) (thread-local adds) + 6 (butterfly) + 4 (fold)
roundings, against relax_ref.dot_depth(n) = 3 + ceil(n / 64) + 6 of the wave form -- MORE below 193 rows, fewer above 320.
`workgroup_depth()` swaps relax_ref.dot_depth for it (relax_ref._dot and _two_loop look the name up at call time, and
cellrelax_ref goes through relax_ref), so that both fp64 references bound the workgroup form; `block_emulation()` swaps the float32
emulation's reduction likewise.  Everything else -- C_RX, the bounds, the ambiguity rule -- is relax_ref's, unchanged.

The batches here are built for sizes the dense SPD matrices of relax_ref.synthetic_batch do not reach: the stored pairs are
y = A s with a MATRIX-FREE symmetric positive definite A = D + U diag(w) U^T: D a diagonal, log-uniform in [20, 1000] with both
ends present, U eight orthonormal columns, w in [100, 1000] -- by Weyl's inequality the spectrum lies in [20, 2000], condition at
most 100, as relax_ref._spd's."""
import contextlib
import math

import numpy as np

from tests import cellrelax_ref as cr
from tests import relax_ref as rr

WG_THREADS = 1024
MEMORY = 4
SENT = 777.0
INTS = ('converged', 'n_steps', 'n_pairs', 'head')


def wg_dot_depth(n):
    return 3 + (n + WG_THREADS - 1) // WG_THREADS + 6 + 4


@contextlib.contextmanager
def workgroup_depth():
    """relax_ref (and through it cellrelax_ref) bound the workgroup form's reductions while this is active"""
    keep = rr.dot_depth
    rr.dot_depth = wg_dot_depth
    try:
        yield
    finally:
        rr.dot_depth = keep


def _block_sum32(t):
    """the workgroup's reduction in float32, operation for operation (the manner of relax_ref._wave_sum32)"""
    acc = np.zeros(WG_THREADS, dtype=np.float32)
    for i0 in range(0, t.shape[0], WG_THREADS):
        chunk = t[i0:i0 + WG_THREADS]
        acc[:chunk.shape[0]] = acc[:chunk.shape[0]] + chunk
    lanes = np.arange(WG_THREADS)
    for d in (32, 16, 8, 4, 2, 1):                     # (t ^ d stays inside the wave of t)
        acc = (acc + acc[lanes ^ d]).astype(np.float32)
    p = acc[::64].copy()                               # what lane 0 of each of the 16 waves writes
    for d in (8, 4, 2, 1):
        p[:d] = (p[:d] + p[d:2 * d]).astype(np.float32)
    return p[0]


@contextlib.contextmanager
def block_emulation():
    """relax_ref.emulate_step (and cellrelax_ref.emulate_system, which calls it) reduce as the workgroup does"""
    keep = rr._wave_sum32
    rr._wave_sum32 = _block_sum32
    try:
        yield
    finally:
        rr._wave_sum32 = keep


def emulate_step(x, F, free, st, tol2, alpha, maxstep, flags=0):
    """relax_ref.emulate_step with the workgroup's reductions"""
    with block_emulation():
        return rr.emulate_step(x, F, free, st, tol2, alpha, maxstep, flags)


# ---- a plain fp64 step, no bounds, O(memory x n) ------------------------------------------------------------------------------------

def plain_step(x, F, free, st, tol2, alpha, maxstep, flags=0):
    """One launch for one molecule in fp64 from the fp32 inputs, without bounds and without dense maps.  Returns dict(x_out, frozen,
    accepted, clamped, converged, n_steps, n_pairs, head)."""
    x, f = np.asarray(x, dtype=np.float64), rr.masked(F, free)
    n, m = x.shape[0], st['S'].shape[0]
    fmax2 = float((f * f).sum(1).max()) if n else 0.0
    now = n == 0 or fmax2 < float(tol2)
    out = dict(accepted=None, clamped=False, n_steps=st['n_steps'], n_pairs=st['n_pairs'], head=st['head'])
    if st['converged'] or now or (flags & rr.CHECK_ONLY):
        out.update(x_out=x.copy(), frozen=True, converged=bool(st['converged'] or now))
        return out
    S, Y, rho = st['S'].copy(), st['Y'].copy(), st['rho'].copy()
    head, n_pairs = st['head'], st['n_pairs']
    if st['n_steps'] > 0:
        y, s = rr.pair_y(st['f_prev'], f), S[head]
        ys, yy, ss = float((y * s).sum()), float((y * y).sum()), float((s * s).sum())
        out['accepted'] = ys > 0.0 and ys * ys > rr.CURVATURE_MIN2 * (yy * ss)
        if out['accepted']:
            Y[head], rho[head] = y, 1.0 / ys
            n_pairs, head = min(n_pairs + 1, m), (head + 1) % m
        elif n_pairs == m:
            n_pairs = m - 1
    slots = rr.pair_slots(head, n_pairs, m)
    q, a = -f, {}
    for k in slots:
        a[k] = rho[k] * float((S[k] * q).sum())
        q = q - a[k] * Y[k]
    z = q / float(alpha)
    for k in reversed(slots):
        z = z + (a[k] - rho[k] * float((Y[k] * z).sum())) * S[k]
    longest = math.sqrt(float((z * z).sum(1).max()))
    out['clamped'] = longest >= float(maxstep)
    if out['clamped']:
        z = z * (float(maxstep) / longest)
    x_out = x - z
    if free is not None:
        x_out = np.where(np.asarray(free, dtype=bool)[:, None], x_out, x)
    out.update(x_out=x_out, frozen=False, converged=False, n_steps=st['n_steps'] + 1, n_pairs=n_pairs, head=head)
    return out


# ---- batches in the kernel's layout, sizes and variants given by the caller ------------------------------------------------------------

class SpdOperator:
    """v -> A v for the matrix-free SPD A of the module docstring over d coordinates, restricted to the coordinates of `mask`"""

    def __init__(self, rng, d, mask):
        self.mask = np.asarray(mask, dtype=np.float64)
        lam = np.exp(rng.uniform(np.log(20.0), np.log(1000.0), d))
        if d:
            lam[0], lam[-1] = 20.0, 1000.0 if d > 1 else 20.0
        r = min(8, d)
        self.lam = lam
        self.U = np.linalg.qr(rng.standard_normal((d, r)))[0] if d else np.zeros((0, 0))
        self.w = rng.uniform(100.0, 1000.0, r)

    def __call__(self, v):
        v = np.asarray(v, dtype=np.float64) * self.mask
        return self.mask * (self.lam * v + self.U @ (self.w * (self.U.T @ v)))


def _history(rng, A, mask, rows, pairs, kind, m):
    """the ring of a system of `rows` rows before the launch: (head, S, Y, rho, n_steps, pending y or None) -- relax_ref's layout:
    heads placed so that rings wrap, unused slots 7.0 (S, Y) and 0.5 (rho)"""
    f32, d = np.float32, 3 * rows
    head = {0: 0, 1: 1, 2: m - 1, m - 1: m - 1, m: 2}[pairs] if kind != 'first' else 0
    S, Y, rho = np.full((m, rows, 3), 7.0, dtype=f32), np.full((m, rows, 3), 7.0, dtype=f32), np.full(m, 0.5, dtype=f32)
    for k in rr.pair_slots(head, min(pairs, m - 1 if kind != 'first' else m), m):
        s = (rng.normal(0, 0.05, d) * mask).astype(f32)
        y = A(s).astype(f32)
        S[k], Y[k] = s.reshape(rows, 3), y.reshape(rows, 3)
        rho[k] = f32(1.0 / float(y.astype(np.float64) @ s.astype(np.float64))) if d else f32(0.5)
    if kind == 'first':
        return head, S, Y, rho, 0, None
    s = (rng.normal(0, 0.05, d) * mask).astype(f32)
    s64 = s.astype(np.float64)
    if kind == 'reject_cos' and d:
        v = rng.normal(0, 1.0, d) * mask
        v -= (v @ s64) / (s64 @ s64) * s64
        y = 5.0 * (v / np.linalg.norm(v) + 2e-5 * s64 / np.linalg.norm(s64))
    else:
        y = A(s64) * (-1.0 if kind == 'reject_neg' else 1.0)
    S[head] = s.reshape(rows, 3)
    return head, S, Y, rho, pairs + 3, y.reshape(rows, 3)


def _free_atoms(rng, n, fixed):
    free = np.ones(n, dtype=bool)
    if fixed and n >= 2:
        free = rng.random(n) >= 0.25
        free[rng.integers(n)] = True
    return free


def relax_batch(cases, seed=0, memory=MEMORY):
    """A batch for nnhip_lbfgs_step(_wg) in the layout of relax_ref.synthetic_batch.  cases: (n atoms, pairs stored, kind, big,
    fixed) per molecule, kinds as relax_ref.SYN_VARIANTS ('empty' for n = 0 is any of them); big: forces of ~30 eV/A (the clamp)
    instead of ~0.5; fixed: a quarter of the atoms held."""
    rng = np.random.default_rng(seed)
    f32, m = np.float32, memory
    mols = []
    for n, pairs, kind, big, fixed in cases:
        free = _free_atoms(rng, n, fixed)
        mask = np.repeat(free, 3).astype(np.float64)
        A = SpdOperator(rng, 3 * n, mask)
        head, S, Y, rho, n_steps, y = _history(rng, A, mask, n, pairs, kind, m)
        F = rng.normal(0, 30.0 if big else 0.5, (n, 3)).astype(f32)
        if kind == 'converging' and n:
            F = (F.astype(np.float64) * (0.005 / np.sqrt((rr.masked(F, free) ** 2).sum(1).max()))).astype(f32)
        f = rr.masked(F, free).astype(f32)
        f_prev = np.full((n, 3), 7.0, dtype=f32) if y is None else (f.astype(np.float64) + y).astype(f32)
        mols.append(dict(n=n, kind=kind, big=big, free=free, x=rng.uniform(-8, 8, (n, 3)).astype(f32), F=F, S=S, Y=Y, rho=rho,
                         f_prev=f_prev, converged=int(kind == 'converged'), n_steps=n_steps,
                         n_pairs=pairs if kind != 'first' else 0, head=head))
    out = dict(ptr=np.concatenate([[0], np.cumsum([q['n'] for q in mols])]).astype(np.int32), kinds=[q['kind'] for q in mols],
               big=[q['big'] for q in mols], memory=m, tol2=rr.SYN_TOL2, alpha=rr.SYN_ALPHA, maxstep=rr.SYN_MAXSTEP)
    for k in ('x', 'F', 'f_prev', 'free'):
        out[k] = np.concatenate([q[k] for q in mols])
    for k in ('S', 'Y'):
        out[k] = np.ascontiguousarray(np.concatenate([q[k] for q in mols], axis=1))
    out['rho'] = np.stack([q['rho'] for q in mols])
    for k in INTS:
        out[k] = np.array([q[k] for q in mols], dtype=np.int32)
    return out


def cell_batch(cases, seed=0, memory=MEMORY):
    """A batch for nnhip_cell_lbfgs_step(_wg) in the layout of cellrelax_ref.synthetic_batch.  cases: (n atoms, pairs stored, kind,
    load, fixed) per system, kinds as cellrelax_ref.SYN_VARIANTS and loads as the names of cellrelax_ref.SYN_LOADS.  Systems
    alternate between cells, deformation gradients, pressures and cell factors as they do there."""
    rng = np.random.default_rng(seed)
    f32, m = np.float32, memory
    loads = {name: (fs, ws) for name, fs, ws in cr.SYN_LOADS}
    systems = []
    for count, (n, pairs, kind, load, fixed) in enumerate(cases, start=1):
        f_scale, w_scale = loads[load]
        free = _free_atoms(rng, n, fixed)
        mask = np.repeat(cr.row_free(free, n), 3).astype(np.float64)
        c = f32(3.5) if count % 4 == 0 else f32(max(n, 1))
        p = f32((0.0, 2e-3, 0.0, -2e-3)[count % 4]) if count % 5 else f32(1e-3)
        h0 = np.diag(rng.uniform(7.0, 12.0, 3))
        if count % 2 == 0:
            h0 = h0 + np.tril(rng.normal(0, 1.5, (3, 3)), -1)
            h0 = h0 @ np.linalg.qr(rng.standard_normal((3, 3)))[0]
            if np.linalg.det(h0) < 0:
                h0[2] = -h0[2]
        h0 = h0.astype(f32)
        F = np.eye(3) if count % 3 == 0 else np.eye(3) + rng.normal(0, 0.05, (3, 3))
        if kind == 'det_neg':
            F = F @ np.diag([1.0, 1.0, -1.0])
        X = np.concatenate([rng.uniform(-8, 8, (n, 3)), float(c) * F]).astype(f32)
        F32 = X[n:].astype(np.float64) / float(c)
        cell = (h0.astype(np.float64) @ F32.T).astype(f32)
        pos = (X[:n].astype(np.float64) @ F32.T).astype(f32)
        f = rng.normal(0, f_scale, (n, 3)).astype(f32)
        W = (rng.normal(0, w_scale * float(c), (3, 3))).astype(f32)
        W = ((W + W.T) / 2).astype(f32)
        G = None
        if kind != 'det_neg':
            G = cr.generalised_forces(f, W, F32, cell, float(p), float(c), free)
            if kind == 'converging':
                s = 0.003 / np.sqrt((G ** 2).sum(1).max())
                pv = float(p) * np.linalg.det(cell.astype(np.float64))
                f = (f.astype(np.float64) * s).astype(f32)
                W = ((W.astype(np.float64) - pv * np.eye(3)) * s + pv * np.eye(3)).astype(f32)
                G = cr.generalised_forces(f, W, F32, cell, float(p), float(c), free)
        A = SpdOperator(rng, 3 * (n + 3), mask)
        head, S, Y, rho, n_steps, y = _history(rng, A, mask, n + 3, pairs, kind, m)
        g_prev = np.full((n + 3, 3), 7.0, dtype=f32)
        if y is not None and G is not None:
            g_prev = (G + y).astype(f32)
        systems.append(dict(n=n, kind=kind, load=load, free=free, X=X, pos=pos, f=f, W=W, cell=cell, h0=h0, p=p, c=c, S=S, Y=Y,
                            rho=rho, g_prev=g_prev, converged=int(kind == 'converged'), n_steps=n_steps,
                            n_pairs=pairs if kind != 'first' else 0, head=head))
    out = dict(ptr=np.concatenate([[0], np.cumsum([s['n'] for s in systems])]).astype(np.int32),
               kinds=[s['kind'] for s in systems], loads=[s['load'] for s in systems], memory=m, tol2=cr.SYN_TOL2, alpha=cr.SYN_ALPHA,
               maxstep=cr.SYN_MAXSTEP)
    for k in ('X', 'pos', 'f', 'g_prev', 'free'):
        out[k] = np.concatenate([s[k] for s in systems])
    for k in ('S', 'Y'):
        out[k] = np.ascontiguousarray(np.concatenate([s[k] for s in systems], axis=1))
    for k in ('rho', 'W', 'cell', 'h0'):
        out[k] = np.stack([s[k] for s in systems])
    for k in ('p', 'c'):
        out[k] = np.array([s[k] for s in systems], dtype=f32)
    for k in INTS:
        out[k] = np.array([s[k] for s in systems], dtype=np.int32)
    return out


# ---- the cases of the tests (shared by the host tests, which show that no decision in them is ambiguous, and the GPU tests) ----------

SMALL_SIZES = (0, 1, 63, 64, 65, 200)                 # every variant, both force scales, with and without fixed atoms
EDGE_SIZES = (1023, 1024, 1025)                       # the last register work vector, the first rows of `work`
EDGE_VARIANTS = ((0, 'first'), (MEMORY, 'accept'), (MEMORY, 'reject_neg'), (1, 'converging'))
LARGE_SIZES = (2049, 5127)                            # 3 and 6 rows per thread, the last pass partial
# variants that leave NO stored pair after the pending decision: the fp64 reference needs no dense map
NO_PAIR_VARIANTS = ((0, 'first'), (0, 'reject_neg'), (2, 'converged'), (1, 'converging'))
SEED = 0


def relax_small_batch():
    """every variant of relax_ref.SYN_VARIANTS at every size of SMALL_SIZES, forces of 0.5 and 30 eV/A, with and without fixed atoms"""
    return relax_batch([(n, pairs, kind, big, fixed) for n in SMALL_SIZES for pairs, kind in rr.SYN_VARIANTS
                        for big in (False, True) for fixed in (False, True)], seed=SEED)


def relax_edge_case(n, v):
    """one molecule of n atoms (EDGE_SIZES, LARGE_SIZES), variant v of EDGE_VARIANTS"""
    pairs, kind = EDGE_VARIANTS[v]
    return relax_batch([(n, pairs, kind, (n + v) % 2 == 1, (n + v // 2) % 2 == 0)], seed=SEED + 1000 * v + n)


def relax_large_batch(n):
    """the NO_PAIR_VARIANTS at n atoms, forces of 0.5 and 30 eV/A, alternately with fixed atoms"""
    return relax_batch([(n, pairs, kind, big, (k + big) % 2 == 0) for k, (pairs, kind) in enumerate(NO_PAIR_VARIANTS)
                        for big in (False, True)], seed=SEED + n)


def relax_history_batch(n):
    """accepted pairs on a full history at n atoms (tier C): unclamped and clamped, without and with fixed atoms"""
    return relax_batch([(n, MEMORY, 'accept', big, big) for big in (False, True)], seed=SEED + 7 * n)


def relax_many_batch(n_mol=2100):
    """n_mol molecules of 1 to 3 atoms, the variants of relax_ref.SYN_VARIANTS in turn: more systems than the 2048 workgroups of the
    grid-stride loop"""
    return relax_batch([(1 + k % 3, *rr.SYN_VARIANTS[k % len(rr.SYN_VARIANTS)], k % 4 == 1, k % 5 == 0) for k in range(n_mol)],
                       seed=SEED + 1)


CELL_SMALL_SIZES = (0, 1, 61, 62, 200)                # 61 and 62 atoms: 64 and 65 rows
CELL_EDGE_ROWS = (1023, 1024, 1025)                   # atoms = rows - 3


def cell_small_batch():
    """every variant of cellrelax_ref.SYN_VARIANTS under every load at every size of CELL_SMALL_SIZES, alternately with fixed atoms"""
    return cell_batch([(n, pairs, kind, load, (k + j) % 2 == 0) for n in CELL_SMALL_SIZES
                       for k, (pairs, kind) in enumerate(cr.SYN_VARIANTS) for j, (load, _, _) in enumerate(cr.SYN_LOADS)], seed=SEED)


def cell_edge_case(rows, v):
    """one system of rows - 3 atoms, variant v of EDGE_VARIANTS, the load alternating"""
    pairs, kind = EDGE_VARIANTS[v]
    return cell_batch([(rows - 3, pairs, kind, cr.SYN_LOADS[(rows + v) % 3][0], (rows + v) % 2 == 0)], seed=SEED + 1000 * v + rows)


def cell_large_batch(n):
    """the NO_PAIR_VARIANTS at n atoms under the three loads in turn"""
    return cell_batch([(n, pairs, kind, cr.SYN_LOADS[(k + j) % 3][0], k % 2 == 0) for k, (pairs, kind) in enumerate(NO_PAIR_VARIANTS)
                       for j in range(2)], seed=SEED + n)


def cell_history_batch(n):
    """accepted pairs on a full history at n atoms (tier C): the clamp decided by no row, by an atom row, by a cell row"""
    return cell_batch([(n, MEMORY, 'accept', load, k == 1) for k, (load, _, _) in enumerate(cr.SYN_LOADS)], seed=SEED + 7 * n)


def cell_many_batch(n_mol=2100):
    """n_mol systems of 1 to 3 atoms, the variants of cellrelax_ref.SYN_VARIANTS and the loads in turn"""
    return cell_batch([(1 + k % 3, *cr.SYN_VARIANTS[k % len(cr.SYN_VARIANTS)], cr.SYN_LOADS[k % 3][0], k % 5 == 0)
                       for k in range(n_mol)], seed=SEED + 1)


# ---- one launch of nnhip_lbfgs_step(_wg) on a batch: the emulation, and the check against the fp64 reference -------------------------

def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def slice_relax(d, b):
    """molecule b of a relax batch as a batch of its own"""
    a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
    out = dict(d, ptr=np.array([0, a1 - a0], dtype=np.int32), kinds=[d['kinds'][b]], big=[d['big'][b]])
    for k in ('x', 'F', 'f_prev', 'free'):
        out[k] = d[k][a0:a1]
    for k in ('S', 'Y'):
        out[k] = np.ascontiguousarray(d[k][:, a0:a1])
    out['rho'] = d['rho'][b:b + 1]
    for k in INTS:
        out[k] = d[k][b:b + 1]
    return out


def emulate_relax_launch(d, flags=0):
    """emulate_step (the workgroup's reductions) over a batch, laid out and sentinel-filled as the GPU test's launch leaves it"""
    f32 = np.float32
    out = {k: d[k].copy() for k in ('S', 'Y', 'rho', 'f_prev') + INTS}
    N, B = d['x'].shape[0], len(d['ptr']) - 1
    out.update(pos_out=np.full((N, 3), SENT, f32), fmax=np.full(B, SENT, f32))
    for b in range(B):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        st = rr.batch_state(d, b)
        x_out, fmax, new = emulate_step(d['x'][a0:a1], d['F'][a0:a1], d['free'][a0:a1], st, d['tol2'], d['alpha'], d['maxstep'], flags)
        out['pos_out'][a0:a1], out['fmax'][b] = x_out, fmax
        out['converged'][b] = int(new['converged'])
        if new['n_steps'] == st['n_steps']:
            continue
        out['S'][:, a0:a1], out['Y'][:, a0:a1], out['rho'][b] = new['S'].astype(f32), new['Y'].astype(f32), new['rho'].astype(f32)
        out['f_prev'][a0:a1] = new['f_prev'].astype(f32)
        out['n_steps'][b], out['n_pairs'][b], out['head'][b] = new['n_steps'], new['n_pairs'], new['head']
    return out


def check_relax_launch(d, out, flags=0):
    """Assert that `out` (the state after the launch, pos_out and fmax written over SENT) is what one launch on the batch `d` must
    leave, by the yardstick of tests/test_hip_relax.py: every output within relax_ref's bound (C_RX x first order) plus half an fp32
    ulp, integers and flags exact, y and S[head] bitwise, everything a step must not touch bitwise untouched.  The caller chooses the
    depth (workgroup_depth()).  Returns (worst err / bound per output, the set of branches seen, the list of ambiguous decisions)."""
    worst = dict(x=0.0, fmax=0.0, rho=0.0)
    seen, ambiguous = set(), []
    for b, kind in enumerate(d['kinds']):
        a0, a1 = int(d['ptr'][b]), int(d['ptr'][b + 1])
        st = rr.batch_state(d, b)
        ref = rr.batch_step(d, b, flags)
        new = ref['state']
        what = f'molecule {b} ({kind}, {a1 - a0} atoms, flags {flags})'
        ambiguous += [(b, kind, k) for k, a in ref['ambiguous'].items() if a]
        seen.add((kind, ref['frozen'], ref['accepted'], ref['clamped']))
        for k in INTS:
            assert int(out[k][b]) == int(new[k]), f'{what}: {k} {out[k][b]} != {int(new[k])}'
        e, bound = abs(float(out['fmax'][b]) - ref['fmax']), ref['b_fmax'] + rr.half_ulp32(ref['fmax'])
        assert e <= bound, f'{what}: fmax err / bound {e / bound:.3f}'
        worst['fmax'] = max(worst['fmax'], e / bound)
        x, xo, free = d['x'][a0:a1], out['pos_out'][a0:a1], d['free'][a0:a1]
        S1, Y1, rho1 = out['S'][:, a0:a1], out['Y'][:, a0:a1], out['rho'][b]
        S0, Y0, rho0 = d['S'][:, a0:a1], d['Y'][:, a0:a1], d['rho'][b]
        if ref['frozen']:
            assert _same_bits(xo, x), f'{what}: a frozen molecule moved'
            assert _same_bits(S1, S0) and _same_bits(Y1, Y0) and _same_bits(rho1, rho0), f'{what}: history touched'
            assert _same_bits(out['f_prev'][a0:a1], d['f_prev'][a0:a1]), f'{what}: f_prev touched'
            continue
        err = np.abs(xo.astype(np.float64) - ref['x_out'])
        bx = ref['bx'] + rr.half_ulp32(ref['x_out'])
        assert np.all(err <= bx), f'{what}: positions err / bound {float((err / bx).max()):.3f}'
        worst['x'] = max(worst['x'], float((err / bx).max()))
        assert _same_bits(xo[~free], x[~free]), f'{what}: a fixed atom moved'
        assert (xo[free] != x[free]).any(), f'{what}: nothing moved'
        h0, h1 = st['head'], new['head']
        assert _same_bits(S1[h1], rr.stored_s(xo, x).astype(np.float32)), f'{what}: S[head]'
        assert _same_bits(out['f_prev'][a0:a1], rr.masked(d['F'][a0:a1], free).astype(np.float32)), f'{what}: f_prev'
        for k in range(d['memory']):
            if k != h1:
                assert _same_bits(S1[k], S0[k]), f'{what}: S[{k}] touched'
            if not (ref['accepted'] and k == h0):
                assert _same_bits(Y1[k], Y0[k]) and _same_bits(rho1[k], rho0[k]), f'{what}: Y / rho [{k}] touched'
        if ref['accepted']:
            assert _same_bits(Y1[h0], new['Y'][h0].astype(np.float32)), f'{what}: Y[head] is not fl32(f_prev - f)'
            e, bound = abs(float(rho1[h0]) - new['rho'][h0]), ref['b_rho_new'] + rr.half_ulp32(new['rho'][h0])
            assert e <= bound, f'{what}: rho err / bound {e / bound:.3f}'
            worst['rho'] = max(worst['rho'], e / bound)
    return worst, seen, ambiguous
