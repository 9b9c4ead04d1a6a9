"""fp64 numpy model of the blocked complex Hermitian Jacobi iteration of csrc/phonon_large.hip: the same padding (the order rounded
up to a multiple of 64, padding rows and columns exactly zero), the same blocks of 32 coordinates on the round-robin ordering, the
same inner solve (scalar round-robin complex Jacobi on the 64 x 64 diagonal sub-problem, stopped at off^2 <= EIG_EPS2 / 64 ||sub||_F^2
or after INNER_SWEEPS sweeps), the Newton-Schulz step on the accumulated rotation, the tile update T <- Qt_k T Qt_l^H, and the outer
rule off^2 <= EIG_EPS2 ||A||_F^2 within MAX_SWEEPS sweeps.  It states on the CPU the convergence argument of DESIGN.md 23a: with the
inner rule 64 times tighter than the outer one the iteration reaches the outer rule.  Independent of the package."""
import numpy as np

BLOCK = 32
SUB = 2 * BLOCK
EIG_EPS2 = (2.0 ** -24) ** 2
INNER_EPS2 = EIG_EPS2 / 64.0
INNER_SWEEPS = 15
MAX_SWEEPS = 30


def rr_pair(k, s, n):
    """the partners of pair k at step s of the round-robin on n players (n even): p < q"""
    m = n - 1
    if k == 0:
        a, b = m, s
    else:
        a, b = (s + k) % m, (s - k) % m
    return (a, b) if a < b else (b, a)


def pad_order(d):
    return (d + SUB - 1) // SUB * SUB


def off2_norm2(A):
    """(off(A)^2, ||A||_F^2), the two parts summed apart as the device does (a difference would cancel)"""
    dg2 = float((np.abs(np.diag(A)) ** 2).sum())
    off = float((np.abs(A - np.diag(np.diag(A))) ** 2).sum())
    return off, off + dg2


def step_rotation(A, s):
    """L of one step of the scalar ordering on A (order n even): the n / 2 disjoint rotations, A <- L A L^H annihilates every a_pq
    of the step.  For pair (p, q): u = a_pq / |a_pq|, tau = (a_qq - a_pp) / (2 |a_pq|), t = sign(tau) / (|tau| + sqrt(1 + tau^2)),
    rows p and q of L are (c, -s u) and (s, c u)."""
    n = A.shape[0]
    L = np.zeros((n, n), dtype=np.complex128)
    for k in range(n // 2):
        p, q = rr_pair(k, s, n)
        apq = A[p, q]
        ab = abs(apq)
        if ab == 0.0:
            L[p, p] = L[q, q] = 1.0
            continue
        u = apq / ab
        tau = (A[q, q].real - A[p, p].real) / (2.0 * ab)
        t = (1.0 if tau >= 0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
        c = 1.0 / np.sqrt(1.0 + t * t)
        sn = t * c
        L[p, p], L[p, q], L[q, p], L[q, q] = c, -sn * u, sn, c * u
    return L


def inner_solve(A):
    """(diagonal, Qt, sweeps): the sub-problem by the scalar cyclic Jacobi, Qt = the accumulated L (A <- Qt A Qt^H is diagonal to the
    inner rule), brought back to the nearest unitary matrix by one Newton-Schulz step"""
    A = A.copy()
    n = A.shape[0]
    Q = np.eye(n, dtype=np.complex128)
    sweeps = 0
    while True:
        off, nrm = off2_norm2(A)
        if off <= INNER_EPS2 * nrm or sweeps == INNER_SWEEPS:
            break
        for s in range(n - 1):
            L = step_rotation(A, s)
            A = L @ A @ L.conj().T
            A = 0.5 * (A + A.conj().T)      # the device writes every tile with its conjugate mirror: exactly Hermitian
            Q = L @ Q
        sweeps += 1
    Q = Q - 0.5 * (Q @ Q.conj().T - np.eye(n)) @ Q
    return np.diag(A).real.copy(), Q, sweeps


def block_jacobi(D, want_modes=True):
    """dict(evals ascending, modes (rows), sweeps, converged, padding_zero, inner_max) of the Hermitian D [d, d]"""
    d = D.shape[0]
    Mp = pad_order(d)
    A = np.zeros((Mp, Mp), dtype=np.complex128)
    A[:d, :d] = 0.5 * (D + D.conj().T)
    W = np.eye(Mp, dtype=np.complex128)
    nblk = Mp // BLOCK
    P = nblk // 2
    sweeps, converged, padding_zero, inner_max = 0, False, True, 0
    while True:
        off, nrm = off2_norm2(A)
        converged = off <= EIG_EPS2 * nrm
        if converged or sweeps == MAX_SWEEPS:
            break
        for s in range(nblk - 1):
            idx, Qt = [], []
            for k in range(P):
                p, q = rr_pair(k, s, nblk)
                ix = np.concatenate([np.arange(p * BLOCK, (p + 1) * BLOCK), np.arange(q * BLOCK, (q + 1) * BLOCK)])
                dg, Qk, n_in = inner_solve(A[np.ix_(ix, ix)])
                inner_max = max(inner_max, n_in)
                A[np.ix_(ix, ix)] = np.diag(dg)          # the solved diagonal and exact zeros
                idx.append(ix)
                Qt.append(Qk)
            for k in range(P):
                for l in range(k + 1, P):
                    T = Qt[k] @ A[np.ix_(idx[k], idx[l])] @ Qt[l].conj().T
                    A[np.ix_(idx[k], idx[l])] = T
                    A[np.ix_(idx[l], idx[k])] = T.conj().T
                if want_modes:
                    W[idx[k], :] = Qt[k].conj() @ W[idx[k], :]
        sweeps += 1
        padding_zero = padding_zero and not A[d:, :].any() and not A[:, d:].any()
    lam = np.diag(A).real[:d]
    order = np.argsort(lam, kind='stable')
    return dict(evals=lam[order], modes=W[:d, :d][order], sweeps=sweeps, converged=converged, padding_zero=padding_zero,
                inner_max=inner_max, identity_on_padding=bool(np.array_equal(W[d:, d:], np.eye(Mp - d)) and not W[:d, d:].any()))


def planted_case(n, seed):
    """(fc fp32 [n,3,n,3], pos, cell, S, masses fp32): a random symmetric block as the force constants of n atoms on the (1, 1, 1)
    supercell of a mildly triclinic 9 A cell, mixed masses (the planted case of tests/test_hip_phonons.py, restated)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3 * n, 3 * n))
    fc = (X + X.T).astype(np.float32).reshape(n, 3, n, 3)
    pos = rng.uniform(0.0, 9.0, (n, 3))
    m = rng.choice([1.008, 12.011, 15.999], n).astype(np.float32)
    return fc, pos, 9.0 * np.eye(3) + 0.3 * rng.standard_normal((3, 3)), (1, 1, 1), m
