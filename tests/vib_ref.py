"""fp64 yardstick of the normal-mode analysis for the tests (pure numpy): symmetrise, mass-weight, build and orthonormalise the
translation / rotation vectors, project, numpy.linalg.eigh.  Independent of the package: nothing here imports newtonnet_amd."""
import numpy as np

EPS32 = 2.0 ** -24
C_SOLVER = 8.0          # constant of the solver bound  c * M * eps32 * ||A||_2  the tests hold the device to
DROP_TOL = 1e-5         # a candidate whose Gram-Schmidt remainder is not above this fraction of its own norm is dropped

# CODATA 2018
E_CHARGE, AMU, C_LIGHT_CM, PLANCK = 1.602176634e-19, 1.66053906660e-27, 2.99792458e10, 6.62607015e-34
WAVENUMBER = np.sqrt(E_CHARGE / (1e-20 * AMU)) / (2.0 * np.pi * C_LIGHT_CM)      # cm^-1 per sqrt(eV / (A^2 amu))
EV_PER_WAVENUMBER = PLANCK * C_LIGHT_CM / E_CHARGE

MASSES = {1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999}


def mass_weighted(H, masses):
    """A = (H + H^T)/2 / sqrt(m_i m_j) for H [n,3,n,3] or [3n,3n]; masses [n] (None: unit)."""
    n3 = int(round(np.sqrt(np.asarray(H).size)))
    A = np.asarray(H, dtype=np.float64).reshape(n3, n3)
    A = 0.5 * (A + A.T)
    if masses is not None:
        r = np.repeat(1.0 / np.sqrt(np.asarray(masses, dtype=np.float64)), 3)
        A = A * r[:, None] * r[None, :]
    return A


def tr_rot_vectors(pos, masses, periodic=False):
    """Orthonormal translation / rotation vectors [n_proj, 3n] in mass-weighted coordinates about the centre of mass (modified
    Gram-Schmidt in the order Tx Ty Tz Rx Ry Rz; periodic: translations only)."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    m = np.ones(n) if masses is None else np.asarray(masses, dtype=np.float64)
    sq = np.sqrt(m)
    cands = []
    for k in range(3):
        v = np.zeros((n, 3))
        v[:, k] = sq
        cands.append(v.reshape(-1))
    if not periodic:
        r = pos - (m[:, None] * pos).sum(0) / m.sum()
        for k in range(3):
            e = np.zeros(3)
            e[k] = 1.0
            cands.append((np.cross(e, r) * sq[:, None]).reshape(-1))
    kept = []
    for v in cands:
        n0 = np.linalg.norm(v)
        for d in kept:
            v = v - (d @ v) * d
        rem = np.linalg.norm(v)
        if rem > DROP_TOL * n0:
            kept.append(v / rem)
    return np.array(kept).reshape(len(kept), 3 * n)


def projected(A, D):
    if len(D) == 0:
        return A
    P = np.eye(A.shape[0]) - D.T @ D
    B = P @ A @ P
    return 0.5 * (B + B.T)


def analyse(H, pos, masses, project=True, periodic=False):
    """dict(A, evals ascending, evecs rows, n_proj, s = ||A||_2) of one molecule."""
    A = mass_weighted(H, masses)
    D = tr_rot_vectors(pos, masses, periodic) if project else np.zeros((0, A.shape[0]))
    A = projected(A, D)
    w, v = np.linalg.eigh(A)
    return dict(A=A, evals=w, evecs=v.T.copy(), n_proj=len(D), s=float(np.abs(w).max()) if w.size else 0.0, D=D)


def frequencies(evals):
    return np.sign(evals) * np.sqrt(np.abs(evals)) * WAVENUMBER


def solver_bound(M, s):
    return C_SOLVER * M * EPS32 * s


# ---- synthetic blocks for the solver tests (seeded; the same arrays on the CPU-only and the GPU side) -----------------------

def random_symmetric(M, rng):
    X = rng.standard_normal((M, M))
    return (X + X.T).astype(np.float32)


def gapped_symmetric(n, rng, masses=None):
    """A random symmetric block [3n, 3n] (fp32) whose mass-weighted form keeps every eigenvalue well away from zero:
    H = X + X^T + c diag(m), so that A = A_0 + c I with c = 1.25 ||A_0||_2 and the spectrum of A lies in [0.2, 1.8] ||A||_2.
    The count of projected zeros in check_solver (|lambda| <= c M eps32 s) needs that gap: a plain random symmetric matrix
    with light and heavy atoms has a genuine eigenvalue inside the bound in about one molecule of twenty.  A shift of the
    diagonal leaves every Jacobi rotation what it was (they depend on a_qq - a_pp), so the solver's work is the same."""
    X = rng.standard_normal((3 * n, 3 * n))
    H = X + X.T
    m = np.ones(3 * n) if masses is None else np.repeat(np.asarray(masses, dtype=np.float64), 3)
    c = 1.25 * np.abs(np.linalg.eigvalsh(mass_weighted(H, None if masses is None else masses))).max()
    return (H + c * np.diag(m)).astype(np.float32)


def every_size_batch(mixed_masses):
    """42 molecules of 1 .. 42 atoms (M = 3 .. 126): (blocks fp32, positions, masses fp32 or None) per molecule; mixed masses
    are H / I-like (1.008 and 126.90) drawn per atom"""
    rng = np.random.default_rng(42)
    sizes = list(range(1, 43))
    masses = [rng.choice([1.008, 126.90], n).astype(np.float32) if mixed_masses else None for n in sizes]
    mats = [gapped_symmetric(n, rng, m) for n, m in zip(sizes, masses)]
    poss = [rng.standard_normal((n, 3)) * 3.0 for n in sizes]
    return sizes, mats, poss, masses


def planted(lam, seed):
    """A = Q diag(lam) Q^T in fp64 with Q from the QR of a seeded Gaussian matrix: (A fp64, A rounded once to fp32)."""
    lam = np.asarray(lam, dtype=np.float64)
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((lam.size, lam.size)))
    A = (Q * lam[None, :]) @ Q.T
    A = 0.5 * (A + A.T)
    return A, A.astype(np.float32)


def two_by_two_blocks(M, rng, ratio, every=1):
    """block-diagonal of 2 x 2 blocks (an odd M leaves the last index alone); block k has a_pq = ratio |a_pp - a_qq| when
    k % every == 0 and an ordinary coupling otherwise"""
    A = np.zeros((M, M))
    d = np.sort(rng.uniform(1.0, 9.0, M))
    A[np.arange(M), np.arange(M)] = d
    for k in range(M // 2):
        p, q = 2 * k, 2 * k + 1
        A[p, q] = A[q, p] = ratio * abs(d[p] - d[q]) if k % every == 0 else rng.uniform(0.5, 1.5)
    return A


def hard_spectra(M):
    """{name: (lam planted or None, A fp64, A fp32)} of the spectra a Jacobi sweep meets worst; M a multiple of 3"""
    rng = np.random.default_rng(1000 + M)
    lams = {
        'cluster': np.concatenate([np.ones(M - 3), np.full(3, 1.0 + 1e-6)]),      # 1 (x M - 3) and 1 + 1e-6 (x 3)
        'triples': np.repeat(np.linspace(-2.0, 3.0, M // 3), 3),                  # M / 3 exact triples
        'rank_one': np.concatenate([np.zeros(M - 1), [5.0]]),
        'graded': np.logspace(-6.0, 0.0, M),
        'negative': -rng.uniform(0.5, 4.0, M),
    }
    out = {k: (np.sort(v),) + planted(v, 77 + i) for i, (k, v) in enumerate(lams.items())}

    def direct(A):
        return (None, A, A.astype(np.float32))
    out['equal'] = direct(2.0 * np.eye(M))
    out['diagonal_descending'] = direct(np.diag(np.arange(M, 0, -1, dtype=np.float64)))
    out['tiny_coupling'] = direct(two_by_two_blocks(M, rng, 1e-30))
    out['tiny_and_plain_coupling'] = direct(two_by_two_blocks(M, rng, 1e-30, every=2))
    return out


def drop_rule_molecules():
    """[(name, pos fp32 [n,3], n_proj of the free molecule)] around the Gram-Schmidt drop rule (DROP_TOL = 1e-5): collinear atoms
    along (1, 2, 2)/3 -- not an axis, so every rotation candidate is non-zero and the rule alone decides -- the same with the
    second atom moved off the line by `bend` x the molecule's length, a decade or more either side of the rule, and a planar
    molecule.  In a periodic cell each of them projects the three translations only."""
    axis = np.array([1.0, 2.0, 2.0]) / 3.0
    perp = np.array([2.0, -1.0, 0.0]) / np.sqrt(5.0)
    origin = np.array([0.3, -0.2, 0.5])
    out = []
    for t in ([0.0, 1.1, 2.3], [0.0, 1.1, 2.3, 3.2]):
        t = np.array(t)
        for bend, n_proj in ((0.0, 5), (1e-7, 5), (1e-3, 6)):
            p = origin + t[:, None] * axis
            p[1] += bend * t[-1] * perp
            out.append((f'linear{len(t)}_bend{bend:g}', p.astype(np.float32), n_proj))
    other = np.cross(axis, perp)
    sq = np.array([[0.0, 0.0], [1.2, 0.1], [1.0, 1.3], [-0.2, 0.9]])
    out.append(('planar4', (origin + sq[:, :1] * perp + sq[:, 1:] * other).astype(np.float32), 6))
    return out
