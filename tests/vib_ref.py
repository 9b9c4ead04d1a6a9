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
