"""fp64 yardstick of the mode Grueneisen parameters for the tests (plain numpy): dD/d eta_k as D's own sum over a plane of
force-constant derivatives, the grouping and rotation rule of degenerate perturbation theory along a split plane, gamma, the
strained-crystal construction restated independently, the mean Grueneisen parameter and the thermal expansion, and the error bounds
the device tests use.  Independent of the package: nothing here imports newtonnet_amd."""
import numpy as np

from tests import phonon_ref as pr
from tests import phonon_velocity_ref as pv

EPS32 = pr.EPS32
MAX_DEGENERATE = pv.MAX_DEGENERATE
VOIGT_PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
# The constant of error_bound in the device tests: the velocity kernel's 16, which holds on every case measured.  Measured on the
# MI355X over the cases as committed: analytic 0.12 / 0.32 / 0.26, crossings 0.34 / 0.05 / 0.48, cap 0.26, d = 99 8.5e-4 and 1.2e-3,
# the blocked solver's modes at d = 36 0.29, end to end 7.5 and 11.4 ('volume'), 6.0 and 12.4 ('voigt').  The rule of DESIGN.md
# section 23b (four times the largest, rounded up to a power of two) would give 64 and is NOT met: with 64 the bound is 3.7 % of the
# largest slope on the d = 66 analytic inputs, against the 1 % condition tests/test_gruneisen_host.py holds.  The margin is 1.3
# (DESIGN.md section 23c says where the end-to-end constant comes from).
BOUND_C = 16.0


def d_dynamical(planes, pos, cell, S, masses, q, table=None, with_abs=False):
    """dD [K, d, d] complex128: dD_k = phonon_ref.dynamical_matrix(planes[k], ...) -- D is linear in the force constants.  with_abs:
    also sum |dPhi| |mean_T exp| (m_i m_j)^-1/2 symmetrised as dD is, the terms of the running-error bound, widened by this
    function's own fp64 error in units of eps32 (per image (8 + 2 pi |q . x|) 2^-52: the phase is rounded at its size)."""
    table = pr.image_table_fast(pos, cell, S) if table is None else table
    planes = np.asarray(planes, dtype=np.float64)
    K, n, N = planes.shape[0], planes.shape[1], planes.shape[3]
    q = np.asarray(q, dtype=np.float64)
    # phonon_ref.dynamical_matrix without its loop over the planes: the weight of a pair is formed once, exactly as there, and the
    # sum over the copies of j is a reshape (J = R n + j); tests/test_gruneisen_host.py holds the two to each other
    w = np.zeros((n, N), dtype=np.complex128)
    qx = 0.0
    for i in range(n):
        for J in range(N):
            xs = table[(i, J)]
            w[i, J] = sum(np.exp(2j * np.pi * float(q @ x)) for x in xs) / len(xs)
            qx = max(qx, max(abs(float(q @ x)) for x in xs))
    m = np.ones(n) if masses is None else np.asarray(masses, dtype=np.float64)
    f = 1.0 / np.sqrt(m[:, None] * m[None, :])
    nR = N // n
    D0 = (planes.reshape(K, n, 3, nR, n, 3) * w.reshape(1, n, 1, nR, n, 1)).sum(axis=3) * f[None, :, None, :, None]
    D0 = D0.reshape(K, 3 * n, 3 * n)
    dD = 0.5 * (D0 + D0.conj().transpose(0, 2, 1))
    if not with_abs:
        return dD
    own = 1.0 + (8.0 + 2.0 * np.pi * qx) * (2.0 ** -52 / EPS32)
    A = (np.abs(planes).reshape(K, n, 3, nR, n, 3) * np.abs(w).reshape(1, n, 1, nR, n, 1)).sum(axis=3) * f[None, :, None, :, None]
    A = A.reshape(K, 3 * n, 3 * n)
    return dD, 0.5 * (A + A.transpose(0, 2, 1)) * own


def eigen_slopes(D, dD, weights, deg_tol, cap=MAX_DEGENERATE):
    """(lam [d], modes [d, d] with ROW k = e_k, dlam [d, K], first [d], capped [d]): phonon_velocity_ref.eigen_gradients with K planes
    in place of the three G_a and the split weights in place of the direction -- a group of one takes Re e^H dD_k e; a group of
    g <= cap diagonalises M_s = sum_k w_k V^H dD_k V (ascending) and hands Re diag(U^H M_k U) to its modes in that order."""
    lam, V = np.linalg.eigh(D)
    d, K = len(lam), len(dD)
    first = pv.groups(lam, deg_tol)
    dlam, capped = np.zeros((d, K)), np.zeros(d, dtype=bool)
    V = V.copy()
    s = 0
    while s < d:
        e = s + 1
        while e < d and first[e] == s:
            e += 1
        if e - s > cap:
            capped[s:e] = True
        else:
            Vg = V[:, s:e]
            M = np.array([Vg.conj().T @ dD[k] @ Vg for k in range(K)])
            if e - s > 1:
                Ms = sum(weights[k] * M[k] for k in range(K))
                _, U = np.linalg.eigh(0.5 * (Ms + Ms.conj().T))
                M = np.array([U.conj().T @ M[k] @ U for k in range(K)])
                V[:, s:e] = Vg @ U
            dlam[s:e] = np.real(np.diagonal(M, axis1=1, axis2=2)).T
        s = e
    return lam, V.T.copy(), dlam, first, capped


def gamma(lam, dlam, zero_tol, capped=None):
    """(gamma [d, K], defined [d]): -dlam / (2 lam); zero and undefined for |lam| <= zero_tol and for capped modes"""
    lam = np.asarray(lam, dtype=np.float64)
    defined = np.abs(lam) > zero_tol
    if capped is not None:
        defined &= ~capped
    safe = np.where(defined, lam, 1.0)
    return np.where(defined[:, None], -np.asarray(dlam) / (2.0 * safe)[:, None], 0.0), defined


def split_weights(K, w=None):
    w = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    return w / np.linalg.norm(w)


def problem(fc, planes, pos, cell, S, masses, q, weights=None, deg_rel=None, scale=None, table=None):
    """dict of one (crystal, q) problem as the library defines it: lam, modes, dlam [d, K], first, capped, gamma, defined, D, dD and
    the tolerances; scale = max |lambda| the tolerances refer to (None: this problem's own)"""
    table = pr.image_table_fast(pos, cell, S) if table is None else table
    D = pr.dynamical_matrix(fc, pos, cell, S, masses, q, table)
    dD = d_dynamical(planes, pos, cell, S, masses, q, table)
    w = split_weights(len(dD), weights)
    d = D.shape[0]
    scale = np.abs(np.linalg.eigvalsh(D)).max() if scale is None else scale
    zero_tol = pv.default_tol(d) * scale
    deg_tol = zero_tol if deg_rel is None else deg_rel * scale
    lam, modes, dlam, first, capped = eigen_slopes(D, dD, w, deg_tol)
    g, defined = gamma(lam, dlam, zero_tol, capped)
    return dict(lam=lam, modes=modes, dlam=dlam, first=first, capped=capped, gamma=g, defined=defined, D=D, dD=dD, w=w, zero_tol=zero_tol,
                deg_tol=deg_tol)


def error_bound(C, p):
    """[d]: C eps32 max_k ||dD_k||_F (1 + ||D||_F / gap_s) of a problem(): the bound on |dlam_device - dlam_ref| with device modes (the
    form of phonon_velocity_ref.error_bound with ||dD_k||_F where it has ||G_a||_F)"""
    gn = max(np.linalg.norm(p['dD'][k]) for k in range(len(p['dD'])))
    return C * EPS32 * gn * (1.0 + np.linalg.norm(p['D']) / pv.gaps(p['lam'], p['first']))


def running_bound(modes, dDabs, n_terms):
    """[d, K]: (n_terms + 2 d + 16) eps32 sum_ij |e_i| |terms|_ij |e_j| per mode and plane: an fp32 evaluation of e^H dD_k e from exact
    eigenvectors rounded to fp32"""
    d = modes.shape[0]
    ae = np.abs(modes)
    return (n_terms + 2 * d + 16) * EPS32 * np.einsum('ki,aij,kj->ka', ae, dDabs, ae)


# ---- strained crystals, restated ---------------------------------------------------------------------------------------------------

def voigt_matrix(J):
    """the unit Voigt strain J (engineering shears): eps_ab = eps_ba = 1/2 for a shear"""
    a, b = VOIGT_PAIRS[J]
    e = np.zeros((3, 3))
    e[a, b] = e[b, a] = 1.0 if a == b else 0.5
    return e


def strain_list(strain):
    if isinstance(strain, str):
        return [np.eye(3) / 3.0] if strain == 'volume' else [voigt_matrix(J) for J in range(6)]
    return [np.asarray(e, dtype=np.float64) for e in strain]


def polar(cell):
    """(P, Q): cell = P Q with P symmetric positive definite (the square root of cell cell^T by its eigen-decomposition) and Q = P^-1 cell"""
    w, U = np.linalg.eigh(cell @ cell.T)
    P = (U * np.sqrt(w)[None, :]) @ U.T
    return P, np.linalg.solve(P, cell)


def strained_crystal(pos, cell, strain, delta):
    """[((pos-, cell-, Q-), (pos+, cell+, Q+))] per strain of ONE crystal, fp64: 'volume' scales by exp(+-delta / 3); any other strain
    deforms by F = I +- delta eps and rotates the result so that the cell is symmetric, cell' = cell F Q^T, pos' = pos F Q^T"""
    pos, cell = np.asarray(pos, dtype=np.float64), np.asarray(cell, dtype=np.float64)
    out = []
    for eps in strain_list(strain):
        pair = []
        for sign in (-1.0, 1.0):
            if isinstance(strain, str) and strain == 'volume':
                f = np.exp(sign * delta / 3.0)
                pair.append((pos * f, cell * f, np.eye(3)))
            else:
                F = np.eye(3) + sign * delta * eps
                P, Q = polar(cell @ F)
                pair.append((pos @ F @ Q.T, P, Q))
        out.append(tuple(pair))
    return out


def rotate_back(phi, Q):
    """Phi = Q^T Phi_rot Q on every 3 x 3 block of phi [n, 3, N, 3]"""
    return np.einsum('ca,icJd,db->iaJb', Q, np.asarray(phi, dtype=np.float64), Q)


def rotate_forward(phi, Q):
    """Phi_rot = Q Phi Q^T: force constants in the frame r' = r Q^T"""
    return np.einsum('ac,icJd,bd->iaJb', Q, np.asarray(phi, dtype=np.float64), Q)


# ---- thermodynamics -----------------------------------------------------------------------------------------------------------------

def mode_sums(evals, gam, defined, T, threshold):
    """(sum c_v gamma_k [K], sum c_v) over the modes with lam > threshold whose gamma is defined; evals [Q, d], gam [Q, d, K]"""
    ev = np.asarray(evals, dtype=np.float64)
    live = (ev > threshold) & np.asarray(defined, dtype=bool)
    cv = np.zeros_like(ev)
    if T > 0.0:
        cv[live] = pv.heat_capacity(ev[live], T)
    return np.einsum('qs,qsk->k', cv, np.asarray(gam, dtype=np.float64)), cv.sum()


def mean(evals, gam, defined, T, threshold):
    """[K]: gamma_k(T) = sum c_v gamma_k / sum c_v"""
    num, den = mode_sums(evals, gam, defined, T, threshold)
    return num / den


def bulk_modulus_voigt(C):
    C = np.asarray(C, dtype=np.float64)
    return (C[0, 0] + C[1, 1] + C[2, 2] + 2.0 * (C[0, 1] + C[0, 2] + C[1, 2])) / 9.0


def thermal_expansion(evals, gam, defined, T, threshold, volume, C, form):
    """1 / K.  form 'volume' (K = 1): alpha_V = sum c_v gamma / (Q V B_Voigt); 'voigt' (K = 6): alpha_I = (1 / (Q V)) sum_J S_IJ sum c_v
    gamma_J, S = C^-1 (C [6, 6] in eV / A^3, volume in A^3)"""
    num, _ = mode_sums(evals, gam, defined, T, threshold)
    Q = np.asarray(evals).shape[0]
    if form == 'volume':
        return num[0] / (Q * volume * bulk_modulus_voigt(C))
    return np.linalg.inv(np.asarray(C, dtype=np.float64)) @ num / (Q * volume)


# ---- the analytic lattice -------------------------------------------------------------------------------------------------------------

# not proportional to phonon_velocity_ref.COUPLED_K; binary fractions, so the plane built from it is exact in fp32
ANALYTIC_DK = np.array([[0.5, -0.25, 0.875], [1.125, 0.25, -0.5], [-0.625, 0.75, 0.375]])


def coupled_cubic_slopes(q, dK=ANALYTIC_DK, K=pv.COUPLED_K, n_fold=1):
    """(lam [3 n_fold], dlam [3 n_fold]): phonon_velocity_ref.coupled_cubic_lattice is linear in its spring constants, so the plane
    built from dK has the slopes coupled_cubic_analytic gives at dK, branch by branch, in the order of the eigenvalues at K (stable).
    At q_x = 1/2 of the folded cell the branches k and n_fold - 1 - k have the same cosines: they stay degenerate under EVERY dK of
    this form (the mirror q_x -> -q_x), with equal slopes."""
    def branch(Kx, qu, b):          # coupled_cubic_analytic's eigenvalue of branch b, unsorted
        return sum(2.0 * Kx[c][b] / pr.CUBIC_MASS * (1.0 - np.cos(2.0 * np.pi * qu[c])) for c in range(3))
    lam, dl = [], []
    for k in range(int(n_fold)):
        qu = np.array([(q[0] + k) / n_fold, q[1], q[2]])
        for b in range(3):
            lam.append(branch(np.asarray(K, dtype=np.float64), qu, b))
            dl.append(branch(np.asarray(dK, dtype=np.float64), qu, b))
    order = np.argsort(np.array(lam), kind='stable')
    return np.array(lam)[order], np.array(dl)[order]


# ---- the d = 99 crystal of phonon_velocity_ref with a plane that tells its atoms apart -------------------------------------------------

def atom_scaled_plane(fc, seed=7):
    """(plane, c): plane[i] = c_i fc[i] with a different factor per home atom, c a permutation of 33 evenly spaced values in [0.5, 2.5].
    In planted_levels_crystal every atom is bound to its own images only, so dD = blockdiag(c_i D_ii) and a mode that lives on atom i
    has the slope c_i lambda: two crossing modes of different atoms are split by (c_j - c_i) lambda."""
    fc = np.asarray(fc, dtype=np.float64)
    n = fc.shape[0]
    c = 0.5 + 2.0 * np.random.default_rng(seed).permutation(n) / max(n - 1, 1)
    return fc * c[:, None, None, None], c
