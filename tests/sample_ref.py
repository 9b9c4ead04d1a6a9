"""fp64 statement of normal-mode sampling and harmonic thermochemistry for the tests (numpy): what csrc/sample.hip and
NormalModes.thermochemistry compute in fp32, per molecule, from the same inputs.

Units as newtonnet_amd/vibrations.py: eigenvalues lambda in eV / (A^2 amu), masses in amu, energies in eV, T in K.  A mode is LIVE
iff lambda > thr; every other mode has amplitude 0 and no thermodynamic weight.  eps = hbar omega = HBAR_UNIT sqrt(lambda)."""
import numpy as np

from tests import vib_ref as vr

K_BOLTZMANN = 8.617333262e-5                            # eV / K
HBAR_UNIT = vr.EV_PER_WAVENUMBER * vr.WAVENUMBER        # eV: hbar omega of lambda = 1 eV / (A^2 amu)
EPS32 = 2.0 ** -24
C_SAMPLE = 8.0                                          # the constant of the eigensolver's bounds (vib_ref.C_SOLVER)


def mode_energy(lam):
    """eps = hbar omega (eV) of eigenvalues lam > 0"""
    return HBAR_UNIT * np.sqrt(np.asarray(lam, dtype=np.float64))


def coth_half(x):
    """coth(x / 2) = 1 + 2 / expm1(x), x > 0 (inf allowed)"""
    with np.errstate(over='ignore'):
        return 1.0 + 2.0 / np.expm1(np.asarray(x, dtype=np.float64))


def variance(lam, thr, T, quantum):
    """sigma_k^2 of the amplitude of every mode (0 for a mode that is not live)"""
    lam = np.asarray(lam, dtype=np.float64)
    live = lam > thr
    l = np.where(live, lam, 1.0)
    kT = K_BOLTZMANN * float(T)
    if quantum:
        eps = mode_energy(l)
        with np.errstate(divide='ignore'):
            c = coth_half(eps / kT) if kT > 0 else np.ones_like(l)
        var = eps / (2.0 * l) * c
    else:
        var = kT / l
    return np.where(live, var, 0.0)


def sample(modes, lam, thr, masses, pos, xi, T, quantum):
    """One molecule.  modes [M, M] (row k = mode k, mass-weighted), lam [M], masses [n] or None, pos [n, 3], xi [S, M].
    Returns dict(pos [S, n, 3], dx [S, n, 3], energy [S], q [S, M], n_skipped)."""
    L = np.asarray(modes, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    M = lam.shape[0]
    n = M // 3
    sig = np.sqrt(variance(lam, thr, T, quantum))
    q = sig[None, :] * np.asarray(xi, dtype=np.float64).reshape(-1, M)
    rs = np.ones(n) if masses is None else 1.0 / np.sqrt(np.asarray(masses, dtype=np.float64))
    dx = (q @ L).reshape(-1, n, 3) * rs[None, :, None]
    energy = 0.5 * (np.where(lam > thr, lam, 0.0)[None, :] * q * q).sum(axis=1)
    return dict(pos=np.asarray(pos, dtype=np.float64)[None] + dx, dx=dx, energy=energy, q=q,
                n_skipped=int(np.count_nonzero(lam < -thr)))


def thermo_terms(lam, thr, T):
    """Per live mode the terms whose sums are U, S, F and C_v: dict of arrays [n_live, ...].
      U: (eps / 2, eps / (e^x - 1))     S: k_B (x / (e^x - 1), -ln(1 - e^-x))
      F: (eps / 2, k_B T ln(1 - e^-x))  Cv: k_B x^2 e^-x / (1 - e^-x)^2            x = eps / k_B T"""
    lam = np.asarray(lam, dtype=np.float64)
    eps = mode_energy(lam[lam > thr])
    zero = np.zeros_like(eps)
    if float(T) == 0.0:
        return dict(U=np.stack([0.5 * eps, zero], 1), S=np.stack([zero, zero], 1), F=np.stack([0.5 * eps, zero], 1), Cv=zero[:, None])
    kT = K_BOLTZMANN * float(T)
    x = eps / kT
    om = -np.expm1(-x)                                   # 1 - e^-x
    occ = np.exp(-x) / om                                # 1 / (e^x - 1)
    ln = np.log(om)
    return dict(U=np.stack([0.5 * eps, eps * occ], 1), S=K_BOLTZMANN * np.stack([x * occ, -ln], 1),
                F=np.stack([0.5 * eps, kT * ln], 1), Cv=(K_BOLTZMANN * x * x * np.exp(-x) / (om * om))[:, None])


def thermochemistry(lam, thr, T):
    """dict(U, S, F, Cv) of one molecule and, under the same keys + '_abs', the sums of the |terms|"""
    t = thermo_terms(lam, thr, T)
    out = {k: float(v.sum()) for k, v in t.items()}
    out.update({k + '_abs': float(np.abs(v).sum()) for k, v in t.items()})
    return out


def displacement_bound(M, q, masses):
    """c M 2^-24 max_k |q_k| / sqrt(m_min) per sample: q [S, M] -> [S]"""
    m_min = 1.0 if masses is None else float(np.min(masses))
    return C_SAMPLE * M * EPS32 * np.abs(q).max(axis=1) / np.sqrt(m_min)


def energy_bound(M, lam, thr, q):
    """the analogous bound of the harmonic energy: c M 2^-24 max_k |lambda_k q_k^2 / 2| per sample"""
    lam = np.asarray(lam, dtype=np.float64)
    t = 0.5 * np.where(lam > thr, lam, 0.0)[None, :] * q * q
    return C_SAMPLE * M * EPS32 * np.abs(t).max(axis=1)


# ---- shared synthetic inputs ------------------------------------------------------------------------------------------------

SYNTHETIC_SIZES = (1, 2, 0, 3, 9, 21, 42)      # atoms per molecule slot; the 0 is an empty slot


def default_threshold(M, top):
    """the library's default zero threshold of a molecule in fp32 arithmetic: (8 x 2^-24) x M x max |lambda|"""
    return np.float32(8.0 * EPS32) * np.float32(M) * np.float32(top)


def synthetic_spectrum(n):
    """Ascending eigenvalues [3 n] fp32 of the synthetic molecule of n atoms: zeros, negatives, and (n >= 3) values within 2 x of
    the default threshold on both sides of it and of its negative, the threshold itself included (not live: the rule is >)."""
    M = 3 * n
    if n == 1:
        return np.zeros(3, dtype=np.float32)                       # nothing live: the sample is the input position
    if n == 2:
        return np.array([0, 0, 0, 0, 0, 0.5], dtype=np.float32)    # one live mode
    top = 2.0 if n == 3 else 30.0
    thr = float(default_threshold(M, top))
    if n == 3:
        lam = [-1.5 * thr, 0.0, 0.0, 0.0, 0.5 * thr, 1.5 * thr, 0.3, 1.1, top]
    else:
        edge = [-0.3 * top, -0.1 * top, -1.99 * thr, -1.5 * thr, -thr, -0.6 * thr, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5 * thr, thr,
                1.01 * thr, 1.5 * thr, 1.99 * thr]
        lam = edge + list(np.geomspace(0.02, top, M - len(edge)))
    lam = np.sort(np.asarray(lam, dtype=np.float64)).astype(np.float32)
    assert lam.shape == (M,) and float(lam[-1]) == top
    return lam


def synthetic_molecules(with_masses, seed=7):
    """[dict(n, lam [M] f32, modes [M, M] f32 (a seeded QR's orthonormal rows, rounded once), pos [n, 3] f32, masses [n] f32 or
    None)] for SYNTHETIC_SIZES; deterministic."""
    rng = np.random.default_rng(seed)
    out = []
    for n in SYNTHETIC_SIZES:
        M = 3 * n
        Q = np.linalg.qr(rng.standard_normal((M, M)))[0] if n else np.zeros((0, 0))
        pos = (1.5 * rng.standard_normal((n, 3))).astype(np.float32)
        m = rng.choice(np.array([1.008, 12.011, 15.999], dtype=np.float32), size=n)
        out.append(dict(n=n, lam=synthetic_spectrum(n) if n else np.zeros(0, dtype=np.float32),
                        modes=np.ascontiguousarray(Q.T).astype(np.float32), pos=pos, masses=m if with_masses else None))
    return out


def synthetic_draws(mols, S, seed=11):
    """[xi [S, M] f32] per molecule; the first rows are the same for every S (the leading draws of a longer run)"""
    out = []
    for k, mol in enumerate(mols):
        rng = np.random.default_rng([seed, k])
        out.append(rng.standard_normal((S, 3 * mol['n'])).astype(np.float32))
    return out
