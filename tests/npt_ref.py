"""fp64 statement of the two launches of constant-pressure dynamics (csrc/npt.hip: nnhip_npt_barostat, nnhip_npt_step) and of a host
loop of the scheme, for the tests (numpy), with first-order rounding bounds in the manner of tests/md_ref.py.

The kernels' chains are written out in include/newtonnet_hip.h; every line there is ONE fp32 rounding, which adds EPS32 |r| to the
bound of its result r (EPS32 = 2^-24), and the bounds of its operands pass through it multiplied by the magnitudes of the other
operands.  Three operations are not half an ulp: expf takes EXP_ULP = 2 ulp and the root SQRT_ULP = 2 ulp (the figures the header
states, more than twice what tools/probes/math_ulp_probe.hip measured on the device), one ulp of r being at most 2 EPS32 |r|; the
fp32 sum of n kinetic energies in an order this file does not restate takes md_ref.kinetic_sum_bound (n EPS32 sum |ke|).
C_MD = 2 multiplies the first-order sums for what first order leaves out, as in md_ref; TINY32 covers results below the normal range.

`barostat` and `npt_step` evaluate in fp64 from the SAME fp32 inputs the kernels get.  `host_loop` is the scheme itself in fp64
(no rounding model): the reference of the ensemble tests."""
import numpy as np

from tests import md_ref as mr

EPS32, C_MD, TINY32 = mr.EPS32, mr.C_MD, mr.TINY32
FINISH, BEGIN = mr.FINISH, mr.BEGIN
EXP_ULP = 2.0
SQRT_ULP = 2.0
ULP = 2.0 * EPS32                       # one ulp of r is at most 2 EPS32 |r|
THIRD32 = float(np.float32(1.0 / 3.0))  # the kernel's constant fl32(1/3) = 0x3eaaaaab
BAR = 1e5 * 1e-30 / 1.602176634e-19     # one bar in eV / Angstrom^3
K_BOLTZMANN = 8.617333262e-5


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _det(c):
    """det of c [3,3] by the kernel's chain and its first-order bound (the entries are exact)"""
    m, bm = [], []
    for (p, q, r, s) in (((1, 1), (2, 2), (1, 2), (2, 1)), ((1, 0), (2, 2), (1, 2), (2, 0)), ((1, 0), (2, 1), (1, 1), (2, 0))):
        t = c[r] * c[s]
        v = c[p] * c[q] - t
        m.append(v)
        bm.append(EPS32 * abs(t) + EPS32 * abs(v))
    t0 = c[0, 0] * m[0]
    b0 = abs(c[0, 0]) * bm[0] + EPS32 * abs(t0)
    t1 = -c[0, 1] * m[1] + t0
    b1 = abs(c[0, 1]) * bm[1] + b0 + EPS32 * abs(t1)
    V = c[0, 2] * m[2] + t1
    return V, abs(c[0, 2]) * bm[2] + b1 + EPS32 * abs(V)


def barostat(v, mass, mol_ptr, cell, virial, a, p0, F=None, hk=None, s2=None, xi=None, dv_in=0.0, dw_in=0.0):
    """One nnhip_npt_barostat launch.  v, F [N,3]; mass, hk [N]; mol_ptr [B+1]; cell, virial [B,3,3]; a, p0, s2, xi [B]: the fp32
    values the kernel gets (F with hk: the pending kick; s2 with xi: the noise).  dv_in: a bound of the input velocities; dw_in: a
    bound of every virial entry (a test that recomputes the virial).  Returns a dict of fp64 [B] arrays ke, volume, pressure,
    deps, mu, inv_mu and cell_out [B,3,3] with their bounds bke, bvolume, ... (C_MD x first order + TINY32)."""
    v, mass, cell, virial, a, p0 = _f64(v), _f64(mass), _f64(cell), _f64(virial), _f64(a), _f64(p0)
    F, hk, s2, xi = _f64(F), _f64(hk), _f64(s2), _f64(xi)
    assert (F is None) == (hk is None) and (s2 is None) == (xi is None)
    B = cell.shape[0]
    bv = np.zeros_like(v) + dv_in
    if F is not None:
        v = hk[:, None] * F + v
        bv = bv + EPS32 * np.abs(v)
    s = v[:, 0] * v[:, 0]
    bs = 2.0 * np.abs(v[:, 0]) * bv[:, 0] + EPS32 * np.abs(s)
    for k in (1, 2):
        s = v[:, k] * v[:, k] + s
        bs = bs + 2.0 * np.abs(v[:, k]) * bv[:, k] + EPS32 * np.abs(s)
    ke = 0.5 * mass * s
    bke = 0.5 * mass * bs + EPS32 * np.abs(ke)
    out = {k: np.zeros(B) for k in ('ke', 'volume', 'pressure', 'deps', 'mu', 'inv_mu', 'bke', 'bvolume', 'bpressure', 'bdeps', 'bmu',
                                    'binv_mu')}
    out['cell_out'], out['bcell_out'] = np.zeros((B, 3, 3)), np.zeros((B, 3, 3))
    for b in range(B):
        seg = slice(int(mol_ptr[b]), int(mol_ptr[b + 1]))
        K = ke[seg].sum()
        bK = bke[seg].sum() + mr.kinetic_sum_bound(ke[seg])
        V, bV = _det(cell[b])
        w = virial[b]
        t1 = w[0, 0] + w[1, 1]
        tr = t1 + w[2, 2]
        btr = 3.0 * dw_in + EPS32 * abs(t1) + EPS32 * abs(tr)
        num = 2.0 * K + tr
        bnum = 2.0 * bK + btr + EPS32 * abs(num)
        den = 3.0 * V
        bden = 3.0 * bV + EPS32 * abs(den)
        P = num / den
        bP = bnum / abs(den) + abs(num) * bden / den ** 2 + EPS32 * abs(P)
        diff = p0[b] - P
        bdiff = bP + EPS32 * abs(diff)
        if xi is not None:
            q = s2[b] / V
            bq = abs(q) * bV / abs(V) + EPS32 * abs(q)
            sd = np.sqrt(q)
            bsd = (bq / (2.0 * sd) if sd > 0 else 0.0) + SQRT_ULP * ULP * sd
            t = sd * xi[b]
            bt = abs(xi[b]) * bsd + EPS32 * abs(t)
            de = -a[b] * diff + t
            bde = a[b] * bdiff + bt + EPS32 * abs(de)
        elif a[b] == 0.0:
            de = bde = 0.0
        else:
            de = -a[b] * diff
            bde = a[b] * bdiff + EPS32 * abs(de)
        e = de * THIRD32
        be = THIRD32 * bde + EPS32 * abs(e)
        mu, inv_mu = np.exp(e), np.exp(-e)
        bmu, binv = mu * be + EXP_ULP * ULP * mu, inv_mu * be + EXP_ULP * ULP * inv_mu
        if xi is None and a[b] == 0.0:
            bmu = binv = 0.0                            # expf(+0) = 1 exactly
        co = mu * cell[b]
        for key, val, bound in (('ke', K, bK), ('volume', V, bV), ('pressure', P, bP), ('deps', de, bde), ('mu', mu, bmu),
                                ('inv_mu', inv_mu, binv), ('cell_out', co, np.abs(cell[b]) * bmu + EPS32 * np.abs(co))):
            out[key][b] = val
            out['b' + key][b] = C_MD * bound + TINY32
    return out


def npt_step(flags, x, v, F, hk, mu, inv_mu, mol, mass=None, sigma=None, xi=None, c1=1.0, dth=0.0, dv_in=0.0, dx_in=0.0, dmu_in=0.0,
             dinv_in=0.0):
    """One nnhip_npt_step launch: md_ref.md_step with  x = mu_b x_in, v = inv_mu_b v  between the begin kick and the first half
    drift (one rounding each).  mu, inv_mu [B] and mol [N] (the system of every atom); dmu_in, dinv_in [B] or numbers: bounds of mu
    and inv_mu (a test that chains the barostat's fp64 statement into this one).  Returns md_step's dict."""
    x, v, F, xi = _f64(x), _f64(v), _f64(F), _f64(xi)
    hk, sigma, mass = _f64(hk), _f64(sigma), _f64(mass)
    c1, dth = float(c1), float(dth)
    assert (sigma is None) == (xi is None)
    h = hk[:, None]
    bv = np.zeros_like(v) + dv_in
    bx = None
    ke = bke = None
    if flags & FINISH:
        v = h * F + v
        bv = bv + EPS32 * np.abs(v)
        if mass is not None:
            s = v[:, 0] * v[:, 0]
            bs = 2.0 * np.abs(v[:, 0]) * bv[:, 0] + EPS32 * np.abs(s)
            for k in (1, 2):
                s = v[:, k] * v[:, k] + s
                bs = bs + 2.0 * np.abs(v[:, k]) * bv[:, k] + EPS32 * np.abs(s)
            ke = 0.5 * mass * s
            bke = 0.5 * mass * bs + EPS32 * np.abs(ke)
    if flags & BEGIN:
        mol = np.asarray(mol, dtype=np.int64)
        m, im = _f64(mu)[mol][:, None], _f64(inv_mu)[mol][:, None]
        dm = (np.zeros(len(_f64(mu))) + dmu_in)[mol][:, None]
        dim = (np.zeros(len(_f64(mu))) + dinv_in)[mol][:, None]
        one = (m == 1.0) & (im == 1.0) & (dm == 0.0) & (dim == 0.0)       # a product with 1.0f is exact
        bx = np.zeros_like(x) + dx_in
        v = h * F + v
        bv = bv + EPS32 * np.abs(v)
        xs = m * x
        bx = np.abs(m) * bx + np.abs(x) * dm + np.where(one, 0.0, EPS32 * np.abs(xs))
        vs = im * v
        bv = np.abs(im) * bv + np.abs(v) * dim + np.where(one, 0.0, EPS32 * np.abs(vs))
        x, v = xs, vs
        x = dth * v + x
        bx = bx + dth * bv + EPS32 * np.abs(x)
        if xi is not None:
            t = c1 * v
            bt = abs(c1) * bv + EPS32 * np.abs(t)
            v = sigma[:, None] * xi + t
            bv = bt + EPS32 * np.abs(v)
        x = dth * v + x
        bx = bx + dth * bv + EPS32 * np.abs(x)
    return dict(x=x if flags & BEGIN else None, v=v, ke=ke, bx=None if bx is None else C_MD * bx + TINY32, bv=C_MD * bv + TINY32,
                bke=None if bke is None else C_MD * bke + TINY32)


def full_step(x, v, F0, F1, W0, cell, hk, mass, mol_ptr, mol, a, p0, s2=None, xi_b=None, sigma=None, xi=None, c1=1.0, dth=0.0,
              dw_in=0.0):
    """One whole constant-pressure step from a full-step state (x, v, cell) with the forces F0 and the virial W0 there: the barostat
    on the full-step velocities, BEGIN with F0 and its mu, FINISH with the forces F1 at the new geometry.  Returns dict(x, v, cell,
    bx, bv, bcell, baro: the barostat's dict); the bounds of each launch enter the next."""
    ba = barostat(v, mass, mol_ptr, cell, W0, a, p0, s2=s2, xi=xi_b, dw_in=dw_in)
    st = npt_step(BEGIN, x, v, F0, hk, ba['mu'], ba['inv_mu'], mol, None, sigma, xi, c1, dth, dmu_in=ba['bmu'] / C_MD,
                  dinv_in=ba['binv_mu'] / C_MD)
    fin = mr.md_step(FINISH, st['x'], st['v'], F1, hk, mass, dv_in=st['bv'] / C_MD)
    return dict(x=st['x'], v=fin['v'], cell=ba['cell_out'], bx=st['bx'], bv=fin['bv'], bcell=ba['bcell_out'], baro=ba)


# ---- the scheme in fp64, for the ensemble tests -------------------------------------------------------------------------------

def host_loop(n_sys, n_atoms, kT, p0, a, c1, n_burn, n_snap, every, seed, v0_volume=None):
    """Ideal gas (zero forces and virial) of n_sys independent systems of n_atoms unit-mass atoms under the scheme, fp64:
    per step  K = sum v^2 / 2;  P = 2 K / (3 V);  d eps = -a (p0 - P) + sqrt(2 kT a / V) xi;  V <- V exp(d eps);
    v <- v exp(-d eps / 3);  v <- c1 v + sqrt((1 - c1^2) kT) xi'   (the two half kicks and the drifts move nothing that P sees).
    Returns the volumes [n_snap, n_sys] at the steps n_burn + every, n_burn + 2 every, ..."""
    rng = np.random.default_rng(seed)
    V = np.full(n_sys, (n_atoms + 1) * kT / p0 if v0_volume is None else v0_volume, dtype=np.float64)
    v = rng.standard_normal((n_sys, n_atoms, 3)) * np.sqrt(kT)
    sig = np.sqrt((1.0 - c1 * c1) * kT)
    snaps = []
    for k in range(1, n_burn + n_snap * every + 1):
        K = 0.5 * (v * v).sum(axis=(1, 2))
        P = 2.0 * K / (3.0 * V)
        de = -a * (p0 - P) + np.sqrt(2.0 * kT * a / V) * rng.standard_normal(n_sys)
        V = V * np.exp(de)
        v = v * np.exp(-de / 3.0)[:, None, None]
        v = c1 * v + sig * rng.standard_normal(v.shape)
        if k > n_burn and (k - n_burn) % every == 0:
            snaps.append(V.copy())
    return np.asarray(snaps)


def mean_and_standard_error(snaps):
    """(mean, standard error) of the volumes [n_snap, n_sys]: the systems are independent, the snapshots of one system are not, so
    the error is taken across the per-system means"""
    per_system = snaps.mean(axis=0)
    return float(per_system.mean()), float(per_system.std(ddof=1) / np.sqrt(per_system.size))
