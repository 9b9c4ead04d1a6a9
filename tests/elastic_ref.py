"""fp64 statement of the elastic constants for the tests, on the pieces of tests/hessian_ref.oracle_energy: the oracle's edge list
is built ONCE at zero strain, its displacement vectors are moved as d_e -> (1 + eps(e)) d_e + u_i - u_j (u a displacement of the
atoms in the laboratory frame, so that dE/du at u = 0 is dE/dpos of the strained crystal, the gradient the model returns, and
Lambda is its strain derivative: the Hessian-vector product along eps pos for a molecule), and plain double backward gives
    born V = d^2E/de de,   Lambda = d^2E/dpos de,   H = d^2E/dpos dpos.
Voigt order xx, yy, zz, yz, xz, xy with engineering shears.  Also the planted inputs of the fold / relaxation stage test and the
test crystals.  Independent of the package: nothing here imports newtonnet_amd."""
import numpy as np
import torch

from oracle import newtonnet_ref as ref
from tests import phonon_ref as pr

EPS32 = 2.0 ** -24
VOIGT_PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
GPA_PER_EV_A3 = 160.21766

# the crystals of tests/test_hip_phonons.py (E2E_*): two primitive cells whose lattice matrices are symmetric
E2E_CELLS = np.array([[[4.2, 0.4, -0.3], [0.4, 4.1, 0.5], [-0.3, 0.5, 4.3]],
                      [[4.3, -0.2, 0.3], [-0.2, 4.2, -0.4], [0.3, -0.4, 4.1]]])
E2E_Z = np.array([6, 1, 8, 1, 1])
E2E_POS = np.array([[0.4, 0.5, 0.3], [1.3, 1.1, 1.0], [0.6, 0.4, 0.5], [1.4, 0.9, 0.8], [0.1, 1.2, 0.2]])
E2E_BATCH = np.array([0, 0, 1, 1, 1])
E2E_RANGES = ((0, 2), (2, 5))
E2E_S = (3, 3, 3)


def voigt_matrix(e):
    """eps [3,3] of Voigt components e [6] (torch, differentiable)"""
    h = 0.5
    return torch.stack([torch.stack([e[0], h * e[5], h * e[4]]), torch.stack([h * e[5], e[1], h * e[3]]),
                        torch.stack([h * e[4], h * e[3], e[2]])])


def voigt_of(eps):
    """Voigt components [6] of a symmetric numpy [3,3]"""
    return np.array([eps[a, b] if a == b else eps[a, b] + eps[b, a] for a, b in VOIGT_PAIRS])


CUBIC_CELLS = np.array([4.2 * np.eye(3), 4.3 * np.eye(3)])   # the same atoms in cells that commute with every strain


def supercell(b, dtype=torch.float64, cells=E2E_CELLS):
    """(z, pos, cell [1,3,3], batch) of the 3 x 3 x 3 supercell of test crystal b, positions and cell rounded to fp32 once (what
    the device sees) and then widened to `dtype`."""
    lo, hi = E2E_RANGES[b]
    pos32 = torch.tensor(E2E_POS[lo:hi], dtype=torch.float32).double().numpy()
    cell32 = torch.tensor(cells[b], dtype=torch.float32).double().numpy()
    zs, ps, cs = pr.build_supercell(E2E_Z[lo:hi], pos32, cell32, E2E_S)
    return (torch.tensor(zs), torch.tensor(ps, dtype=torch.float32).to(dtype), torch.tensor(cs, dtype=torch.float32).to(dtype)[None],
            torch.zeros(len(zs), dtype=torch.long))


def supercell_batch(dtype=torch.float64, cells=E2E_CELLS):
    """both supercells (54 and 81 atoms) as one batch: z, pos, cell [2,3,3], batch"""
    parts = [supercell(b, dtype, cells) for b in range(2)]
    return (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]),
            torch.cat([p[3] + b for b, p in enumerate(parts)]))


def periodic_strains(seed=3):
    """[7, 2, 6] Voigt strains of the periodic test: the six unit strains (both systems alike) and one random symmetric strain per
    system"""
    rng = np.random.default_rng(seed)
    unit = np.repeat(np.eye(6)[:, None, :], 2, axis=1)
    x = rng.standard_normal((2, 3, 3))
    rand = np.stack([voigt_of(0.5 * (m + m.T)) for m in x])
    return np.concatenate([unit, rand[None]])


class StrainedOracle:
    """E(u, e) of one batch with the edge list frozen at (pos, e = 0): d_e(u, e) = (1 + eps(e_b)) d_e + u_i - u_j.  (Straining u
    as well, d_e = (1 + eps)(d_e + u_i - u_j), would add eps^T dE/dpos to Lambda: the two agree where the forces vanish.)"""

    def __init__(self, sd, z, pos, cell, batch, cutoff=5.0, dtype=torch.float64):
        self.sd = {k: v.to(dtype) for k, v in sd.items()}
        self.z, self.batch, self.cutoff, self.dtype = z, batch, cutoff, dtype
        self.n_mol = cell.shape[0]
        self.pos = pos.detach().to(dtype)
        self.edge_index, disp = ref.radius_graph(self.pos, cell.detach().to(dtype), batch, cutoff)
        self.disp = disp.detach()

    def energy(self, u, e):
        """energy [B]; u [N,3] position displacement, e [B,6] Voigt strain"""
        ei = self.edge_index
        eps = torch.stack([voigt_matrix(e[b]) for b in range(self.n_mol)])[self.batch[ei[0]]]
        d = self.disp + torch.bmm(eps, self.disp.unsqueeze(-1)).squeeze(-1) + u[ei[0]] - u[ei[1]]
        freq = self.sd['embedding_layers.edge_embedding.embedding.frequencies']
        dist_edge, dir_edge = ref.edge_features(d, self.cutoff, freq)
        atom_node = self.sd['embedding_layers.node_embedding.weight'][self.z]
        force_node = torch.zeros(self.z.shape[0], 3, atom_node.shape[1], dtype=self.dtype)
        for l in range(ref.n_layers(self.sd)):
            atom_node, force_node = ref.interaction(self.sd, l, atom_node, force_node, dir_edge, dist_edge, ei)
        return ref.energy_head(self.sd, 0, atom_node, self.z, self.batch, self.n_mol)[0]

    def variables(self):
        u = torch.zeros_like(self.pos).requires_grad_(True)
        e = torch.zeros(self.n_mol, 6, dtype=self.dtype).requires_grad_(True)
        return u, e

    def first(self):
        """(dE/de [B,6], dE/dpos [N,3]) at zero strain, fp64"""
        u, e = self.variables()
        ge, gu = torch.autograd.grad(self.energy(u, e).sum(), (e, u))
        return ge.double(), gu.double()

    def strain_tangent(self, eta):
        """(dgrad [N,3], d2 [B,6]) along the Voigt strains eta [B,6]: what hessian.strain_vector_product returns"""
        u, e = self.variables()
        ge, gu = torch.autograd.grad(self.energy(u, e).sum(), (e, u), create_graph=True)
        w = ((ge * eta.to(self.dtype)).sum())
        d2, dgrad = torch.autograd.grad(w, (e, u))
        return dgrad.double(), d2.double()

    def second(self, home):
        """(born V [B,6,6], Lambda [N,3,B,6] -> its diagonal-in-system part [N,3,6], H columns of the `home` atoms [len(home),3,N,3])"""
        u, e = self.variables()
        ge, gu = torch.autograd.grad(self.energy(u, e).sum(), (e, u), create_graph=True)
        bv = torch.zeros(self.n_mol, 6, 6, dtype=torch.float64)
        lam = torch.zeros(self.pos.shape[0], 3, 6, dtype=torch.float64)
        for b in range(self.n_mol):
            for J in range(6):
                d2, dg = torch.autograd.grad(ge[b, J], (e, u), retain_graph=True)
                bv[b, :, J] = d2[b].double()
                lam[:, :, J] += dg.double() * (self.batch == b)[:, None]
        H = torch.zeros(len(home), 3, self.pos.shape[0], 3, dtype=torch.float64)
        for k, i in enumerate(home):
            for a in range(3):
                (h,) = torch.autograd.grad(gu[i, a], u, retain_graph=True)
                H[k, a] = h.double()
        return bv, lam, H


def gamma_force_constants(H, n):
    """Phi0 [3n,3n] fp64 (numpy) from the home columns H [n,3,N,3]: summed over the copies of every atom, symmetrised, with the
    acoustic sum rule of phonons.acoustic_sum_rule applied to the supercell force constants first"""
    phi = np.array(H, dtype=np.float64)
    for i in range(n):
        blk = phi[i, :, i, :] - phi[i].sum(axis=1)
        phi[i, :, i, :] = 0.5 * (blk + blk.T)
    N = phi.shape[2]
    p0 = phi.reshape(n, 3, N // n, n, 3).sum(axis=2).reshape(3 * n, 3 * n)
    return 0.5 * (p0 + p0.T)


def pinv_nonacoustic(phi0, n_null=3):
    """(pseudo-inverse of a symmetric matrix over all but its n_null eigenvalues of smallest magnitude, eigenvalues)"""
    w, q = np.linalg.eigh(phi0)
    keep = np.argsort(np.abs(w))[n_null:]
    return (q[:, keep] / w[keep][None, :]) @ q[:, keep].T, w


def elastic_reference(sd, b):
    """dict of the fp64 reference of test crystal b: born, relaxation, C [6,6] (eV / A^3), lam [3n,6], phi0, volume, plus the
    supercell quantities bornV [6,6] and lam_sc [N,3,6]"""
    z, pos, cell, batch = supercell(b)
    n = E2E_RANGES[b][1] - E2E_RANGES[b][0]
    o = StrainedOracle(sd, z, pos, cell, batch)
    bv, lam_sc, H = o.second(range(n))
    v_sc = abs(np.linalg.det(cell[0].numpy()))
    v = v_sc / np.prod(E2E_S)
    born = bv[0].numpy() / v_sc
    born = 0.5 * (born + born.T)
    lam = lam_sc[:n].numpy().reshape(3 * n, 6)
    phi0 = gamma_force_constants(H.numpy(), n)
    pinv, w = pinv_nonacoustic(phi0)
    relaxation = lam.T @ pinv @ lam / v
    return dict(born=born, relaxation=relaxation, C=born - relaxation, lam=lam, phi0=phi0, evals=w, volume=v, bornV=bv[0].numpy(),
                lam_sc=lam_sc.numpy(), H=H.numpy())


# ---- planted inputs of the fold / relaxation stage test ---------------------------------------------------------------------------

def planted_phi0(n, seed, kappa=100.0, n_null=3, negative=False):
    """(Phi0 [3n,3n], Lambda [3n,6]) fp64: Phi0 = Q diag(lambda) Q^T with the three translations as exact null vectors (n_null = 4
    adds one more null direction), the other eigenvalues log-spaced over [1, kappa] (the smallest negated with negative=True);
    Lambda random with zero column sums over the atoms (translation invariance)."""
    rng = np.random.default_rng(seed)
    d = 3 * n
    T = np.zeros((d, 3))
    for a in range(3):
        T[a::3, a] = 1.0 / np.sqrt(n)
    X = rng.standard_normal((d, d))
    X -= T @ (T.T @ X)
    Q, _ = np.linalg.qr(np.concatenate([T, X], axis=1)[:, :d])
    live = d - n_null
    lam = np.zeros(d)
    if live > 0:
        lam[n_null:] = np.logspace(0.0, np.log10(kappa), live) if live > 1 else [1.0]
        if negative:
            lam[n_null] = -lam[n_null]
    phi0 = (Q * lam[None, :]) @ Q.T
    L = rng.standard_normal((n, 3, 6))
    L -= L.mean(axis=0, keepdims=True)
    return 0.5 * (phi0 + phi0.T), L.reshape(d, 6)


def spread_over_copies(phi0, n, copies, seed):
    """force constants [n,3,n copies,3] fp64 whose sum over the copies is phi0 [3n,3n]: random parts that cancel"""
    rng = np.random.default_rng(seed)
    p = phi0.reshape(n, 3, n, 3)
    parts = rng.standard_normal((copies, n, 3, n, 3))
    parts -= parts.mean(axis=0, keepdims=True)
    parts += p[None] / copies
    return np.ascontiguousarray(parts.transpose(1, 2, 0, 3, 4).reshape(n, 3, copies * n, 3))


def relaxation_reference(phi0, lam, thr):
    """(R [6,6], n_zero, n_negative) fp64 over the modes with |lambda| > thr"""
    w, q = np.linalg.eigh(np.asarray(phi0, dtype=np.float64))
    keep = np.abs(w) > thr
    p = q[:, keep].T @ np.asarray(lam, dtype=np.float64)
    return (p.T / w[keep][None, :]) @ p, int((~keep).sum()), int((w[keep] < 0).sum())


def planted_eigenpairs(d, seed, n_zero=3, negative=False, kappa=100.0):
    """(evals fp32 [d] ascending, Q fp32 [d,d] with ROW m = mode m, Lambda fp32 [d,6]) as nnhip_elastic_relax takes them: Q an
    orthogonal matrix from a QR rounded to fp32, n_zero exact zeros among the eigenvalues, the others log-spaced over [1, kappa]
    (the smallest negated with negative=True)"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    ev = np.zeros(d)
    live = d - n_zero
    if live > 0:
        ev[n_zero:] = np.logspace(0.0, np.log10(kappa), live) if live > 1 else [1.0]
        if negative:
            ev[n_zero] = -ev[n_zero]
    ev = np.sort(ev)
    return ev.astype(np.float32), np.ascontiguousarray(Q.T.astype(np.float32)), rng.standard_normal((d, 6)).astype(np.float32)


def relaxation_from_eigenpairs(evals, modes, lam, thr):
    """(R [6,6], n_zero, n_negative, bound [6,6]) fp64 of nnhip_elastic_relax on the eigenpairs GIVEN (evals [d], modes [d,d] with
    row m = mode m, lam [d,6]; nothing is diagonalised): R = sum over the modes with |lambda| > thr (a NaN is not) of
    p_m p_m^T / lambda_m, p_m = q_m . Lambda.  bound: the rounding of R to fp32 plus d 2^-52 of the sum of the term magnitudes
    (sum_c |q| |Lambda_I|)(sum_c |q| |Lambda_J|) / |lambda| -- the kernel sums in fp64."""
    ev = np.asarray(evals, dtype=np.float64).reshape(-1)
    Q = np.asarray(modes, dtype=np.float64).reshape(len(ev), len(ev))
    L = np.asarray(lam, dtype=np.float64).reshape(len(ev), 6)
    keep = np.abs(ev) > float(thr)                     # False for a NaN
    R, T = np.zeros((6, 6)), np.zeros((6, 6))
    for m in np.nonzero(keep)[0]:
        p, a = Q[m] @ L, np.abs(Q[m]) @ np.abs(L)
        R += np.outer(p, p) / ev[m]
        T += np.outer(a, a) / abs(ev[m])
    return R, int((~keep).sum()), int((ev[keep] < 0).sum()), EPS32 * np.abs(R) + len(ev) * 2.0 ** -52 * T


def cubic_moduli(c11, c12, c44):
    """(K, G_V, G_R) of a cubic crystal"""
    return (c11 + 2.0 * c12) / 3.0, (c11 - c12 + 3.0 * c44) / 5.0, 5.0 * (c11 - c12) * c44 / (4.0 * c44 + 3.0 * (c11 - c12))


def cubic_matrix(c11, c12, c44):
    C = np.zeros((6, 6))
    C[:3, :3] = c12
    C[np.arange(3), np.arange(3)] = c11
    C[np.arange(3, 6), np.arange(3, 6)] = c44
    return C
