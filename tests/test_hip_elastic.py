"""Analytic elastic constants on the device (newtonnet_amd/elastic.py, hessian.strain_vector_product, csrc/elastic.hip) against the
fp64 yardstick of tests/elastic_ref.py: the strain tangent pass on molecules (where it is a Hessian-vector product) and on
periodic supercells, the replica scheme, the fold and relaxation kernels on planted inputs, and the whole chain.

Error models.
  dgrad (Lambda): the project's Hessian form, max <= 1e-4 scale and mean <= 1e-5 scale, scale = the largest reference magnitude.
  d2 (Born sums): 4 x the error of the SAME double backward run in fp32 through the oracle (per system, the largest over the
    strains and components), the project's yardstick of what fp32 can give.
  R (relaxation kernel): STAGE_C kappa d eps32 max |R| -- the pseudo-inverse over the live modes has norm kappa / ||Phi0||, the
    solver perturbs Phi0 by d eps32 ||Phi0||.  STAGE_C = 4 x the largest measured ratio (see STAGE_C below)."""
import numpy as np
import pytest
import torch

from newtonnet_amd import elastic as el
from newtonnet_amd import hessian as nh
from newtonnet_amd import phonons as ph
from tests import elastic_ref as er
from tests import hessian_ref as hr
from tests import util
from tests.test_hip_hessian import make_model

pytestmark = pytest.mark.gpu

EPS32 = er.EPS32
# measured |R - R_ref| / (kappa d eps32 max |R|) on the planted cases of test_stage_fold_and_relaxation (kappa = 100):
# n_b = 1: 0 (R = 0), 2: 0.0195, 11: 0.0181, 32: 0.0462, negative mode (n_b = 5): 0.0224, four null modes (n_b = 4): 0.0995.
# STAGE_C = 4 x the largest.
STAGE_C = 0.4
KAPPA = 100.0


def cuda(*ts):
    return [t.cuda() for t in ts]


# ---- 1. molecules ------------------------------------------------------------------------------------------------------------------

def test_strain_vp_on_molecules_is_the_hvp_along_eta_pos():
    """cell = 0: dd_e = eta (pos_i - pos_j) = v_i - v_j with v_i = eta_b pos_i, so dgrad = H v.  The two device results differ only
    in how tgeo was rounded -- the strain pass forms dd_e from the edge, the HVP from a direction that was rounded to fp32 per
    atom (the aspirin sits 30 A from the origin, so |v_i| is ten times |dd_e|) -- and each may err against fp64 as the HVP does.
    Allowed between them, per molecule: the HVP's own measured error against the oracle's column combination H_ref v, with v
    the exact direction eta pos in fp64, the one the identity is about (a wrong system index or Voigt convention is an O(1)
    difference)."""
    sd = util.load_state('rand')
    z, pos, cell, batch = hr.ethanol_and_aspirin()
    model = make_model(sd)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 3, 3))
    eta = torch.tensor(0.5 * (x + x.transpose(0, 2, 1)), dtype=torch.float32)
    assert not torch.allclose(eta[0], eta[1])
    v64 = torch.bmm(eta.double()[batch], pos.double().unsqueeze(-1)).squeeze(-1)
    v = v64.float()                                                    # rounded once: the best direction the HVP can be given
    dgrad, d2 = model.strain_vector_product(*cuda(z, pos, cell, batch), eta.cuda())
    hv = model.hessian_vector_product(*cuda(z, pos, cell, batch, v))
    assert dgrad.shape == (30, 3) and d2.shape == (2, 6) and dgrad.dtype == torch.float32
    H = hr.oracle_hessian(sd, z, pos.double(), cell.double(), batch).reshape(90, 90)
    want = (H @ v64.reshape(-1)).reshape(30, 3)
    voigt, _ = model.strain_vector_product(*cuda(z, pos, cell, batch), nh.voigt_strain(eta, 2).cuda())
    assert torch.equal(voigt, dgrad)                                   # [B,6] and [B,3,3] are one path
    for m in range(2):
        sel = batch == m
        tol = (hv.cpu().double()[sel] - want[sel]).abs().max().item()
        diff = (dgrad.cpu().double()[sel] - hv.cpu().double()[sel]).abs().max().item()
        own = (dgrad.cpu().double()[sel] - want[sel]).abs().max().item()
        scale = want[sel].abs().max().item()
        print(f'molecule {m}: |strain VP - HVP| {diff:.3e}, HVP error {tol:.3e}, strain VP error {own:.3e}, scale {scale:.3e}')
        assert diff <= tol
    # the other system's strain does not leak: zero strain on the aspirin leaves its rows exactly zero
    eta0 = eta.clone()
    eta0[1] = 0.0
    g0, s0 = model.strain_vector_product(*cuda(z, pos, cell, batch), eta0.cuda())
    assert torch.count_nonzero(g0[9:]) == 0 and torch.count_nonzero(s0[1]) == 0 and torch.equal(g0[:9], dgrad[:9])
    # d2 of a molecule against fp64, same yardstick as the periodic test
    o64 = er.StrainedOracle(sd, z, pos, cell, batch)
    o32 = er.StrainedOracle(sd, z, pos, cell, batch, dtype=torch.float32)
    e6 = nh.voigt_strain(eta, 2).double()
    ref2, yard = o64.strain_tangent(e6)[1], o32.strain_tangent(e6)[1]
    for m in range(2):
        tol = 4.0 * (yard[m] - ref2[m]).abs().max().item()
        err = (d2.cpu().double()[m] - ref2[m]).abs().max().item()
        print(f'molecule {m}: d2 error {err:.3e}, allowed {tol:.3e} (4 x the fp32 oracle), scale {ref2[m].abs().max().item():.3e}')
        assert err <= tol


# ---- 2./3. periodic supercells -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def periodic():
    sd = util.load_state('rand')
    model = make_model(sd)
    args = er.supercell_batch(torch.float32)
    o64 = er.StrainedOracle(sd, *er.supercell_batch())
    o32 = er.StrainedOracle(sd, *er.supercell_batch(), dtype=torch.float32)
    strains = torch.tensor(er.periodic_strains())
    ref = [o64.strain_tangent(s) for s in strains]
    yard = [o32.strain_tangent(s)[1] for s in strains]
    d2_tol = [4.0 * max((y[b] - r[1][b]).abs().max().item() for y, r in zip(yard, ref)) for b in range(2)]
    return dict(sd=sd, model=model, args=args, strains=strains, ref=ref, d2_tol=d2_tol)


def test_periodic_strain_vp_against_fp64(periodic):
    model, (z, pos, cell, batch) = periodic['model'], periodic['args']
    assert torch.bincount(batch).tolist() == [54, 81]
    worst = [0.0, 0.0]
    for k, (s, (want_g, want_2)) in enumerate(zip(periodic['strains'], periodic['ref'])):
        dgrad, d2 = model.strain_vector_product(*cuda(z, pos, cell, batch), s.float().cuda())
        dgrad, d2 = dgrad.cpu().double(), d2.cpu().double()
        for b in range(2):
            sel = batch == b
            scale = want_g[sel].abs().max().item()
            d = (dgrad[sel] - want_g[sel]).abs()
            err2 = (d2[b] - want_2[b]).abs().max().item()
            worst[b] = max(worst[b], err2)
            print(f'strain {k} system {b}: dgrad max {d.max().item():.3e} mean {d.mean().item():.3e} of {scale:.3e}; '
                  f'd2 error {err2:.3e} of {want_2[b].abs().max().item():.3e}, allowed {periodic["d2_tol"][b]:.3e}')
            assert d.max().item() <= 1e-4 * scale and d.mean().item() <= 1e-5 * scale
            assert err2 <= periodic['d2_tol'][b]
            # translation invariance, and the copies of a home atom carry its Lambda
            assert dgrad[sel].sum(dim=0).abs().max().item() <= 1e-4 * scale
            n = (2, 3)[b]
            img = dgrad[sel].reshape(27, n, 3)
            assert (img - img[:1]).abs().max().item() <= 1e-4 * scale
    print(f'd2: worst error {worst[0]:.3e} / {worst[1]:.3e}, allowed {periodic["d2_tol"][0]:.3e} / {periodic["d2_tol"][1]:.3e}')


def test_replicas_and_repeatability(periodic):
    model, args = periodic['model'], cuda(*periodic['args'])
    tol = torch.tensor(periodic['d2_tol'])[:, None, None]
    base, lam = el.born_pass(model, *args, replicas=1)
    again, lam2 = el.born_pass(model, *args, replicas=1)
    assert torch.equal(base, again) and torch.equal(lam, lam2)
    want = torch.stack([torch.stack([periodic['ref'][J][1][b] for J in range(6)], dim=1) for b in range(2)])     # [b, I, J]
    assert ((base.cpu().double() - want).abs() <= tol).all()
    for R in (2, 3, 6):
        d2, lr = el.born_pass(model, *args, replicas=R)
        diff = (d2 - base).abs().cpu().double()
        print(f'replicas {R}: max |d d2| {diff.max().item():.3e}, max |d Lambda| {(lr - lam).abs().max().item():.3e}')
        assert (diff <= tol).all()
        # a replica is the same rows through the same kernels: the Born sums and Lambda keep every bit
        assert torch.equal(d2, base) and torch.equal(lr, lam)
    asym = (base - base.transpose(1, 2)).abs().cpu().double().amax(dim=(1, 2))
    print(f'asymmetry of the Born sums: {asym.tolist()}, allowed {periodic["d2_tol"]}')
    assert (asym <= tol.reshape(-1)).all()
    assert nh.replicas_for(135, 6) == 6 and el.born_pass(model, *args)[0].equal(el.born_pass(model, *args, replicas=6)[0])


# ---- 4. the fold and relaxation kernels on planted inputs ----------------------------------------------------------------------------

def planted(n, seed, copies=(2, 1, 2), **kw):
    phi0, lam = er.planted_phi0(n, seed, kappa=KAPPA, **kw)
    fc = er.spread_over_copies(phi0, n, int(np.prod(copies)), seed).astype(np.float32)
    rng = np.random.default_rng(seed)
    return fc, lam.astype(np.float32), rng.uniform(0.0, 6.0, (n, 3)), 6.0 * np.eye(3), copies


def run_stage(cases):
    """the cases as ONE batch through nnhip_elastic_fold, eig_blocks and nnhip_elastic_relax"""
    counts = [len(c[2]) for c in cases]
    p = ph.Phonons.from_force_constants([c[0] for c in cases], np.ones(sum(counts), dtype=np.int64), np.concatenate([c[2] for c in cases]),
                                        np.stack([c[3] for c in cases]), np.array([c[4] for c in cases]),
                                        batch=np.repeat(np.arange(len(cases)), counts), device='cuda')
    phi0 = el.fold_force_constants(p)
    lam = torch.tensor(np.concatenate([c[1] for c in cases]), dtype=torch.float32, device='cuda')
    R, n_zero, n_neg, status = el.relaxation_term(phi0, p.out_ptr, counts, lam)
    out, o, a = [], 0, 0
    for n in counts:
        out.append((phi0[o:o + 9 * n * n].cpu().numpy().reshape(3 * n, 3 * n), lam[3 * a:3 * a + 3 * n].cpu().numpy()))
        o, a = o + 9 * n * n, a + n
    return out, R.cpu().numpy(), n_zero.cpu().tolist(), n_neg.cpu().tolist(), status.cpu().tolist()


def check_stage(case, dev, R, what):
    fc, lam32, _, _, copies = case
    n, d, c = len(lam32) // 3, len(lam32), int(np.prod(copies))
    phi_dev, lam_dev = dev
    # the fold: fp64 sums rounded once, and exactly symmetric
    s = fc.astype(np.float64).reshape(n, 3, c, n, 3).sum(axis=2).reshape(d, d)
    want = 0.5 * (s + s.T)
    assert np.array_equal(phi_dev, phi_dev.T), f'{what}: Phi0 not exactly symmetric'
    terms = np.abs(fc.astype(np.float64)).reshape(n, 3, c, n, 3).sum(axis=2).reshape(d, d)
    assert np.all(np.abs(phi_dev - want) <= EPS32 * np.abs(want) + 2.0 ** -52 * c * (terms + terms.T)), f'{what}: fold'
    w = np.linalg.eigvalsh(phi_dev.astype(np.float64))
    thr = 8.0 * EPS32 * d * np.abs(w).max()
    R_ref, nz, nn = er.relaxation_reference(phi_dev, lam_dev, thr)
    scale = np.abs(R_ref).max()
    bound = STAGE_C * KAPPA * d * EPS32 * scale
    err = np.abs(R.astype(np.float64) - R_ref).max()
    ratio = err / (KAPPA * d * EPS32 * scale) if scale > 0 else 0.0
    print(f'{what}: |dR| {err:.3e} of {scale:.3e}, ratio to kappa d eps32 max|R| = {ratio:.4f} (allowed {STAGE_C})')
    assert np.array_equal(R, R.T) and err <= bound, f'{what}: |dR| {err:.3e} above {bound:.3e}'
    return nz, nn


def test_stage_fold_and_relaxation():
    cases = [planted(n, seed=40 + n) for n in (1, 2, 11, 32)]
    cases.append(planted(5, seed=51, negative=True))
    cases.append(planted(4, seed=52, n_null=4))
    dev, R, n_zero, n_neg, status = run_stage(cases)
    names = ['n_b = 1', 'n_b = 2', 'n_b = 11', 'n_b = 32', 'negative mode', 'four null modes']
    for k, (case, name) in enumerate(zip(cases, names)):
        nz, nn = check_stage(case, dev[k], R[k], name)
        assert (n_zero[k], n_neg[k]) == (nz, nn), f'{name}: counts {n_zero[k]}, {n_neg[k]} against {nz}, {nn}'
        assert status[k] == (el.STATUS_ZERO if nz != 3 else 0) | (el.STATUS_NEGATIVE if nn else 0)
    assert n_zero[1:4] == [3, 3, 3] and status[1:4] == [0, 0, 0]
    assert n_neg[4] == 1 and status[4] == el.STATUS_NEGATIVE
    assert n_zero[5] == 4 and status[5] == el.STATUS_ZERO
    # a crystal alone gives what it gives in the batch, bit for bit
    _, R1, _, _, _ = run_stage([cases[2]])
    assert np.array_equal(R1[0], R[2])


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def e2e(periodic):
    sd, model = periodic['sd'], periodic['model']
    z, batch = torch.tensor(er.E2E_Z), torch.tensor(er.E2E_BATCH)
    pos, cell = torch.tensor(er.E2E_POS, dtype=torch.float32), torch.tensor(er.E2E_CELLS, dtype=torch.float32)
    args = cuda(z, pos, cell, batch)
    return dict(model=model, args=args, res=model.elastic_constants(*args, supercell=er.E2E_S),
                ref=[er.elastic_reference(sd, b) for b in range(2)], d2_tol=periodic['d2_tol'])


def test_end_to_end_against_fp64(e2e):
    """born: the Born sums' tolerance over the supercell volume.  Lambda: the Hessian form.  relaxation: with a_J = pinv(Phi0)
    Lambda_J (fp64 reference),  dR_IJ = dLambda_I . a_J + a_I . dLambda_J - a_I dPhi0 a_J  to first order, so
        |dR_IJ| <= tol_L (|a_I|_1 + |a_J|_1) + |a_I|_1 |a_J|_1 tol_Phi + STAGE_C kappa d eps32 max |R|
    with tol_L = 1e-4 max |Lambda| and tol_Phi = 27 x 1e-4 max |H| (test 2's model, the project's Hessian form, on Lambda and on
    the force constants: an entry of Phi0 sums 27 of them), and kappa d eps32 the relaxation kernel's model (test 4) at the
    crystal's own kappa.  The fp64 fold of the device's force constants is asserted against tol_Phi before it is carried.
    C: the sum of the born and relaxation bounds.  Figures: not measured."""
    res, model, args = e2e['res'], e2e['model'], e2e['args']
    assert res.C.shape == (2, 6, 6) and res.counts == [2, 3] and res.internal_strain.shape == (15, 6)
    phon = model.phonons(*args, supercell=er.E2E_S)
    off = 0
    for b in range(2):
        r, n = e2e['ref'][b], (2, 3)[b]
        d, v, v_sc = 3 * n, r['volume'], r['volume'] * 27
        assert abs(float(res.volume[b]) - v) <= 4 * EPS32 * v       # the reference's supercell lattice is 3 x cell rounded to fp32 again
        tol_born = e2e['d2_tol'][b] / v_sc
        err_born = np.abs(res.born[b].cpu().double().numpy() - r['born']).max()
        lam = res.internal_strain[off:off + d].cpu().double().numpy()
        off += d
        tol_l = 1e-4 * np.abs(r['lam']).max()
        err_l = np.abs(lam - r['lam'])
        assert err_l.max() <= tol_l and err_l.mean() <= 0.1 * tol_l
        fc = phon.force_constants(b).cpu().double().numpy()
        p0 = fc.reshape(n, 3, 27, n, 3).sum(axis=2).reshape(d, d)
        dphi = np.abs(0.5 * (p0 + p0.T) - r['phi0']).max()
        tol_phi = 27 * 1e-4 * np.abs(r['H']).max()
        pinv, w = er.pinv_nonacoustic(r['phi0'])
        aw = np.sort(np.abs(w))
        kappa = aw[-1] / aw[3]
        a1 = np.abs(pinv @ r['lam']).sum(axis=0)                                 # |a_J|_1
        scale_r = np.abs(r['relaxation']).max() * v
        tol_r = (tol_l * (a1[:, None] + a1[None, :]) + a1[:, None] * a1[None, :] * tol_phi + STAGE_C * kappa * d * EPS32 * scale_r) / v
        err_r = np.abs(res.relaxation[b].cpu().double().numpy() - r['relaxation'])
        err_c = np.abs(res.C[b].cpu().double().numpy() - r['C'])
        print(f'crystal {b}: born error {err_born:.3e} (allowed {tol_born:.3e}) of {np.abs(r["born"]).max():.3e}; Lambda max '
              f'{err_l.max():.3e} mean {err_l.mean():.3e} of {np.abs(r["lam"]).max():.3e}; kappa {kappa:.1f}, |dPhi0| {dphi:.3e} (allowed {tol_phi:.3e}); '
              f'relaxation error {err_r.max():.3e} (allowed up to {tol_r.max():.3e}) of {np.abs(r["relaxation"]).max():.3e}; C error '
              f'{err_c.max():.3e}; status {int(res.status[b])}, n_zero {int(res.n_zero[b])}, n_negative {int(res.n_negative[b])}')
        assert err_born <= tol_born and dphi <= tol_phi
        assert np.all(err_r <= tol_r)
        assert np.all(err_c <= tol_born + tol_r)
        assert int(res.n_zero[b]) == 3 and int(res.n_negative[b]) == int((r['evals'] < -1e-6).sum())
        assert int(res.status[b]) == (el.STATUS_NEGATIVE if int(res.n_negative[b]) else 0)
        assert float(res.asymmetry[b]) <= tol_born
    assert torch.equal(res.C, res.C.transpose(1, 2))


def test_end_to_end_forms_are_bitwise_one(e2e):
    res, model, args = e2e['res'], e2e['model'], e2e['args']
    phon = model.phonons(*args, supercell=er.E2E_S)
    given = model.elastic_constants(*args, supercell=er.E2E_S, phonons=phon)
    for name in ('born', 'relaxation', 'C', 'asymmetry', 'internal_strain', 'status', 'n_zero', 'n_negative'):
        assert torch.equal(getattr(given, name), getattr(res, name)), name
    clamped = model.elastic_constants(*args, supercell=er.E2E_S, relaxed=False)
    assert torch.equal(clamped.C, res.born) and torch.equal(clamped.born, res.born)
    assert torch.count_nonzero(clamped.relaxation) == 0 and torch.count_nonzero(clamped.status) == 0
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    calc = MLAseCalculator(util.load_state('rand', torch.float32), properties=['energy', 'forces'], device='cuda')
    frames = [FakeAtoms(er.E2E_Z[lo:hi], er.E2E_POS[lo:hi], cell=er.E2E_CELLS[b], pbc=(True, True, True))
              for b, (lo, hi) in enumerate(er.E2E_RANGES)]
    both = calc.elastic_constants(frames, er.E2E_S)
    direct = calc.model.elastic_constants(*calc.format_data(frames), er.E2E_S)
    assert torch.equal(both.C, direct.C) and torch.equal(both.born, direct.born) and torch.equal(both.relaxation, direct.relaxation)
    assert torch.equal(both.C, res.C)
    one = calc.elastic_constants(frames[0], er.E2E_S, relaxed=False)
    assert one.C.shape == (1, 6, 6) and one.counts == [2]
    # four atoms over the limit of the relaxed term
    n = el.max_dim() // 3 + 4
    rng = np.random.default_rng(0)
    big = cuda(torch.ones(n, dtype=torch.long), torch.tensor(rng.uniform(0.0, 12.0, (n, 3)), dtype=torch.float32),
               12.0 * torch.eye(3)[None], torch.zeros(n, dtype=torch.long))
    with pytest.raises(NotImplementedError, match=r'elastic\.max_dim\(\)'):
        model.elastic_constants(*big, supercell=(1, 1, 1))
