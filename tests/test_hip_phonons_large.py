"""Phonons above the one-workgroup bound on the device (csrc/phonon_large.hip, solver='auto' / 'blocked' of newtonnet_amd/phonons.py)
against the fp64 yardstick of tests/phonon_ref.py: the smallest size above the old bound, every padding and pairing class, the bound
itself, the two forms against each other, routing and independence, status and refusals, the chain from the model, and the relaxed
elastic term above the old bound.

Bounds (those of tests/test_hip_phonons.py).  Assembly, per element: (n_terms + 8) eps32 sum |terms| (phonon_ref.dynamical_matrix).
Eigenvalues and residuals of a d x d problem: vib_ref.solver_bound(2 d, ||D||_2) -- a complex rotation is the real one of the 2 d
embedding -- plus the Frobenius norm of the assembly bound (Weyl).  ||V V^H - I||_max <= 2 d eps32 x 8.  The measured constant c
(error in units of 2 d eps32 ||D||_2) is printed per size; nothing here is tuned to it."""
import ctypes

import numpy as np
import pytest
import torch

from newtonnet_amd import elastic as el
from newtonnet_amd import hip
from newtonnet_amd import phonons as ph
from tests import elastic_ref as er
from tests import phonon_large_ref as plr
from tests import phonon_ref as pr
from tests import util
from tests import vib_ref as vr

pytestmark = pytest.mark.gpu

EPS32 = vr.EPS32
Q3 = np.array([[0.0, 0.0, 0.0], [0.31, -0.17, 0.44], [-0.5, 0.25, 0.125]])
STATUS_SIZE, STATUS_MASS = hip.abi.CONSTANTS['NNHIP_EIG_STATUS_SIZE'], hip.abi.CONSTANTS['NNHIP_EIG_STATUS_MASS']


def make(cases, **kw):
    """one Phonons over the cases (fc, pos, cell, S, masses), one crystal each"""
    cases = [cases] if isinstance(cases, tuple) else list(cases)
    counts = [len(c[1]) for c in cases]
    return ph.Phonons.from_force_constants([c[0] for c in cases], np.ones(sum(counts), dtype=np.int64), np.concatenate([c[1] for c in cases]),
                                           np.stack([c[2] for c in cases]), np.array([c[3] for c in cases]),
                                           masses=np.concatenate([c[4] for c in cases]), batch=np.repeat(np.arange(len(cases)), counts),
                                           device='cuda', **kw)


def reference(case, q):
    """[(D fp64, assembly bound)] per q, from the force constants and masses as the device holds them (fp32)"""
    fc, pos, cell, S, m = case
    table = pr.image_table_fast(pos, cell, S)
    return [pr.dynamical_matrix(fc.astype(np.float64), pos, cell, S, m.astype(np.float64), x, table, with_bound=True) for x in q]


def eig_bound(D, B):
    return vr.solver_bound(2 * D.shape[0], np.linalg.norm(D, 2)) + np.linalg.norm(B)


def check_spectrum(D, B, ev, modes=None, what=''):
    """device eigenvalues (and modes, rows) of one problem against the fp64 D they belong to; returns the measured constants"""
    d = D.shape[0]
    bound = eig_bound(D, B)
    unit = 2 * d * EPS32 * np.linalg.norm(D, 2)
    err = np.abs(np.asarray(ev, dtype=np.float64) - np.linalg.eigvalsh(D)).max()
    out = dict(c_eig=err / unit, bound=bound)
    assert np.all(np.diff(ev) >= 0), f'{what}: eigenvalues not ascending'
    if modes is not None:
        V = np.asarray(modes, dtype=np.complex128)
        res = np.linalg.norm(D @ V.T - V.T * np.asarray(ev, dtype=np.float64)[None, :], axis=0).max()
        orth = np.abs(V @ V.conj().T - np.eye(d)).max()
        out.update(c_res=res / unit, c_orth=orth / (2 * d * EPS32))
    print(f'{what}: ' + ', '.join(f'{k} = {v:.3g}' for k, v in out.items()))
    assert err <= bound, f'{what}: eigenvalue error {err:.3e} above the bound {bound:.3e}'
    if modes is not None:
        assert res <= bound, f'{what}: residual {res:.3e} above the bound {bound:.3e}'
        assert orth <= 2 * d * EPS32 * 8, f'{what}: ||V V^H - I||_max = {orth:.3e} above {2 * d * EPS32 * 8:.3e}'
        for row in V:   # the largest component is real and positive (the device ranks |v|^2 in fp32: any of the near-largest may be it)
            top = row[np.abs(row) >= np.abs(row).max() * (1.0 - 1e-5)]
            assert np.any((top.real > 0) & (np.abs(top.imag) <= 4 * EPS32)), f'{what}: phase convention'
    return out


def bits(x):
    """the bit patterns of a real or complex fp32 tensor"""
    x = torch.view_as_real(x) if x.is_complex() else x
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---- 1. the smallest size above the old bound -------------------------------------------------------------------------------------

@pytest.mark.parametrize('copies', [8, 9])
def test_smallest_size_above_the_old_bound(copies):
    """d = 99 pads to 128: two block pairs.  9 copies cross the 8-copy phase chunk of the one-workgroup form (and the chunk of 4 here)"""
    case = pr.stage_case(99, copies)
    with pytest.raises(NotImplementedError, match=r'phonons\.max_dim\(\)'):
        make(case)
    p = make(case, solver='auto')
    bands = p.frequencies(pr.STAGE_Q, modes=True, dynamical_matrix=True)
    assert int(bands.status.abs().max()) == 0 and int(bands.sweeps.min()) >= 1
    ev, _, modes = (x.cpu().numpy() for x in bands.crystal(0))
    Dd = bands.dynamical(0).cpu().numpy()
    worst = 0.0
    for k, (D, B) in enumerate(reference(case, pr.STAGE_Q)):
        diff = np.abs(Dd[k].astype(np.complex128) - D)
        assert np.all(diff <= B), f'q {k}: |dD| exceeds the assembly bound by {np.max(diff - B):.3e}'
        assert np.array_equal(Dd[k], Dd[k].conj().T), 'D(q) on the device is not exactly Hermitian'
        worst = max(worst, float(np.max(diff / np.where(B > 0, B, 1.0))))
        check_spectrum(D, B, ev[k], modes[k], f'd = 99, {copies} copies, q {k}')
    print(f'{copies} copies: max |dD| / bound = {worst:.3f}, sweeps {bands.sweeps.cpu().tolist()}')


# ---- 2. every padding and pairing class ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('d', [3, 33, 96, 129, 192, 252])
def test_every_padding_and_pairing_class(d):
    """d = 3: one pair, no tile update at all; 33, 96: one and two pairs with padding; 129: three pairs; 192: no padding; 252: the
    aspirin cell"""
    case = plr.planted_case(d // 3, 100 + d)
    bands = make(case, solver='blocked').frequencies(Q3, modes=True)
    assert int(bands.status.abs().max()) == 0 and int(bands.sweeps.min()) >= 1
    ev, _, modes = (x.cpu().numpy() for x in bands.crystal(0))
    for k, (D, B) in enumerate(reference(case, Q3)):
        check_spectrum(D, B, ev[k], modes[k], f'd = {d} q {k}')
    print(f'd = {d}: sweeps {bands.sweeps.cpu().tolist()}')


# ---- 3. at the bound ------------------------------------------------------------------------------------------------------------------

def test_at_the_bound():
    d = ph.max_dim_large()
    assert d == 768
    case = plr.planted_case(d // 3, 100 + d)
    q = Q3[1:2]
    bands = make(case, solver='auto').frequencies(q, modes=True)
    assert int(bands.status.abs().max()) == 0
    ev, _, modes = (x.cpu().numpy() for x in bands.crystal(0))
    (D, B), = reference(case, q)
    check_spectrum(D, B, ev[0], modes[0], f'd = {d}')
    print(f'd = {d}: sweeps {bands.sweeps.cpu().tolist()}')


# ---- 4. the two forms against each other ----------------------------------------------------------------------------------------------

def test_forms_against_each_other():
    cases = [plr.planted_case(3, 11), pr.stage_case(24, 9), pr.stage_case(72, 8), plr.planted_case(32, 12)]
    p = make(cases)
    lds = p.frequencies(pr.STAGE_Q, dynamical_matrix=True)
    blk = p.frequencies(pr.STAGE_Q, dynamical_matrix=True, solver='blocked')
    assert int(lds.status.abs().max()) == 0 and int(blk.status.abs().max()) == 0
    assert same_bits(lds.dynamical_matrix, blk.dynamical_matrix), 'D(q) of the two forms differs in some bit'
    for b, case in enumerate(cases):
        e0, e1 = (x.crystal(b)[0].cpu().numpy().astype(np.float64) for x in (lds, blk))
        for k, (D, B) in enumerate(reference(case, pr.STAGE_Q)):
            bound = eig_bound(D, B)
            assert np.abs(e0[k] - e1[k]).max() <= 2 * bound, (b, k, np.abs(e0[k] - e1[k]).max(), bound)


# ---- 5. routing and independence ---------------------------------------------------------------------------------------------------

def test_routing_and_independence():
    cases = [pr.stage_case(24, 9), pr.stage_case(99, 8), plr.planted_case(3, 13), plr.planted_case(43, 14)]
    q = pr.STAGE_Q[1:4]
    p = make(cases, solver='auto')
    both = p.frequencies(q, modes=True, dynamical_matrix=True)
    assert int(both.status.abs().max()) == 0
    for b, case in enumerate(cases):
        alone = make(case, solver='lds' if b in (0, 2) else 'blocked').frequencies(q, modes=True, dynamical_matrix=True)
        assert same_bits(alone.crystal(0)[0], both.crystal(b)[0]), f'crystal {b}: eigenvalues'
        assert same_bits(alone.crystal(0)[2], both.crystal(b)[2]), f'crystal {b}: modes'
        assert same_bits(alone.dynamical(0), both.dynamical(b)), f'crystal {b}: D(q)'
        assert torch.equal(alone.sweeps[0], both.sweeps[b])
    one = p.frequencies(q[1:2], modes=True)                                    # a q alone
    for b in range(4):
        assert same_bits(one.crystal(b)[0][0], both.crystal(b)[0][1]) and same_bits(one.crystal(b)[2][0], both.crystal(b)[2][1])
    plain = p.frequencies(q)                                                   # without modes
    assert plain.modes is None and same_bits(plain.eigenvalues, both.eigenvalues) and torch.equal(plain.sweeps, both.sweeps)
    again = p.frequencies(q, modes=True, dynamical_matrix=True)                # two calls
    assert same_bits(again.eigenvalues, both.eigenvalues) and same_bits(again.modes, both.modes)
    assert same_bits(again.dynamical_matrix, both.dynamical_matrix)
    chunked = p.frequencies(q, modes=True, dynamical_matrix=True, workspace_bytes=1)   # one q per chunk
    assert same_bits(chunked.eigenvalues, both.eigenvalues) and same_bits(chunked.modes, both.modes)
    assert same_bits(chunked.dynamical_matrix, both.dynamical_matrix)
    assert torch.equal(chunked.sweeps, both.sweeps) and torch.equal(chunked.status, both.status)


# ---- 6. status and refusals -----------------------------------------------------------------------------------------------------------

def raw_call(p, q, cry_dev=None, cry_host=None, ws_bytes=None, ws_shift=0, n_cry=None):
    """nnhip_phonon_bands_large on the tables of p with outputs pre-filled with sentinels: (rc, evals, modes, sweeps, status)"""
    L, dev = hip.lib(), p.fc.device
    B, Q = len(p.counts) if n_cry is None else n_cry, len(q)
    n_val, n_sq = 3 * sum(p.counts), sum(9 * n * n for n in p.counts)
    evals = torch.full((Q * n_val,), -7.0, dtype=torch.float32, device=dev)
    modes = torch.full((Q * n_sq, 2), -7.0, dtype=torch.float32, device=dev)
    sweeps, status = (torch.full((B, Q), -7, dtype=torch.int32, device=dev) for _ in range(2))
    q_dev = torch.tensor(np.asarray(q), dtype=torch.float64, device=dev)
    cry_host = p._cry_host if cry_host is None else cry_host
    need = int(L.nnhip_phonon_large_ws_bytes(p._cry_host.data_ptr(), len(p.counts), Q, 1, None))
    ws = torch.zeros(need + 512, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    rc = L.nnhip_phonon_bands_large(hip._ptr(p.fc), hip._ptr(p.fc_ptr), hip._ptr(p.cry_ptr if cry_dev is None else cry_dev),
                                    cry_host.data_ptr(), hip._ptr(p.sc_atoms), hip._ptr(p.img_ptr), hip._ptr(p.img_start),
                                    hip._ptr(p.img_off), hip._ptr(p.masses), hip._ptr(p.out_ptr), B, hip._ptr(q_dev), Q, hip._ptr(evals),
                                    hip._ptr(modes), None, hip._ptr(sweeps), hip._ptr(status), None, ws.data_ptr() + ws_shift,
                                    need if ws_bytes is None else ws_bytes, hip._stream(dev))
    torch.cuda.synchronize()
    return rc, evals, modes, sweeps, status


def test_status_bits():
    cases = [plr.planted_case(33, 21), plr.planted_case(3, 22)]
    bad = (cases[0][0], cases[0][1], cases[0][2], cases[0][3], cases[0][4].copy())
    bad[4][5] = 0.0                                                       # a mass that is not positive
    p = make([bad, cases[1]], solver='blocked')
    bands = p.frequencies(Q3, modes=True)
    assert bands.status[0].tolist() == [STATUS_MASS] * 3 and bands.status[1].tolist() == [0] * 3
    assert int(bands.crystal(0)[0].abs().max()) == 0 and int(bands.sweeps[0].abs().max()) == 0     # nothing of it is computed
    alone = make(cases[1], solver='blocked').frequencies(Q3, modes=True)
    assert same_bits(alone.crystal(0)[0], bands.crystal(1)[0]) and same_bits(alone.crystal(0)[2], bands.crystal(1)[2])
    # the device's cry_ptr gives the crystal one atom more than the host copy the regions were sized from
    good = make(cases[0], solver='blocked')
    rc, evals, modes, sweeps, status = raw_call(good, Q3, cry_dev=torch.tensor([0, 34], dtype=torch.int32, device='cuda'))
    assert rc == 0
    assert status.tolist() == [[STATUS_SIZE] * 3] and sweeps.tolist() == [[0] * 3]
    assert bool((evals == -7.0).all()) and bool((modes == -7.0).all())     # nothing else is written
    rc, evals, _, _, status = raw_call(good, Q3)                           # (the helper's call is a good one otherwise)
    assert rc == 0 and status.tolist() == [[0] * 3] and same_bits(evals, good.frequencies(Q3).eigenvalues)


def test_refusals():
    L = hip.lib()
    p = make(plr.planted_case(33, 21), solver='blocked')
    need = int(L.nnhip_phonon_large_ws_bytes(p._cry_host.data_ptr(), 1, 3, 1, None))
    for kw in (dict(ws_bytes=need - 1), dict(ws_shift=128)):
        rc, evals, modes, sweeps, status = raw_call(p, Q3, **kw)
        assert rc == hip.abi.CONSTANTS['NNHIP_E_WORKSPACE'], kw
        assert bool((evals == -7.0).all()) and bool((status == -7).all())
    # one atom above the bound: refused before any kernel, from Python and from the ABI
    n = ph.max_dim_large() // 3 + 1
    big = (np.zeros((n, 3, n, 3), dtype=np.float32), np.random.default_rng(5).uniform(0.0, 9.0, (n, 3)), 9.0 * np.eye(3), (1, 1, 1),
           np.ones(n, dtype=np.float32))
    for solver in ('auto', 'blocked'):
        with pytest.raises(NotImplementedError, match=r'768 of phonons\.max_dim_large\(\)'):
            make(big, solver=solver)
    rc, evals, modes, sweeps, status = raw_call(p, Q3, cry_host=torch.tensor([0, n], dtype=torch.int32))
    assert rc == hip.abi.CONSTANTS['NNHIP_E_UNSUPPORTED']
    msg = L.nnhip_last_error().decode()
    assert 'crystal 0' in msg and '768' in msg and str(3 * n) in msg, msg
    assert bool((evals == -7.0).all()) and bool((status == -7).all()) and bool((sweeps == -7).all())


# ---- 7. end to end with the model -----------------------------------------------------------------------------------------------------

E2E_CELL = np.array([[8.5, 0.3, -0.2], [0.3, 8.4, 0.25], [-0.2, 0.25, 8.6]])      # symmetric, mildly triclinic
E2E_S = (2, 2, 2)


def e2e_atoms():
    """33 atoms of H / C / O in E2E_CELL, every pair (periodic images included) at least 0.9 A apart"""
    rng = np.random.default_rng(33)
    shifts = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64) @ E2E_CELL
    pos = []
    for _ in range(100000):
        x = rng.uniform(0.0, 1.0, 3) @ E2E_CELL
        if all(np.linalg.norm(x - y[None, :] + shifts, axis=1).min() >= 0.9 for y in pos) and \
                np.linalg.norm(shifts[np.abs(shifts).sum(axis=1) > 0], axis=1).min() >= 0.9:
            pos.append(x)
        if len(pos) == 33:
            break
    assert len(pos) == 33
    return rng.choice([1, 6, 8], 33), np.array(pos)


@pytest.fixture(scope='module')
def e2e():
    from tests.test_hip_hessian import make_model
    model = make_model(util.load_state('rand'))
    z, pos = e2e_atoms()
    args = [torch.tensor(z).cuda(), torch.tensor(pos, dtype=torch.float32).cuda(), torch.tensor(E2E_CELL, dtype=torch.float32)[None].cuda(),
            torch.zeros(33, dtype=torch.long).cuda()]
    return dict(model=model, args=args, z=z, phon=model.phonons(*args, supercell=E2E_S, solver='auto'))


def test_end_to_end_with_the_model(e2e):
    model, args, p = e2e['model'], e2e['args'], e2e['phon']
    with pytest.raises(NotImplementedError, match=r'phonons\.max_dim\(\)'):
        model.phonons(*args, supercell=E2E_S)
    assert p.counts == [33] and p.sc_counts == [264] and p.solver == 'auto'
    q = np.concatenate([[[0.0, 0.0, 0.0]], np.random.default_rng(23).uniform(-0.5, 0.5, (3, 3))])
    bands = p.frequencies(q)
    assert int(bands.status.abs().max()) == 0
    ev = bands.crystal(0)[0].cpu().numpy().astype(np.float64)
    m = np.array([vr.MASSES[int(x)] for x in e2e['z']], dtype=np.float32)
    case = (p.force_constants(0).cpu().numpy(), args[1].double().cpu().numpy(), args[2][0].double().cpu().numpy(), E2E_S, m)
    ref = reference(case, q)
    for k, (D, B) in enumerate(ref):
        check_spectrum(D, B, ev[k], None, f'model, q {k}')
    assert np.sum(np.abs(ev[0]) <= eig_bound(*ref[0])) >= 3, ev[0][:8]      # the sum rule: three acoustic modes at Gamma
    mesh = p.mesh(2, 2, 2)
    t = mesh.thermochemistry(300.0)
    for key in ('ZPE', 'U', 'S', 'F', 'Cv'):
        assert bool(torch.isfinite(getattr(t, key)).all()), key
    want = pr.thermochemistry(mesh.bands.crystal(0)[0].cpu().numpy(), 300.0, float(mesh.threshold()[0]))
    assert int(t.n_skipped_zero[0]) == want['n_zero'] >= 3                  # the acoustic modes at Gamma
    np.testing.assert_allclose(float(t.F[0]), want['F'], rtol=1e-5)


def test_calculator_phonons_agree_with_the_model(e2e):
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    calc = MLAseCalculator(util.load_state('rand', torch.float32), properties=['energy', 'forces'], device='cuda')
    frame = FakeAtoms(e2e['z'], e2e['args'][1].double().cpu().numpy(), cell=E2E_CELL, pbc=(True, True, True))
    with pytest.raises(NotImplementedError, match=r'phonons\.max_dim\(\)'):
        calc.phonons([frame], E2E_S)
    both = calc.phonons([frame], E2E_S, solver='auto')
    z, pos, cell, batch = calc.format_data([frame])
    direct = calc.model.phonons(z, pos, cell, batch, E2E_S, solver='auto')
    q = np.array([[0.0, 0.0, 0.0], [0.2, 0.1, -0.4]])
    assert torch.equal(both.fc, direct.fc) and same_bits(both.frequencies(q).eigenvalues, direct.frequencies(q).eigenvalues)


# ---- 8. the relaxed elastic term above the old bound ----------------------------------------------------------------------------------

STAGE_C, KAPPA = 0.4, 100.0        # the tolerance of test_stage_fold_and_relaxation (tests/test_hip_elastic.py) for this comparison


@pytest.mark.parametrize('n', [33, 43])
def test_elastic_relaxed_term_above_the_old_bound(n):
    """n = 33: above elastic.max_dim() = 96, still on the one-workgroup real solver (99 <= 126); n = 43: the blocked real solver"""
    phi0, lam = er.planted_phi0(n, 60 + n, kappa=KAPPA)
    d = 3 * n
    phi_dev = torch.tensor(phi0.astype(np.float32).reshape(-1), device='cuda')
    lam_dev = torch.tensor(lam.astype(np.float32), device='cuda')
    ptr = torch.zeros(1, dtype=torch.int64, device='cuda')
    with pytest.raises(NotImplementedError, match=rf'crystal 0 has 3 x {n} = {d} coordinates, above the 96 of elastic\.max_dim\(\)'):
        el.relaxation_term(phi_dev, ptr, [n], lam_dev)
    R, n_zero, n_neg, status = el.relaxation_term(phi_dev, ptr, [n], lam_dev, solver='auto')
    assert n_zero.tolist() == [3] and n_neg.tolist() == [0] and status.tolist() == [0]
    phi64 = phi_dev.cpu().numpy().astype(np.float64).reshape(d, d)
    phi64 = 0.5 * (phi64 + phi64.T)
    w = np.linalg.eigvalsh(phi64)
    thr = 8.0 * EPS32 * d * np.abs(w).max()
    R_ref, nz, nn = er.relaxation_reference(phi64, lam_dev.cpu().numpy(), thr)
    assert (nz, nn) == (3, 0)
    R = R[0].cpu().numpy()
    scale = np.abs(R_ref).max()
    err = np.abs(R.astype(np.float64) - R_ref).max()
    bound = STAGE_C * KAPPA * d * EPS32 * scale
    print(f'n = {n}: |dR| {err:.3e} of {scale:.3e}, ratio to kappa d eps32 max|R| = {err / (KAPPA * d * EPS32 * scale):.4f} (allowed {STAGE_C})')
    assert np.array_equal(R, R.T) and err <= bound, f'n = {n}: |dR| {err:.3e} above {bound:.3e}'
