"""CPU-side checks of variable-cell relaxation (newtonnet_amd/cellrelax.py, csrc/cellrelax.hip): the C ABI exports the kernel and
the header's constants are the Python ones, arguments are refused before any device work, the generalised forces are minus the
gradient of the enthalpy (torch float64 autograd), the fp64 reference driver (tests/cellrelax_ref.py) takes the analytic crystal to
its known minimum, a numpy-float32 emulation of the launch stays inside the reference's bound, and the synthetic batch of the GPU
test reaches every branch with no ambiguous decision."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import cellrelax_ref as cr
from tests import relax_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_symbol_is_declared_listed_and_exported():
    from newtonnet_amd import abi, hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    name = 'nnhip_cell_lbfgs_step'
    assert name in declared and name in abi.FUNCTIONS and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bcellrelax\b.*\)', f.read(), re.M)
    assert callable(hip.cell_lbfgs_step)
    for py, c_name, ref in ((hip.CELL_LBFGS_CHECK_ONLY, 'NNHIP_CELL_LBFGS_CHECK_ONLY', cr.CHECK_ONLY),
                            (hip.CELL_LBFGS_HYDROSTATIC, 'NNHIP_CELL_LBFGS_HYDROSTATIC', cr.HYDROSTATIC),
                            (hip.CELL_LBFGS_CONSTANT_VOLUME, 'NNHIP_CELL_LBFGS_CONSTANT_VOLUME', cr.CONSTANT_VOLUME)):
        in_header = int(re.search(r'^#define\s+' + c_name + r'\s+(\d+)\s*$', header, re.M).group(1))
        assert py == in_header == ref == abi.CONSTANTS[c_name]
    assert hip.CELL_LBFGS_MASK_ALL == cr.MASK_ALL == 63 and hip.CELL_LBFGS_CHECK_ONLY == hip.LBFGS_CHECK_ONLY
    from newtonnet_amd import npt
    assert cr.BAR == npt.BAR


class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force', 'virial']


def _inputs(n=3, b=1):
    return (torch.ones(n, dtype=torch.long), torch.zeros(n, 3), 10.0 * torch.eye(3).repeat(b, 1, 1), torch.zeros(n, dtype=torch.long))


def test_cell_relaxation_validates_before_any_device_work():
    from newtonnet_amd.cellrelax import CellRelaxation
    from newtonnet_amd.models.newtonnet import NewtonNet
    assert callable(NewtonNet.cell_relaxation)
    z, pos, cell, batch = _inputs()
    ok = _FakeModel()
    no_virial = _FakeModel()
    no_virial.output_properties = ['energy', 'gradient_force']
    with pytest.raises(ValueError, match='virial'):
        CellRelaxation(no_virial, z, pos, cell, batch)
    no_force = _FakeModel()
    no_force.output_properties = ['energy', 'virial']
    with pytest.raises(ValueError, match='gradient_force'):
        CellRelaxation(no_force, z, pos, cell, batch)
    train = _FakeModel()
    train.training = True
    with pytest.raises(ValueError, match='eval'):
        CellRelaxation(train, z, pos, cell, batch)
    for kw, match in ((dict(fmax=0.0), 'fmax'), (dict(fmax=float('nan')), 'fmax'), (dict(memory=0), 'memory'),
                      (dict(memory=65), 'memory'), (dict(memory=2.5), 'memory'), (dict(maxstep=-0.1), 'maxstep'),
                      (dict(alpha=0.0), 'alpha'), (dict(alpha=float('inf')), 'alpha'),
                      (dict(mask=[1, 1, 1]), 'mask'), (dict(mask=np.ones((3, 3))), 'mask'), (dict(mask=[1, 1, 1, 0, 0, 2]), 'mask'),
                      (dict(pressure=float('nan')), 'pressure'), (dict(pressure=float('inf')), 'pressure'),
                      (dict(pressure=torch.tensor([float('nan')])), 'pressure'), (dict(pressure=torch.ones(2)), 'pressure'),
                      (dict(hydrostatic=1), 'hydrostatic'), (dict(constant_volume='yes'), 'constant_volume'),
                      (dict(cell_factor=0.0), 'cell_factor'), (dict(cell_factor=float('nan')), 'cell_factor'),
                      (dict(fixed=torch.zeros(2, dtype=torch.bool)), 'fixed')):
        with pytest.raises(ValueError, match=match):
            CellRelaxation(ok, z, pos, cell, batch, **kw)
    with pytest.raises(ValueError, match='pos'):
        CellRelaxation(ok, z, torch.zeros(3, 2), cell, batch)
    with pytest.raises(ValueError, match='cell'):
        CellRelaxation(ok, z, pos, cell[0], batch)
    # a stress head serves as well; with sound arguments the first thing missing is the device
    stress = _FakeModel()
    stress.output_properties = ['energy', 'gradient_force', 'stress']
    for model in (ok, stress):
        with pytest.raises(RuntimeError, match='MI355X'):
            CellRelaxation(model, z, pos, cell, batch, pressure=1000.0, mask=[1, 1, 1, 0, 0, 0], hydrostatic=False,
                           fixed=torch.zeros(3, dtype=torch.bool))


def test_calculator_relax_cell_validates_before_any_device_work():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype = torch.device('cpu'), torch.float32
    calc.model = _FakeModel()
    box = dict(cell=8.0 * np.eye(3), pbc=(True, True, True))
    a, b = FakeAtoms([8, 1, 1], np.zeros((3, 3)), **box), FakeAtoms([6, 1], np.zeros((2, 3)), **box)
    with pytest.raises(ValueError, match='at least one'):
        calc.relax_cell([])
    with pytest.raises(ValueError, match='sizes'):
        calc.relax_cell([a, b])
    for kw, match in ((dict(fmax=-0.01), 'fmax'), (dict(max_steps=-1), 'max_steps'), (dict(max_steps=2.5), 'max_steps'),
                      (dict(memory=0), 'memory'), (dict(maxstep=0.0), 'maxstep'), (dict(alpha=-70.0), 'alpha'),
                      (dict(check_every=-1), 'check_every'), (dict(fixed=[True, False]), 'fixed'), (dict(mask=[1, 0]), 'mask'),
                      (dict(pressure=float('nan')), 'pressure'), (dict(pressure=[1.0, 2.0]), 'pressure'),
                      (dict(pressure=[float('inf')]), 'pressure'), (dict(cell_factor=-1.0), 'cell_factor'),
                      (dict(hydrostatic=None), 'hydrostatic')):
        with pytest.raises(ValueError, match=match):
            calc.relax_cell(a, **kw)
    calc.model = _FakeModel()
    calc.model.output_properties = ['energy', 'gradient_force']
    with pytest.raises(ValueError, match='virial'):
        calc.relax_cell(a)
    calc.model = _FakeModel()
    calc.model.training = True
    with pytest.raises(ValueError, match='eval'):
        calc.relax_cell(a)
    calc.model = _FakeModel()
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.relax_cell(a, pressure=[100.0], mask=[1, 1, 1, 0, 0, 0])


# ---- the generalised forces are minus the gradient of the enthalpy -------------------------------------------------------------------

def _energy(x, h):
    """an analytic energy of Cartesian positions x [n,3] and the cell h [3,3] (rows are lattice vectors), invariant under nothing in
    particular: pair terms on minimum-image-free distances, a term in the fractional coordinates and a term in the metric"""
    d = x[:, None, :] - x[None, :, :]
    r2 = (d * d).sum(-1) + torch.eye(x.shape[0], dtype=x.dtype)
    pair = (torch.exp(-0.3 * r2) * (1.0 - torch.eye(x.shape[0], dtype=x.dtype))).sum()
    frac = x @ torch.linalg.inv(h)
    metric = h @ h.T
    return pair + 0.2 * torch.sin(2.0 * frac).sum() + 0.01 * (metric * metric).sum() - 0.3 * torch.logdet(h) + 0.05 * (x @ h[0]).sum()


def _autograd_problem(seed=5, n=7):
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    h0 = torch.diag(torch.tensor([6.0, 7.0, 8.0], dtype=f64)) + 0.7 * torch.tril(torch.randn(3, 3, generator=g, dtype=f64), -1)
    F = torch.eye(3, dtype=f64) + 0.08 * torch.randn(3, 3, generator=g, dtype=f64)          # triclinic, F != I, not symmetric
    q = 6.0 * torch.rand(n, 3, generator=g, dtype=f64)
    return h0, F, q


def _mask_independent(flags6):
    xx, yy, zz, yz, xz, xy = flags6
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=np.float64)


@pytest.mark.parametrize('option', ['none', 'mask', 'hydrostatic', 'constant_volume', 'mask_constant_volume', 'fixed'])
def test_generalised_forces_are_minus_the_enthalpy_gradient(option):
    h0, F, q = _autograd_problem()
    n, c, p = q.shape[0], 7.0, 0.013
    # H(X) = E(x(X), h(X)) + p det h(X):  x = q F^T, h = h0 F^T, F = X[n:] / c
    X = torch.cat([q, c * F]).requires_grad_(True)
    Fx = X[n:] / c
    H = _energy(X[:n] @ Fx.T, h0 @ Fx.T) + p * torch.linalg.det(h0 @ Fx.T)
    grad = -torch.autograd.grad(H, X)[0].numpy()
    # the model's view: forces at fixed cell, the virial as minus the strain derivative at eps = 0
    x, h = (q @ F.T).detach().requires_grad_(True), (h0 @ F.T).detach()
    eps = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
    one = torch.eye(3, dtype=torch.float64) + eps
    E = _energy(x @ one.T, h @ one.T)
    gx, ge = torch.autograd.grad(E, (x, eps))
    f, W = -gx.numpy(), -ge.numpy()
    flags6 = (1, 0, 1, 0, 1, 1)
    bits = sum(1 << k for k in range(6) if flags6[k])
    want = grad.copy()
    Wc = want[n:] * c
    free, kw = None, {}
    if option in ('mask', 'mask_constant_volume'):
        Wc = Wc * _mask_independent(flags6)
        kw['bits'] = bits
    if option == 'hydrostatic':
        Wc = np.eye(3) * np.trace(Wc) / 3.0
        kw['flags'] = cr.HYDROSTATIC
    if option in ('constant_volume', 'mask_constant_volume'):
        Wc = Wc - np.eye(3) * np.trace(Wc) / 3.0
        kw['flags'] = cr.CONSTANT_VOLUME
    if option == 'fixed':
        free = np.array([True, False, True, True, False, True, True])
        want[:n][~free] = 0.0
    want[n:] = Wc / c
    G = cr.generalised_forces(f, W, F.numpy(), h.numpy(), p, c, free, **kw)
    scale = np.abs(grad).max()
    print(f'{option}: max |G + dH/dX| / max |dH/dX| = {np.abs(G - want).max() / scale:.2e}')
    assert np.abs(G - want).max() <= 1e-10 * scale
    assert np.abs(grad[n:]).min() > 1e-3 * scale                 # every cell component carries weight: the check is not vacuous
    # and the Val prologue of the reference (the fp64 values of its chain, eps = 0) is the same G
    pro = cr.prologue((c * F).numpy(), f, W, h.numpy(), free, p, c, kw.get('bits', cr.MASK_ALL), kw.get('flags', 0), eps=0.0)
    assert not pro['skip'] and np.abs(pro['G'].v - want).max() <= 1e-10 * scale and not pro['G'].b.any()


# ---- the reference driver and the analytic crystal ------------------------------------------------------------------------------------

_crystal = {}


def host_crystal(fmax=1e-3):
    """the fp64 driver's minimum of the analytic crystal, computed once per process (shared with tests/test_hip_cellrelax.py)"""
    if fmax not in _crystal:
        c = cr.crystal()
        _crystal[fmax] = (c, cr.minimise(lambda x, h: cr.crystal_efv(c, x, h), c['x0'], c['h0'], c['ptr'], fmax=fmax, max_steps=400,
                                         pressure=c['p']))
    return _crystal[fmax]


def metric_bound(c, b, fmax, F):
    """|F^T F - (I + 2 eps0)|_max at a point whose three generalised cell rows are below fmax, at zero pressure:  G_cell = -F A / n
    with A = K V0 (eps_G - eps0) and cell_factor = n, so |F A|_F <= n sqrt(3) fmax, |A|_F <= |F^-1|_2 n sqrt(3) fmax, and
    F^T F - I - 2 eps0 = 2 A / (K V0)"""
    n = int(c['ptr'][b + 1] - c['ptr'][b])
    return 2.0 * n * np.sqrt(3.0) * fmax * np.linalg.norm(np.linalg.inv(F), 2) / (c['K'] * c['V0'][b])


def test_crystal_closed_form_is_its_own_gradient():
    c = cr.crystal()
    t = cr.crystal_tensors(c, 'cpu', torch.float64)
    rng = np.random.default_rng(2)
    B = len(c['ptr']) - 1
    F = np.eye(3) + rng.normal(0, 0.03, (B, 3, 3))
    h = np.stack([c['h0'][b].astype(np.float64) @ F[b].T for b in range(B)])
    bt = t['batch'].numpy()
    x = np.einsum('ni,nji->nj', c['x0'].astype(np.float64), F[bt])
    E, f, W = cr.crystal_efv(c, x, h)
    xt, eps = torch.tensor(x, requires_grad=True), torch.zeros(B, 3, 3, dtype=torch.float64, requires_grad=True)
    one = torch.eye(3, dtype=torch.float64) + eps
    Et, _, _ = cr.crystal_efv_torch(t, (xt[:, None, :] @ one[t['batch']].transpose(1, 2))[:, 0, :], torch.tensor(h) @ one.transpose(1, 2))
    gx, ge = torch.autograd.grad(Et.sum(), (xt, eps))
    Et2, ft, Wt = cr.crystal_efv_torch(t, torch.tensor(x), torch.tensor(h))
    np.testing.assert_allclose(Et2.numpy(), E, rtol=1e-12)
    np.testing.assert_allclose(ft.numpy(), f, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(Wt.numpy(), W, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(-gx.numpy(), f, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(-ge.numpy(), W, rtol=1e-9, atol=1e-10)


def test_reference_driver_takes_the_crystal_to_its_known_minimum():
    fmax = 1e-3
    c, res = host_crystal(fmax)
    B = len(c['ptr']) - 1
    print('fp64 driver on the crystal: steps', res['n_steps'].tolist(), 'fmax', np.round(res['fmax'], 6).tolist())
    assert res['converged'].all() and (res['fmax'] < fmax).all() and (res['n_steps'] > 3).all()
    assert np.all(res['enthalpy_trace'][-1] < res['enthalpy_trace'][0])
    for b in range(B):
        s = slice(int(c['ptr'][b]), int(c['ptr'][b + 1]))
        F = res['F'][b]
        dev = np.abs(F.T @ F - np.eye(3) - 2.0 * c['eps0'][b]).max()
        if c['p'][b] == 0.0:
            assert dev <= metric_bound(c, b, fmax, F), (b, dev, metric_bound(c, b, fmax, F))
            h0 = c['h0'][b].astype(np.float64)
            np.testing.assert_allclose(res['cell'][b] @ res['cell'][b].T, h0 @ (np.eye(3) + 2 * c['eps0'][b]) @ h0.T,
                                       atol=np.abs(h0).sum(1).max() ** 2 * metric_bound(c, b, fmax, F))
        else:
            assert dev > 10 * metric_bound(c, b, fmax, F)              # the pressure moves the minimum: 0.02 / K of strain
            assert np.linalg.det(F) < np.sqrt(np.linalg.det(np.eye(3) + 2.0 * c['eps0'][b]))          # and compresses it
        q = res['x'][s] @ np.linalg.inv(F).T
        assert np.abs(q - c['q0'][s]).max() <= fmax / c['k'] * 1.0001       # G_atom = -k (q - q0), row norm below fmax


# ---- the emulation inside the bound; the synthetic batch ---------------------------------------------------------------------------

@pytest.fixture(scope='module')
def syn():
    return cr.synthetic_batch()


@pytest.mark.parametrize('bits,flags', list(cr.SYN_OPTIONS) + [(cr.MASK_ALL, cr.CHECK_ONLY)])
def test_float32_emulation_stays_inside_the_bound_and_no_decision_is_ambiguous(syn, bits, flags):
    out = cr.emulate_launch(syn, bits, flags)
    worst, seen, ambiguous = cr.check_launch(syn, out, bits, flags)
    print(f'emulated launch bits = {bits}, flags = {flags}, {len(syn["kinds"])} systems, {syn["X"].shape[0]} rows: worst err / bound '
          + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert not ambiguous, ambiguous
    assert all(v <= 0.75 for v in worst.values())          # a correct fp32 chain sits well inside C_RX = 2 x first order


def test_synthetic_batch_reaches_every_branch(syn):
    d = syn
    sizes = np.diff(d['ptr'])
    assert set(sizes) == set(cr.SYN_SIZES) and 64 in sizes + 3 and 65 in sizes + 3
    _, seen, ambiguous = cr.check_launch(d, cr.emulate_launch(d), cr.MASK_ALL, 0)
    assert not ambiguous
    for want in ([('accept', 'step', True, False, False), ('accept', 'step', True, True, False), ('accept', 'step', True, True, True),
                  ('first', 'step', None, False, False), ('first', 'step', None, True, False), ('first', 'step', None, True, True),
                  ('converged', 'frozen', None, False, False), ('converging', 'frozen', None, False, False),
                  ('det_neg', 'skip', None, False, False)]
                 + [(k, 'step', False, cl, False) for k in ('reject_neg', 'reject_cos') for cl in (False, True)]):
        assert want in seen, (want, sorted(seen, key=str))
    # the inputs vary as the docstring says
    F = np.stack([d['X'][cr.rows_of(d, b)[1]:cr.rows_of(d, b)[2]] / d['c'][b] for b in range(len(sizes))])
    at_identity = np.array([np.array_equal(f, np.eye(3, dtype=np.float32)) for f in F])
    ortho = np.array([np.count_nonzero(h) == 3 for h in d['h0']])
    assert at_identity.any() and (~at_identity).any() and ortho.any() and (~ortho).any()
    assert (d['p'] == 0).any() and (d['p'] > 0).any() and (d['p'] < 0).any() and not d['free'].all()
    assert (np.linalg.det(d['h0'].astype(np.float64)) > 0).all()
    # heads wrap: some system's newest pair sits in a higher slot than its pending one
    assert any(int(d['n_pairs'][b]) >= 2 and int(d['head'][b]) < int(d['n_pairs'][b]) for b in range(len(sizes)))
    # with every strain component masked the cell rows of G are exactly zero and the cell does not move
    out = cr.emulate_launch(d, 0, 0)
    for b, kind in enumerate(d['kinds']):
        _, rc, r1 = cr.rows_of(d, b)
        if kind in ('first',) and sizes[b] > 0:
            assert not out['G'][rc:r1].any() and np.array_equal(out['x_out'][rc:r1], d['X'][rc:r1]), b
