"""CPU-side checks of the phonon module (newtonnet_amd/phonons.py, csrc/phonon.hip): the convention of the dynamical matrix on an
analytic lattice and on the commensurate wave vectors of a random crystal (fp64 yardstick, tests/phonon_ref.py), the product's
host helpers against that yardstick, every argument check before any device work, and the build plumbing."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from newtonnet_amd import phonons as ph
from tests import phonon_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_analytic_cubic_lattice():
    """omega^2_c = (2 K_c / m)(1 - cos 2 pi q_c) at 20 random q; the S = 2 axis goes through the tie multiplicity"""
    fc, pos, cell = pr.cubic_lattice()
    table = pr.image_table(pos, cell, pr.CUBIC_S)
    assert len(table[(0, pr.lattice_offsets(pr.CUBIC_S).index((1, 0, 0)))]) == 2          # both neighbours along x: one atom, two images
    assert len(table[(0, pr.lattice_offsets(pr.CUBIC_S).index((0, 1, 0)))]) == 1
    rng = np.random.default_rng(0)
    worst = 0.0
    for q in rng.uniform(-1.0, 1.0, (20, 3)):
        D = pr.dynamical_matrix(fc, pos, cell, pr.CUBIC_S, [pr.CUBIC_MASS], q, table)
        worst = max(worst, np.abs(np.linalg.eigvalsh(D) - pr.cubic_omega2(q)).max())
    print(f'analytic lattice: max |d omega^2| = {worst:.2e}')
    assert worst <= 1e-12


def test_commensurate_q_reproduce_the_supercell_spectrum():
    S, m = pr.TRICLINIC_S, pr.TRICLINIC_MASSES
    H, fc = pr.random_crystal(2, S, seed=5)
    table = pr.image_table(pr.TRICLINIC_POS, pr.TRICLINIC_CELL, S)
    ev = []
    for q in pr.commensurate_q(S):
        ev.extend(np.linalg.eigvalsh(pr.dynamical_matrix(fc, pr.TRICLINIC_POS, pr.TRICLINIC_CELL, S, m, q, table)))
    want = pr.supercell_eigenvalues(H, m, 18)
    assert len(ev) == 108 == len(want)
    err = np.abs(np.sort(ev) - want).max()
    # D before the symmetrisation is already Hermitian at a generic q
    q = np.array([0.137, -0.291, 0.418])
    D0 = np.zeros((6, 6), dtype=np.complex128)
    for (i, J), xs in table.items():
        j = J % 2
        w = sum(np.exp(2j * np.pi * float(q @ x)) for x in xs) / len(xs)
        D0[3 * i:3 * i + 3, 3 * j:3 * j + 3] += fc[i, :, J, :] * w / np.sqrt(m[i] * m[j])
    herm = np.abs(D0 - D0.conj().T).max()
    print(f'commensurate union: {err:.2e}; Hermitian at a generic q: {herm:.2e}')
    assert err <= 1e-12 * max(1.0, np.abs(want).max()) and herm <= 1e-12


def test_supercell_order_and_image_table_match_the_yardstick():
    for pos, cell, S in ((pr.TRICLINIC_POS, pr.TRICLINIC_CELL, (3, 2, 3)), (pr.TRICLINIC_POS, pr.TRICLINIC_CELL, (1, 2, 1)),
                         (pr.cubic_lattice()[1], pr.cubic_lattice()[2], pr.CUBIC_S)):
        n = len(pos)
        z = np.arange(1, n + 1)
        zs, ps, cs = ph.build_supercell(z, pos, cell, S)
        zr, pr_, cr = pr.build_supercell(z, pos, cell, S)
        assert np.array_equal(zs, zr) and np.allclose(ps, pr_, rtol=0, atol=1e-13) and np.allclose(cs, cr, rtol=0, atol=0)
        assert np.array_equal(ps[:n], np.asarray(pos, dtype=np.float64))                  # the home cell first, untouched
        assert [tuple(r) for r in ph.lattice_offsets(S).tolist()] == pr.lattice_offsets(S)
        start, off = ph.image_table(pos, cell, S)
        want = pr.image_table(pos, cell, S)
        N = len(zs)
        assert start.dtype == np.int32 and start.shape == (n * N + 1,) and start[0] == 0 and start[-1] == len(off)
        for i in range(n):
            for J in range(N):
                got = off[start[i * N + J]:start[i * N + J + 1]]
                assert len(got) == len(want[(i, J)]) >= 1
                assert np.allclose(got, np.array(want[(i, J)]), rtol=0, atol=1e-13)
    # the S = 2 axis of the cubic lattice: two equally near images, +1 and -1 lattice vectors away
    fc, pos, cell = pr.cubic_lattice()
    start, off = ph.image_table(pos, cell, pr.CUBIC_S)
    J = pr.lattice_offsets(pr.CUBIC_S).index((1, 0, 0))
    assert np.array_equal(off[start[J]:start[J + 1]], np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]))


def test_perpendicular_widths():
    w = ph.perpendicular_widths(pr.TRICLINIC_CELL)
    inv = np.linalg.inv(pr.TRICLINIC_CELL)
    assert np.allclose(w, 1.0 / np.linalg.norm(inv, axis=0), rtol=1e-13)
    assert np.allclose(ph.perpendicular_widths(2.5 * np.eye(3)), 2.5)


def test_symmetric_cell_is_a_rigid_rotation():
    pos, cell = ph.symmetric_cell(pr.TRICLINIC_POS, pr.TRICLINIC_CELL)
    assert np.allclose(cell, cell.T, rtol=0, atol=1e-14) and np.all(np.linalg.eigvalsh(cell) > 0)
    assert np.allclose(cell @ cell.T, pr.TRICLINIC_CELL @ pr.TRICLINIC_CELL.T, rtol=1e-13)        # lengths and angles kept
    assert np.allclose(pos @ np.linalg.inv(cell), pr.TRICLINIC_POS @ np.linalg.inv(pr.TRICLINIC_CELL), rtol=0, atol=1e-13)
    assert np.isclose(np.linalg.det(cell), np.linalg.det(pr.TRICLINIC_CELL), rtol=1e-13)
    same_pos, same = ph.symmetric_cell(pos, cell)
    assert np.allclose(same, cell, rtol=0, atol=1e-13) and np.allclose(same_pos, pos, rtol=0, atol=1e-13)


def test_grid_and_path_match_the_yardstick():
    for n, shift in (((4, 4, 4), False), ((3, 2, 5), False), ((2, 3, 2), True), ((1, 1, 1), False)):
        g = ph.monkhorst_pack(*n, shift=shift)
        assert g.shape == (n[0] * n[1] * n[2], 3) and np.allclose(g, pr.monkhorst_pack(*n, shift=shift), rtol=0, atol=1e-15)
        assert (g >= -0.5).all() and (g < 0.5).all()
        assert shift or np.array_equal(g[0], np.zeros(3))
    # the unshifted grid of a supercell's shape is its commensurate set (modulo reciprocal lattice vectors)
    d = ph.monkhorst_pack(3, 2, 3) - pr.commensurate_q((3, 2, 3))
    assert np.allclose(d, np.round(d), atol=1e-15)
    points = [[0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0], [0, 0, 0]]
    q, ticks = ph.band_path(points, 7)
    qr, length, tr = pr.band_path(points, 7, pr.TRICLINIC_CELL)
    assert q.shape == (22, 3) and ticks == tr == [0, 7, 14, 21]
    assert np.allclose(q, qr, rtol=0, atol=1e-15) and np.array_equal(q[ticks], np.array(points, dtype=np.float64))
    assert np.allclose(ph.path_length(q, pr.TRICLINIC_CELL), length, rtol=1e-13)
    for bad in (dict(points=[[0, 0, 0]], n_per_segment=3), dict(points=points, n_per_segment=0),
                dict(points=[[0, 0, 0], [np.nan, 0, 0]], n_per_segment=3)):
        with pytest.raises(ValueError):
            ph.band_path(**bad)
    with pytest.raises(ValueError, match='mesh'):
        ph.monkhorst_pack(0, 2, 2)


def test_acoustic_sum_rule_on_torch_tensors():
    rng = np.random.default_rng(2)
    phi = torch.tensor(rng.standard_normal((2, 3, 8, 3)), dtype=torch.float32)
    out = ph.acoustic_sum_rule(phi)
    want = phi.double().clone()
    for i in range(2):
        blk = want[i, :, i, :] - phi.double()[i].sum(dim=1)
        want[i, :, i, :] = 0.5 * (blk + blk.T)
    assert torch.allclose(out.double(), want, rtol=0, atol=1e-6)
    assert torch.equal(out[0, :, 0, :], out[0, :, 0, :].T)
    other = torch.ones(2, 3, 8, 3, dtype=torch.bool)
    other[0, :, 0, :] = other[1, :, 1, :] = False
    assert torch.equal(out[other], phi[other])                    # only the self blocks change
    # force constants that are symmetric in the self block to begin with end up with sum_J Phi(i, J) = 0
    sym = phi.clone()
    for i in range(2):
        sym[i, :, i, :] = 0.5 * (phi[i, :, i, :] + phi[i, :, i, :].T)
        rest = sym[i].sum(dim=1) - sym[i, :, i, :]
        sym[i, :, (i + 2) % 8, :] -= 0.5 * (rest - rest.T)        # make the sum over the others symmetric too
    assert ph.acoustic_sum_rule(sym).double().sum(dim=2).abs().max() <= 1e-5


class _Embedding:
    cutoff = 5.0


class _Layers:
    edge_embedding = _Embedding()


class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force']
    embedding_layers = _Layers()


def _crystal(n=2, b=1, a=4.2):
    pos = torch.tensor(np.random.default_rng(0).uniform(0.0, a, (n * b, 3)), dtype=torch.float32)
    return (torch.ones(n * b, dtype=torch.long), pos, a * torch.eye(3).repeat(b, 1, 1), torch.arange(b).repeat_interleave(n))


def test_model_phonons_validates_before_any_device_work():
    from newtonnet_amd.models.newtonnet import NewtonNet
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    assert callable(NewtonNet.phonons) and callable(MLAseCalculator.phonons)
    z, pos, cell, batch = _crystal()
    ok = _FakeModel()
    train = _FakeModel()
    train.training = True
    with pytest.raises(NotImplementedError, match='eval'):
        ph.phonons(train, z, pos, cell, batch, (3, 3, 3))
    no_energy = _FakeModel()
    no_energy.output_properties = ['direct_force']
    with pytest.raises(NotImplementedError, match='energy'):
        ph.phonons(no_energy, z, pos, cell, batch, (3, 3, 3))
    with pytest.raises(ValueError, match='zero'):
        ph.phonons(ok, z, pos, torch.zeros(1, 3, 3), batch, (3, 3, 3))
    z2, pos2, cell2, batch2 = _crystal(b=2)
    cell2[1] = 0.0
    with pytest.raises(ValueError, match='crystal 1.*zero'):
        ph.phonons(ok, z2, pos2, cell2, batch2, (3, 3, 3))
    skew = cell.clone()
    skew[0, 0, 1] = 0.4
    with pytest.raises(ValueError, match='symmetric'):
        ph.phonons(ok, z, pos, skew, batch, (3, 3, 3))
    for bad in ((3, 0, 3), (3, -1, 3), (3.0, 3.0, 3.0), (3, 3), torch.tensor([[3, 3, 3], [3, 3, 3]])):
        with pytest.raises(ValueError, match='supercell'):
            ph.phonons(ok, z, pos, cell, batch, bad)
    # the width check names the widths: 4.2 A x 1 and 4.2 A x 2 are below 2 x 5 A, 3 x 4.2 A is not (and then the device is asked for)
    with pytest.raises(ValueError, match=r'widths 4\.200, 4\.200, 4\.200 A.*2 x cutoff = 10\.000'):
        ph.phonons(ok, z, pos, cell, batch, (1, 1, 1))
    with pytest.raises(ValueError, match=r'widths 12\.600, 8\.400, 12\.600'):
        ph.phonons(ok, z, pos, cell, batch, (3, 2, 3))
    with pytest.raises(RuntimeError, match='MI355X'):
        ph.phonons(ok, z, pos, cell, batch, (3, 3, 3))
    with pytest.raises(RuntimeError, match='MI355X'):
        ph.phonons(ok, z, pos, cell, batch, torch.tensor([[3, 3, 3]]))
    # a primitive cell above the kernel's bound
    bound = ph.max_dim()
    assert bound % 3 == 0 and bound >= 72
    zb, pb, cb, bb = _crystal(n=bound // 3 + 1, a=12.0)
    with pytest.raises(NotImplementedError, match=r'phonons\.max_dim\(\)'):
        ph.phonons(ok, zb, pb, cb, bb, (1, 1, 1))
    with pytest.raises(ValueError, match='masses'):
        ph.phonons(ok, z, pos, cell, batch, (3, 3, 3), masses=torch.ones(3))
    with pytest.raises(ValueError, match='atomic weight'):
        ph.phonons(ok, torch.tensor([1, 99]), pos, cell, batch, (3, 3, 3))


def test_from_force_constants_and_q_validate_before_any_device_work():
    fc, pos, cell = pr.cubic_lattice()
    p = ph.Phonons.from_force_constants(fc, [1], pos, cell, pr.CUBIC_S, masses=[pr.CUBIC_MASS], device='cpu')
    assert p.counts == [1] and p.sc_counts == [24] and tuple(p.force_constants(0).shape) == (1, 3, 24, 3)
    assert p.fc.dtype == torch.float32 and p.img_off.dtype == torch.float64 and p.img_start.dtype == torch.int32
    with pytest.raises(ValueError, match='finite'):
        p.frequencies([[0.0, float('nan'), 0.0]])
    with pytest.raises(ValueError, match='finite'):
        p.frequencies(torch.tensor([[0.0, float('inf'), 0.0]]))
    with pytest.raises(RuntimeError, match='MI355X'):
        p.frequencies([[0.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match='fc of crystal 0'):
        ph.Phonons.from_force_constants(fc[:, :, :23], [1], pos, cell, pr.CUBIC_S, masses=[2.0], device='cpu')
    with pytest.raises(ValueError, match='supercell'):
        ph.Phonons.from_force_constants(fc, [1], pos, cell, (2, 3, 0), masses=[2.0], device='cpu')
    with pytest.raises(ValueError, match='zero'):
        ph.Phonons.from_force_constants(fc, [1], pos, np.zeros((3, 3)), pr.CUBIC_S, masses=[2.0], device='cpu')
    with pytest.raises(ValueError, match='batch'):
        ph.Phonons.from_force_constants([fc, fc], [1, 1], np.zeros((2, 3)), np.stack([cell, cell]), pr.CUBIC_S, device='cpu')
    n = ph.max_dim() // 3 + 1
    with pytest.raises(NotImplementedError, match=r'phonons\.max_dim\(\)'):
        ph.Phonons.from_force_constants(np.zeros((n, 3, n, 3)), [1] * n, np.random.default_rng(0).uniform(0, 9, (n, 3)), 9.0 * np.eye(3),
                                        (1, 1, 1), device='cpu')


def test_kernel_symbols_are_declared_listed_and_exported():
    from newtonnet_amd import abi, hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    for name in ('nnhip_phonon_bands', 'nnhip_phonon_dos', 'nnhip_phonon_max_dim'):
        assert name in declared and name in abi.FUNCTIONS and name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bphonon\b.*\)', f.read(), re.M)
    lib.nnhip_phonon_max_dim.restype = ctypes.c_int
    assert lib.nnhip_phonon_max_dim() == ph.max_dim() >= 72
    # the bound is refused by the library itself as well, from the host offsets and before any launch
    hip.abi.bind(lib, ('nnhip_phonon_bands', 'nnhip_last_error'))
    n = ph.max_dim() // 3 + 1
    host = (ctypes.c_int32 * 2)(0, n)
    one = ctypes.c_void_p(8)        # never dereferenced: the size check comes first
    rc = lib.nnhip_phonon_bands(one, one, one, host, one, one, one, one, None, one, 1, one, 1, one, None, None, one, one, None)
    assert rc == 2 and str(ph.max_dim()) in lib.nnhip_last_error().decode()


# ---- the yardstick functions of tests/test_hip_crystal_stages.py --------------------------------------------------------------

def test_vectorised_image_table_is_the_loop_version():
    cases = [(pr.TRICLINIC_POS, pr.TRICLINIC_CELL, (3, 2, 3)), (pr.cubic_lattice()[1], pr.cubic_lattice()[2], pr.CUBIC_S),
             pr.tie_crystal()[1:4], pr.stage_case(9, 12)[1:4], pr.stage_case(27, 8)[1:4]]
    for pos, cell, S in cases:
        slow, fast = pr.image_table(pos, cell, S), pr.image_table_fast(pos, cell, S)
        assert list(slow) == list(fast)
        for key in slow:
            assert len(slow[key]) == len(fast[key]) >= 1
            assert np.array_equal(np.array(slow[key]), np.array(fast[key])), key
    # ... and the product's own table holds the same images for a large cell
    fc, pos, cell, S, _ = pr.stage_case(ph.max_dim(), 9)
    start, off = ph.image_table(pos, cell, S)
    want = pr.image_table_fast(pos, cell, S)
    N = fc.shape[2]
    assert all(np.allclose(off[start[i * N + J]:start[i * N + J + 1]], np.array(want[(i, J)]), rtol=0, atol=1e-13) for (i, J) in want)


def test_stage_grid_cases():
    """the planted crystals of the dimension and copy grid: the shapes, the supercells' copy counts, and a far wave vector whose
    phase the reference still resolves (q and q minus a reciprocal lattice vector give the same spectrum to 1e-9 of its scale:
    the two D differ by the gauge exp(2 pi i G . (f_j - f_i)))"""
    for nR, S in pr.STAGE_SUPERCELLS.items():
        assert int(np.prod(S)) == nR == len(pr.lattice_offsets(S))
    for d, nR in ((27, 8), (30, 9), (33, 12)):
        fc, pos, cell, S, m = pr.stage_case(d, nR)
        assert fc.shape == (d // 3, 3, d // 3 * nR, 3) and fc.dtype == np.float32 and m.dtype == np.float32 and len(set(m.tolist())) > 1
        assert np.abs(cell - np.diag(np.diag(cell))).max() > 0.3
    assert pr.STAGE_Q.shape == (5, 3) and np.abs(pr.STAGE_Q[4]).max() > 1e4
    fc, pos, cell, S, m = pr.stage_case(9, 12)
    table = pr.image_table_fast(pos, cell, S)
    far = pr.dynamical_matrix(fc.astype(np.float64), pos, cell, S, m.astype(np.float64), pr.STAGE_Q[4], table)
    near = pr.dynamical_matrix(fc.astype(np.float64), pos, cell, S, m.astype(np.float64), pr.STAGE_Q[4] - np.array([1e5, -3e4, 0.0]), table)
    assert np.abs(np.linalg.eigvalsh(far) - np.linalg.eigvalsh(near)).max() <= 1e-9 * np.abs(near).max()
    assert np.abs(far - near).max() > 0.1          # ... in another gauge


@pytest.mark.parametrize('M', [30, 33])
def test_hard_spectra_in_the_gauge_of_a_crystal(M):
    """tests/vib_ref.hard_spectra as force constants (phonon_ref.gauge_case): the reference D(q) is P^H A P, so its spectrum is that
    of A at every q, and at the generic q the planted full matrices have a large imaginary part"""
    from tests import vib_ref as vr
    for name, (lam, A64, A32) in vr.hard_spectra(M).items():
        fc, pos, cell, S, m = pr.gauge_case(A32)
        f = pos @ np.linalg.inv(cell)
        assert f.min() >= 0.0 and f.max() < 0.4
        table = pr.image_table(pos, cell, S)
        assert all(len(v) == 1 and np.array_equal(v[0], f[J] - f[i]) for (i, J), v in table.items())          # T = 0 everywhere
        A = A32.astype(np.float64)
        scale = max(np.abs(A).max(), 1.0)
        for q in (np.zeros(3), pr.GAUGE_Q):
            D = pr.dynamical_matrix(fc.astype(np.float64), pos, cell, S, m.astype(np.float64), q, table)
            assert np.abs(D - pr.gauge_matrix(A, pos, cell, q)).max() <= 1e-14 * scale
            assert np.abs(np.linalg.eigvalsh(D) - np.linalg.eigvalsh(A)).max() <= 1e-13 * scale, name
        if lam is not None:
            print(f'M = {M} {name}: max |Im D| = {np.abs(D.imag).max():.3f}')
            off = np.abs(A - np.diag(np.diag(A))).max()
            assert np.abs(D.imag).max() >= 0.25 * off, name         # the gauge turns the couplings well away from the real axis
            assert name in ('cluster', 'graded') or np.abs(D.imag).max() >= 0.1, name     # (those two have small couplings)
            assert np.abs(pr.dynamical_matrix(fc.astype(np.float64), pos, cell, S, m.astype(np.float64), np.zeros(3), table).imag).max() == 0.0


def test_tie_crystal_has_every_multiplicity():
    fc, pos, cell, S, m = pr.tie_crystal()
    assert fc.shape == (11, 3, 88, 3) and np.array_equal(pos @ np.linalg.inv(cell) * 16.0, np.round(pos @ np.linalg.inv(cell) * 16.0))
    table = pr.image_table(pos, cell, S)
    assert pr.multiplicities(table) == [1, 2, 4, 8] == pr.multiplicities(pr.image_table_fast(pos, cell, S))
    offs = pr.lattice_offsets(S)
    assert len(table[(0, 11 * offs.index((1, 0, 0)))]) == 2 and len(table[(0, 11 * offs.index((1, 1, 0)))]) == 4
    assert len(table[(0, 11 * offs.index((1, 1, 1)))]) == 8
    assert len(table[(0, 11 * offs.index((1, 0, 0)) + 1)]) == 2          # atoms 0 and 1 share their x: a tie between DIFFERENT atoms
    assert len(table[(1, 11 * offs.index((1, 1, 0)) + 2)]) == 4          # atoms 1 and 2 share x and y
    start, off = ph.image_table(pos, cell, S)
    assert sorted(set(np.diff(start).tolist())) == [1, 2, 4, 8]
    for (i, J), v in table.items():
        assert np.array_equal(off[start[i * 88 + J]:start[i * 88 + J + 1]], np.array(v))


def test_dos_yardstick_and_the_margin_of_its_inputs():
    # exact cases: width 1/4, every edge exact
    for n_bins in (1, 4, 257):
        hi = n_bins / 4.0
        v = np.array([0.0, hi, np.nextafter(np.float32(0.0), np.float32(-1.0)), np.nextafter(np.float32(hi), np.float32(np.inf)),
                      np.nan, np.inf, -np.inf] + [k / 4.0 for k in range(n_bins)], dtype=np.float32)
        c = pr.dos_counts(v, 0.0, hi, n_bins)
        want = np.ones(n_bins, dtype=np.int64)
        want[0] += 1
        want[-1] += 1
        assert np.array_equal(c, want)
    rng = np.random.default_rng(0)
    x = rng.uniform(-3.0, 7.0, 500)
    edges = -3.0 + 10.0 / 50 * np.arange(51)
    assert np.array_equal(pr.dos_counts(x, -3.0, 7.0, 50), np.histogram(x, bins=edges)[0])
    for n_bins in (1, 255, 256, 257, 1000):
        v, margin = pr.dos_values(600, -37.3, 912.7, n_bins, seed=n_bins)
        lo, hi = np.float32(-37.3), np.float32(912.7)
        assert v.dtype == np.float32 and margin == 8 * pr.EPS32 * n_bins
        assert pr.dos_quotient_margin(v, lo, hi, n_bins) > margin
        assert (v < lo).sum() >= 5 and (v > hi).sum() >= 5 and ((v >= lo) & (v <= hi)).sum() >= 400
        assert pr.dos_counts(v, lo, hi, n_bins).sum() == ((v >= lo) & (v <= hi)).sum()
    # the Gaussian form integrates to the number of values when the range holds them, and its error model is positive
    g, model = pr.dos_gaussian(x, -13.0, 17.0, 3000, 0.5, with_model=True)
    assert abs(g.sum() * 0.01 - 500) <= 1e-6 * 500 and (model > 0).all() and model.max() <= 1e-4 * g.max()


def test_wrapper_takes_a_crystal_slot_without_atoms():
    a, b = pr.stage_case(3, 1), pr.stage_case(6, 8)
    p = ph.Phonons.from_force_constants([a[0], np.zeros((0, 3, 0, 3), np.float32), b[0]], np.ones(3, dtype=np.int64),
                                        np.concatenate([a[1], b[1]]), np.stack([a[2], a[2], b[2]]), np.array([a[3], (2, 2, 2), b[3]]),
                                        masses=np.concatenate([a[4], b[4]]), batch=np.array([0, 2, 2]), device='cpu')
    assert p.counts == [1, 0, 2] and p.sc_counts == [1, 0, 16] and p.cry_ptr.tolist() == [0, 1, 1, 3]
    assert p.img_ptr.tolist() == [0, 2, 3] and p.out_ptr.tolist() == [0, 9, 9]
