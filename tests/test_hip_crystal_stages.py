"""The phonon and elastic kernels (csrc/phonon.hip: nnhip_phonon_bands, nnhip_phonon_dos; csrc/elastic.hip: nnhip_elastic_fold,
nnhip_elastic_relax) at the sizes where they change form, each against the fp64 yardsticks of tests/phonon_ref.py and
tests/elastic_ref.py (held to themselves on the CPU in tests/test_phonon_host.py and tests/test_elastic_host.py).

Forms of nnhip_phonon_bands.  Mp = d rounded up to even.  Mp <= 32: one wave per problem, four problems per workgroup, their four
LDS slots side by side (d = 30 is the one size at which the four together pass 64 KiB, the opt-in limit of dynamic LDS); above, a
workgroup per problem (64 KiB is crossed between d = 60 and d = 63).  The phase factors of the supercell copies are staged eight
copies at a time in the LDS the eigenvectors take later; without modes that chunk buffer alone sizes the region.

Bounds (none of them new).  Assembly, per element: phonon_ref.dynamical_matrix(with_bound=True).  Eigenvalues and residuals:
vib_ref.solver_bound(2 d, ||D||_2) + ||B||_F; orthogonality 2 d x 8 eps32; the phase convention: check_spectrum of
tests/test_hip_phonons.py, imported.  Histogram: equal to the fp64 count, the inputs drawn with a margin (phonon_ref.dos_values).
Gaussian density: DOS_C x the fp32 error model of phonon_ref.dos_gaussian.  Fold: the fp64 sum rounded once (check_stage of
tests/test_hip_elastic.py).  Relaxation on GIVEN eigenpairs: the rounding of R plus d 2^-52 of the term magnitudes
(elastic_ref.relaxation_from_eigenpairs).  Direct library calls start from outputs filled with a sentinel bit pattern, so
"not written" is checked as such.  Every ratio of an error to its bound is printed per case and summed up in STAGE-SUMMARY lines."""
import numpy as np
import pytest
import torch

from newtonnet_amd import elastic as el
from newtonnet_amd import hip
from newtonnet_amd import phonons as ph
from tests import elastic_ref as er
from tests import phonon_ref as pr
from tests import vib_ref as vr
from tests.test_hip_dense_stages import SENT, _stop_after_a_gpu_fault  # noqa: F401  (the fixture is autouse here too)
from tests.test_hip_phonons import check_spectrum, eig_bound

pytestmark = pytest.mark.gpu

EPS32 = vr.EPS32
OK, E_INVALID, E_UNSUPPORTED = 0, 1, 2
ST_SWEEPS, ST_SIZE, ST_MASS = (hip.abi.CONSTANTS['NNHIP_EIG_STATUS_' + k] for k in ('SWEEPS', 'SIZE', 'MASS'))
FOLD_SIZE = hip.abi.CONSTANTS['NNHIP_ELASTIC_STATUS_SIZE']
RATIOS = {}
_REF = {}
# Constant of the Gaussian density's error model (phonon_ref.dos_gaussian): DOS_C = 4 x the largest measured
# |device - fp64| / model over the bin counts and widths of test_dos_random_values (the convention of STAGE_C in
# tests/test_hip_elastic.py).  Measured, largest per n_bins over the four widths and both crystals:
# n_bins 1: 0.035, 255: 0.296 (a tenth of a bin wide), 256: 0.147, 257: 0.199, 1000: 0.225.
DOS_C = 4 * 0.296


def note(stage, form, ratio):
    RATIOS[(stage, form)] = max(RATIOS.get((stage, form), 0.0), float(ratio))


def form_of(d):
    mp = (d + 1) & ~1
    return f'{"wave" if mp <= 32 else "workgroup"} d = {d}'


def empty_case():
    return np.zeros((0, 3, 0, 3), np.float32), np.zeros((0, 3)), pr.STAGE_CELL.copy(), (1, 1, 1), np.zeros(0, np.float32)


def make(cases, masses=None):
    """one Phonons on the device from a list of (fc, pos, cell, S, masses)"""
    counts = [len(c[1]) for c in cases]
    return ph.Phonons.from_force_constants([c[0] for c in cases], np.ones(sum(counts), dtype=np.int64),
                                           np.concatenate([c[1].reshape(-1, 3) for c in cases]), np.stack([c[2] for c in cases]),
                                           np.array([c[3] for c in cases]), masses=np.concatenate([c[4] for c in cases]) if masses is None else masses,
                                           batch=np.repeat(np.arange(len(cases)), counts), device='cuda')


def reference(key, case, q):
    """[(D fp64, assembly bound)] per q from the fp32 force constants and masses the device holds; computed once per key"""
    if key not in _REF:
        fc, pos, cell, S, m = case
        table = pr.image_table_fast(pos, cell, S)
        _REF[key] = [pr.dynamical_matrix(fc.astype(np.float64), pos, cell, S, m.astype(np.float64), x, table, with_bound=True) for x in q]
    return _REF[key]


def judge(stage, form, what, D, B, Dd, ev, modes):
    """one problem: D on the device exactly Hermitian and within the assembly bound, the spectrum within check_spectrum's bounds;
    returns (assembly ratio, solver ratio)"""
    d = D.shape[0]
    assert np.array_equal(Dd, Dd.conj().T), f'{what}: D(q) on the device is not exactly Hermitian'
    diff = np.abs(Dd.astype(np.complex128) - D)
    assert np.all(diff <= B), f'{what}: |dD| exceeds the assembly bound by {np.max(diff - B):.3e}'
    r_asm = float(np.max(diff / np.where(B > 0, B, 1.0)))
    err, bound = check_spectrum(D, B, ev, modes, what)
    V = np.asarray(modes, dtype=np.complex128)
    res = np.linalg.norm(D @ V.T - V.T * np.asarray(ev, dtype=np.float64)[None, :], axis=0).max()
    orth = np.abs(V @ V.conj().T - np.eye(d)).max()
    r_sol = max(err / bound, res / bound, orth / (2 * d * EPS32 * 8))
    note(stage + ' assembly', form, r_asm)
    note(stage + ' solver', form, r_sol)
    return r_asm, r_sol


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. nnhip_phonon_bands: assembly and solver per form ---------------------------------------------------------------------------

GRID = [(d, c) for d in (27, 30, 33) for c in (1, 8, 9, 12, 27)] + [(60, 9), (63, 9), (93, 12), ('max', 9), ('max', 27)]


@pytest.mark.parametrize('d,copies', GRID)
def test_assembly_and_solver_per_form(d, copies):
    """either side of the wave / workgroup switch (30 | 33), of the 64 KiB opt-in in both forms (27 | 30, 60 | 63), odd d in the
    workgroup form (33, 63, 93), and the copies in chunks of eight: one short chunk (1), exactly one (8), one and one copy (9),
    one and a half (12), three and a remainder (27) -- at d = max_dim() the chunk buffer is at its largest"""
    d = ph.max_dim() if d == 'max' else d
    case = pr.stage_case(d, copies)
    q = pr.STAGE_Q
    p = make([case])
    assert p.sc_counts == [d // 3 * copies]
    full = p.frequencies(q, modes=True, dynamical_matrix=True)
    assert int(full.status.abs().max()) == 0 and int(full.sweeps.min()) >= 1
    ev, _, modes = (x.cpu().numpy() for x in full.crystal(0))
    Dd = full.dynamical(0).cpu().numpy()
    worst = [0.0, 0.0]
    for k, (D, B) in enumerate(reference(('grid', d, copies), case, q)):
        r = judge('bands', form_of(d), f'd = {d} copies {copies} q {k}', D, B, Dd[k], ev[k], modes[k])
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f'STAGE-RATIO bands [{form_of(d)}] copies {copies}: assembly {worst[0]:.3f} solver {worst[1]:.3f} sweeps {full.sweeps.cpu().tolist()}')
    # without modes the chunk buffer alone sizes the shared region; the eigenvalues and the sweeps keep every bit
    plain = p.frequencies(q)
    assert plain.modes is None and same_bits(plain.eigenvalues, full.eigenvalues) and torch.equal(plain.sweeps, full.sweeps)
    assert int(plain.status.abs().max()) == 0
    d_only = p.frequencies(q, dynamical_matrix=True)
    assert same_bits(d_only.eigenvalues, full.eigenvalues) and torch.equal(d_only.sweeps, full.sweeps)
    assert same_bits(torch.view_as_real(d_only.dynamical_matrix), torch.view_as_real(full.dynamical_matrix))


@pytest.mark.parametrize('M', [30, 33])
def test_hard_spectra_through_the_complex_path(M):
    """vib_ref.hard_spectra in the gauge of a crystal (phonon_ref.gauge_case): at Gamma the solver gets the real matrix, at the
    generic q the same spectrum in a genuinely complex one.  Both are held to the reference D (check_spectrum: eigenvalues,
    residual, orthogonality, phase -- for the degenerate cases no single vector is compared) and, where a spectrum was planted, to
    it within ||A32 - A64||_2 plus check_spectrum's eigenvalue bound.  The diagonal cases are exact."""
    cases = vr.hard_spectra(M)
    names = list(cases)
    crystals = [pr.gauge_case(cases[k][2]) for k in names]
    q = np.stack([np.zeros(3), pr.GAUGE_Q])
    bands = make(crystals).frequencies(q, modes=True, dynamical_matrix=True)
    assert bool(torch.isfinite(bands.eigenvalues).all()) and bool(torch.isfinite(torch.view_as_real(bands.modes)).all())
    assert int(bands.status.abs().max()) == 0
    sweeps = bands.sweeps.cpu().numpy()
    eye = np.eye(M, dtype=np.complex64)
    for slot, k in enumerate(names):
        lam, A64, A32 = cases[k]
        ev, _, modes = (x.cpu().numpy() for x in bands.crystal(slot))
        Dd = bands.dynamical(slot).cpu().numpy()
        assert np.count_nonzero(Dd[0].imag) == 0, f'{k}: D(Gamma) is real'
        for iq, (D, B) in enumerate(reference(('gauge', M, k), crystals[slot], q)):
            path = 'real' if iq == 0 else 'complex'
            r = judge('hard spectra', f'{form_of(M)} {path}', f'M = {M} {k} {path}', D, B, Dd[iq], ev[iq], modes[iq])
            if lam is not None:
                lim = np.linalg.norm(A32.astype(np.float64) - A64, 2) + eig_bound(D, B)
                err = np.abs(ev[iq].astype(np.float64) - lam).max()
                note('hard spectra planted', f'{form_of(M)} {path}', err / lim)
                assert err <= lim, f'M = {M} {k} {path}: {err:.3e} from the planted spectrum, allowed {lim:.3e}'
                if iq == 1:
                    assert np.abs(Dd[1].imag).max() >= 0.2 * np.abs(A32 - np.diag(np.diag(A32))).max(), f'{k}: the device saw a real matrix'
            print(f'STAGE-RATIO hard spectra [{form_of(M)} {path}] {k}: assembly {r[0]:.3f} solver {r[1]:.3f} sweeps {int(sweeps[slot, iq])}')
            if k == 'equal':
                assert sweeps[slot, iq] == 0 and np.array_equal(ev[iq], np.full(M, 2.0, np.float32)) and np.array_equal(modes[iq], eye)
            elif k == 'diagonal_descending':
                assert sweeps[slot, iq] == 0 and np.array_equal(ev[iq], np.arange(1, M + 1, dtype=np.float32))
                assert np.array_equal(modes[iq], eye[::-1])                    # a permutation, every phase 1
            elif k == 'tiny_coupling':
                assert sweeps[slot, iq] == 0 and np.array_equal(ev[iq], np.sort(np.diag(A32)))
            elif k == 'tiny_and_plain_coupling':
                assert sweeps[slot, iq] >= 1
            elif k == 'negative':
                assert (ev[iq] < 0).all()


def test_equally_near_images_in_a_larger_cell():
    """11 atoms (d = 33) on a 2 x 2 x 2 supercell with 1, 2, 4 and 8 equally near images of a pair, read from the table the
    device is given"""
    case = pr.tie_crystal()
    p = make([case])
    mult = np.diff(p.img_start.cpu().numpy())
    assert sorted(set(mult.tolist())) == [1, 2, 4, 8] and len(mult) == 11 * 88
    q = pr.STAGE_Q
    bands = p.frequencies(q, modes=True, dynamical_matrix=True)
    assert int(bands.status.abs().max()) == 0
    ev, _, modes = (x.cpu().numpy() for x in bands.crystal(0))
    Dd = bands.dynamical(0).cpu().numpy()
    for k, (D, B) in enumerate(reference('tie', case, q)):
        r = judge('bands ties', form_of(33), f'tie crystal q {k}', D, B, Dd[k], ev[k], modes[k])
        print(f'STAGE-RATIO bands ties [{form_of(33)}] q {k}: assembly {r[0]:.3f} solver {r[1]:.3f}')


def crystal_bits(bands, b):
    ev, _, modes = bands.crystal(b)
    return ev.contiguous().view(torch.int32).cpu(), torch.view_as_real(modes).contiguous().view(torch.int32).cpu(), bands.sweeps[b].cpu()


def test_packing_and_independence():
    """d = 3, 30, 33, max_dim() and a slot without atoms in one launch at five wave vectors (the wave form's last workgroup holds
    one problem): every crystal alone, and the batch in reversed order, give the same bits; a second call repeats the first"""
    cases = [pr.stage_case(3, 8), pr.stage_case(30, 9), empty_case(), pr.stage_case(33, 8), pr.stage_case(ph.max_dim(), 1)]
    q = pr.STAGE_Q
    p = make(cases)                                  # the wrapper takes the empty slot (tests/test_phonon_host.py)
    assert p.counts == [1, 10, 0, 11, ph.max_dim() // 3]
    first = p.frequencies(q, modes=True)
    again = p.frequencies(q, modes=True)
    assert int(first.status.abs().max()) == 0
    assert same_bits(first.eigenvalues, again.eigenvalues) and same_bits(torch.view_as_real(first.modes), torch.view_as_real(again.modes))
    assert torch.equal(first.sweeps, again.sweeps)
    assert first.sweeps[2].tolist() == [0] * 5 and first.status[2].tolist() == [0] * 5 and first.crystal(2)[0].numel() == 0
    back = make(cases[::-1]).frequencies(q, modes=True)
    for b, case in enumerate(cases):
        want = crystal_bits(first, b)
        rev = crystal_bits(back, len(cases) - 1 - b)
        assert all(torch.equal(x, y) for x, y in zip(want, rev)), f'crystal {b} depends on its slot'
        if len(case[1]):
            one = crystal_bits(make([case]).frequencies(q, modes=True), 0)
            assert all(torch.equal(x, y) for x, y in zip(want, one)), f'crystal {b} alone differs from the batch'
            assert int(want[2].min()) >= 1
    # the library itself leaves the empty slot's rows of sweeps and status as the caller filled them
    rc, out = call_bands(p, q)
    assert rc == OK and bool((out['sweeps'][2] == SENT).all()) and bool((out['status'][2] == SENT).all())
    for b in (0, 1, 3, 4):
        assert torch.equal(out['sweeps'][b].cpu(), first.sweeps[b].cpu()) and out['status'][b].tolist() == [0] * 5


# ---- direct library calls ----------------------------------------------------------------------------------------------------------

BAND_ARGS = ('fc', 'fc_ptr', 'cry_ptr', 'cry_ptr_host', 'sc_atoms', 'img_ptr', 'img_start', 'img_off', 'masses', 'out_ptr', 'n_cry',
             'q', 'n_q', 'evals', 'modes', 'dmat', 'sweeps', 'status')


def sentinel(shape, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=torch.int32, device='cuda').view(dtype)


def untouched(t):
    return bool((t.contiguous().view(torch.int32) == SENT).all())


def call_bands(p, wave_vectors, modes=True, dmat=True, **override):
    """nnhip_phonon_bands on the tables of the Phonons p with every output buffer filled with the sentinel first; override: any
    argument by name (a tensor, an integer, or None for a null pointer)"""
    q = np.asarray(wave_vectors, dtype=np.float64).reshape(-1, 3)
    Q, B = len(q), len(p.counts)
    n_val, n_sq = 3 * sum(p.counts), sum(9 * n * n for n in p.counts)
    out = dict(evals=sentinel((max(Q, 1) * n_val,)), modes=sentinel((max(Q, 1) * n_sq, 2)) if modes else None,
               dmat=sentinel((max(Q, 1) * n_sq, 2)) if dmat else None, sweeps=sentinel((B, max(Q, 1)), torch.int32),
               status=sentinel((B, max(Q, 1)), torch.int32))
    args = dict(fc=p.fc, fc_ptr=p.fc_ptr, cry_ptr=p.cry_ptr, cry_ptr_host=p._cry_host, sc_atoms=p.sc_atoms, img_ptr=p.img_ptr,
                img_start=p.img_start, img_off=p.img_off, masses=p.masses, out_ptr=p.out_ptr, n_cry=B,
                q=torch.tensor(q if Q else np.zeros((1, 3)), dtype=torch.float64).cuda(), n_q=Q, **out)
    args.update(override)
    keep = {k: (torch.tensor(v, dtype=torch.int32) if k == 'cry_ptr_host' and v is not None and not isinstance(v, torch.Tensor) else v) for k, v in args.items()}
    raw = [v.data_ptr() if isinstance(v, torch.Tensor) else v for v in (keep[k] for k in BAND_ARGS)]
    rc = hip.lib().nnhip_phonon_bands(*raw, hip._stream(p.fc.device))
    torch.cuda.synchronize()
    return rc, out


def slices(p, out, b, Q):
    """the parts of the raw outputs that belong to crystal b: evals, modes, dmat, sweeps, status"""
    n = p.counts[b]
    o, s = 3 * int(p.cry_ptr[b]), p._sq_offsets[b]
    return (out['evals'][Q * o:Q * (o + 3 * n)], out['modes'][Q * s:Q * (s + 9 * n * n)], out['dmat'][Q * s:Q * (s + 9 * n * n)],
            out['sweeps'][b], out['status'][b])


def assert_same_crystal(p, got, want, b, Q, what):
    for x, y in zip(slices(p, got, b, Q), slices(p, want, b, Q)):
        assert same_bits(x, y), f'{what}: crystal {b} changed'


def assert_flagged(p, out, b, Q, bit, what):
    ev, modes, dmat, sweeps, status = slices(p, out, b, Q)
    assert status.tolist() == [bit] * Q and sweeps.tolist() == [0] * Q, f'{what}: status {status.tolist()} sweeps {sweeps.tolist()}'
    assert untouched(ev) and untouched(modes) and untouched(dmat), f'{what}: outputs of the flagged crystal were written'


def three_crystals():
    """a wave-form, a workgroup-form and another wave-form crystal: d = 9 on 8 copies, d = 33 on one, d = 6 on 9"""
    return make([pr.stage_case(9, 8), pr.stage_case(33, 1), pr.stage_case(6, 9)])


def test_null_masses_are_unit_masses():
    p = three_crystals()
    q = pr.STAGE_Q
    rc1, ones = call_bands(p, q, masses=torch.ones(sum(p.counts), device='cuda'))
    rc0, null = call_bands(p, q, masses=None)
    assert rc0 == rc1 == OK and not untouched(ones['evals'])
    for k in ('evals', 'modes', 'dmat', 'sweeps', 'status'):
        assert same_bits(ones[k], null[k]), k
    assert int(null['status'].abs().max()) == 0


@pytest.mark.parametrize('bad', [1, 2], ids=['workgroup form', 'wave form'])
def test_bad_mass_flags_its_crystal_alone(bad):
    p = three_crystals()
    q = pr.STAGE_Q
    rc, clean = call_bands(p, q)
    assert rc == OK and int(clean['status'].abs().max()) == 0
    for value in (0.0, -1.0, float('nan'), float('inf')):
        m = p.masses.clone()
        m[int(p.cry_ptr[bad]) + 1] = value
        rc, out = call_bands(p, q, masses=m)
        assert rc == OK
        assert_flagged(p, out, bad, len(q), ST_MASS, f'mass {value}')
        for b in set(range(3)) - {bad}:
            assert_same_crystal(p, out, clean, b, len(q), f'mass {value}')


@pytest.mark.parametrize('value', [float('nan'), float('inf')])
def test_non_finite_force_constants_hit_the_sweep_cap(value):
    p = three_crystals()
    q = pr.STAGE_Q
    _, clean = call_bands(p, q)
    for bad in (1, 2):
        fc = p.fc.clone()
        fc[p._fc_offsets[bad] + 7] = value
        rc, out = call_bands(p, q, fc=fc)
        assert rc == OK
        status, sweeps = out['status'][bad].tolist(), out['sweeps'][bad].tolist()
        print(f'{value} in crystal {bad}: status {status} sweeps {sweeps}')
        assert status == [ST_SWEEPS] * len(q) and max(sweeps) <= 30
        for b in set(range(3)) - {bad}:
            assert_same_crystal(p, out, clean, b, len(q), f'{value} in crystal {bad}')


@pytest.mark.parametrize('layout', ['wave forms only', 'beside a workgroup form'])
def test_size_mismatch_flags_every_problem_of_the_crystal(layout):
    """cry_ptr_host names crystal 1 smaller than the device's cry_ptr does; every buffer has the device's layout.  The launch is
    sized from the host offsets, so the crystal does not fit: NNHIP_EIG_STATUS_SIZE and 0 sweeps for EVERY wave vector, nothing
    else of it written, the others served.  'wave forms only': by the host offsets no crystal needs the workgroup form, so the
    grid has one workgroup per four wave vectors -- fewer than the crystal has problems."""
    if layout == 'wave forms only':
        p = make([pr.stage_case(6, 9), pr.stage_case(33, 1), pr.stage_case(9, 8)])
        host = [0, 2, 2 + 5, 2 + 5 + 3]                  # crystal 1: 5 atoms by the host copy, 11 on the device
    else:
        p = make([pr.stage_case(6, 9), pr.stage_case(63, 9), pr.stage_case(60, 9)])
        host = [0, 2, 2 + 11, 2 + 11 + 20]               # crystal 1: 11 atoms (Mp = 34) by the host copy, 21 (Mp = 64) on the device
    q = pr.STAGE_Q
    _, clean = call_bands(p, q)
    assert int(clean['status'].abs().max()) == 0
    rc, out = call_bands(p, q, cry_ptr_host=host)
    assert rc == OK
    assert_flagged(p, out, 1, len(q), ST_SIZE, layout)
    for b in (0, 2):
        assert_same_crystal(p, out, clean, b, len(q), layout)


def test_refusals_and_empty_calls_write_nothing():
    p = make([pr.stage_case(6, 9), pr.stage_case(33, 1)])
    q = pr.STAGE_Q
    lib = hip.lib()
    refused = [(dict(n_cry=-1), E_INVALID, 'bad arguments'), (dict(n_q=-1), E_INVALID, 'bad arguments'),
               (dict(n_cry=70000), E_UNSUPPORTED, '65535'), (dict(cry_ptr_host=[0, 2, 1]), E_INVALID, 'decreases'),
               (dict(cry_ptr_host=[0, 2, 2 + ph.max_dim() // 3 + 1]), E_UNSUPPORTED, str(ph.max_dim()))]
    refused += [({k: None}, E_INVALID, 'bad arguments') for k in ('fc', 'fc_ptr', 'cry_ptr', 'cry_ptr_host', 'sc_atoms', 'img_ptr',
                                                                  'img_start', 'img_off', 'out_ptr', 'q', 'evals', 'sweeps', 'status')]
    for override, code, text in refused:
        rc, out = call_bands(p, q, **override)
        assert rc == code and text in lib.nnhip_last_error().decode(), (override, rc, lib.nnhip_last_error())
        assert all(untouched(v) for v in out.values() if v is not None), f'{override}: written'
    for override in (dict(n_q=0), dict(n_cry=0), dict(n_cry=0, fc=None, cry_ptr_host=None, evals=None)):
        rc, out = call_bands(p, q, **override)
        assert rc == OK and all(untouched(v) for v in out.values() if v is not None), override
    rc, out = call_bands(p, q, modes=False, dmat=False)
    assert rc == OK and int(out['status'].abs().max()) == 0 and not untouched(out['evals'])       # modes and dmat are optional


# ---- 2. nnhip_phonon_dos -----------------------------------------------------------------------------------------------------------

def call_dos(values, val_ptr, lo, hi, n_bins, width, counts=True, density=True, n_cry=None):
    x = torch.tensor(np.asarray(values, dtype=np.float32)).cuda()
    vp = torch.tensor(val_ptr, dtype=torch.int64).cuda()
    B = len(val_ptr) - 1
    c = sentinel((B, max(n_bins, 1)), torch.int32) if counts else None
    d = sentinel((B, max(n_bins, 1))) if density else None
    rc = hip.lib().nnhip_phonon_dos(x.data_ptr(), vp.data_ptr(), B if n_cry is None else n_cry, lo, hi, n_bins, width, hip._ptr(c),
                                    hip._ptr(d), hip._stream(x.device))
    torch.cuda.synchronize()
    return rc, c, d


@pytest.mark.parametrize('n_bins', [1, 4, 255, 256, 257, 1000])
def test_dos_histogram_exact_cases(n_bins):
    """bins of width 1/4 from 0: every edge is exact in fp32.  k / 4 lands in bin k, hi in the last bin, lo in bin 0; the
    neighbours of lo and hi outside the range, NaN and the infinities are not counted"""
    hi = n_bins / 4.0
    edge = [k / 4.0 for k in range(n_bins)]
    out = [np.nextafter(np.float32(0.0), np.float32(-1.0)), np.nextafter(np.float32(hi), np.float32(np.inf)), np.nan, np.inf, -np.inf]
    v0 = np.array([0.0, hi] + out + edge, dtype=np.float32)
    v2 = np.array(edge[::-1] + out + [hi, hi, 0.0], dtype=np.float32)
    values, val_ptr = np.concatenate([v0, v2]), [0, len(v0), len(v0), len(v0) + len(v2)]
    rc, c, _ = call_dos(values, val_ptr, 0.0, hi, n_bins, 0.0, density=False)
    assert rc == OK
    c = c.cpu().numpy()
    want0 = np.ones(n_bins, dtype=np.int64)
    want0[0] += 1
    want0[-1] += 1
    want2 = np.ones(n_bins, dtype=np.int64)
    want2[0] += 1
    want2[-1] += 2
    assert np.array_equal(c[0], want0) and np.array_equal(c[2], want2) and np.count_nonzero(c[1]) == 0
    assert np.array_equal(c[0], pr.dos_counts(v0, 0.0, hi, n_bins)) and np.array_equal(c[2], pr.dos_counts(v2, 0.0, hi, n_bins))
    note('dos histogram', 'exact edges', 0.0)


@pytest.mark.parametrize('n_bins', [1, 255, 256, 257, 1000])
def test_dos_random_values(n_bins):
    """three crystals, the middle one without values: counts equal to the fp64 histogram (inputs with a margin of 8 eps32 n_bins
    from every edge, nothing excluded), the Gaussian density within its model for widths from a tenth of a bin to the whole
    range, and each output with the same bits alone and beside the other"""
    lo, hi = np.float32(-37.3), np.float32(912.7)
    v0, _ = pr.dos_values(600, lo, hi, n_bins, seed=n_bins)
    v2, _ = pr.dos_values(257, lo, hi, n_bins, seed=n_bins + 7)
    values, val_ptr = np.concatenate([v0, v2]), [0, 600, 600, 857]
    wbin = (float(hi) - float(lo)) / n_bins
    for width in (0.1 * wbin, wbin, 0.05 * float(hi - lo), float(hi - lo)):
        rc, c, d = call_dos(values, val_ptr, float(lo), float(hi), n_bins, width)
        rc1, c1, _ = call_dos(values, val_ptr, float(lo), float(hi), n_bins, 0.0, density=False)
        rc2, _, d2 = call_dos(values, val_ptr, float(lo), float(hi), n_bins, width, counts=False)
        assert rc == rc1 == rc2 == OK and same_bits(c, c1) and same_bits(d, d2)
        c, d = c.cpu().numpy(), d.cpu().numpy().astype(np.float64)
        assert np.count_nonzero(c[1]) == 0 and np.count_nonzero(d[1]) == 0
        for b, v in ((0, v0), (2, v2)):
            assert np.array_equal(c[b], pr.dos_counts(v, lo, hi, n_bins)), f'n_bins {n_bins} crystal {b}: counts'
            want, model = pr.dos_gaussian(v, lo, hi, n_bins, np.float32(width), with_model=True)
            ratio = float((np.abs(d[b] - want) / model).max())
            print(f'STAGE-RATIO dos gaussian [n_bins {n_bins} width {width / wbin:.3g} bins] crystal {b}: |d| / model = {ratio:.3f}')
            note('dos gaussian', f'n_bins {n_bins}', ratio / DOS_C)
            assert ratio <= DOS_C, f'n_bins {n_bins} width {width}: {ratio:.3f} x the model, allowed {DOS_C}'
    note('dos histogram', f'n_bins {n_bins}', 0.0)


def test_dos_refusals_write_nothing():
    v = np.linspace(0.0, 1.0, 7, dtype=np.float32)
    nan, inf = float('nan'), float('inf')
    bad = [dict(n_bins=0), dict(n_bins=-3), dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0), dict(lo=nan), dict(hi=nan), dict(lo=-inf),
           dict(hi=inf), dict(counts=False, density=False), dict(width=0.0), dict(width=-1.0), dict(width=nan), dict(width=inf),
           dict(n_cry=-1)]
    for kw in bad:
        a = dict(lo=0.0, hi=1.0, n_bins=4, width=0.1)
        a.update(kw)
        rc, c, d = call_dos(v, [0, 7], **a)
        assert rc == E_INVALID, kw
        assert (c is None or untouched(c)) and (d is None or untouched(d)), kw
    rc, c, d = call_dos(v, [0, 7], 0.0, 1.0, 4, 0.0, density=False)          # the width is the density's alone
    assert rc == OK and c.cpu().tolist() == [[2, 1, 2, 2]]
    rc, c, d = call_dos(v, [0, 7], 0.0, 1.0, 4, 0.1, n_cry=0)
    assert rc == OK and untouched(c) and untouched(d)


# ---- 3. nnhip_elastic_fold and nnhip_elastic_relax alone ---------------------------------------------------------------------------

FOLD_SPECS = [(n, c) for n in (1, 10, 11, 32) for c in (1, 4, 27)]
FOLD_SPECS.insert(5, (0, 0))


def fold_inputs():
    rng = np.random.default_rng(2024)
    return [rng.standard_normal((n, 3, n * c, 3)).astype(np.float32) for n, c in FOLD_SPECS]


def call_fold(fcs, sc_atoms=None, n_cry=None):
    ns = [f.shape[0] for f in fcs]
    sizes = np.array([f.size for f in fcs], dtype=np.int64)
    sq = np.array([9 * n * n for n in ns], dtype=np.int64)
    fc = torch.tensor(np.concatenate([f.reshape(-1) for f in fcs])).cuda()
    dev = [torch.tensor(a, dtype=t).cuda() for a, t in ((np.cumsum(sizes) - sizes, torch.int64), (np.concatenate([[0], np.cumsum(ns)]), torch.int32),
                                                       ([f.shape[2] for f in fcs] if sc_atoms is None else sc_atoms, torch.int32),
                                                       (np.cumsum(sq) - sq, torch.int64))]
    phi0, status = sentinel((int(sq.sum()),)), sentinel((len(fcs),), torch.int32)
    rc = hip.lib().nnhip_elastic_fold(fc.data_ptr(), *[t.data_ptr() for t in dev], len(fcs) if n_cry is None else n_cry, phi0.data_ptr(),
                                      status.data_ptr(), hip._stream(fc.device))
    torch.cuda.synchronize()
    off = (np.cumsum(sq) - sq).tolist()
    return rc, [phi0[o:o + s] for o, s in zip(off, sq.tolist())], status


def test_fold_alone():
    """1, 4 and 27 copies of 1, 10, 11 and 32 atoms and a slot without atoms in one call: the fp64 sum rounded once (the bound of
    check_stage, tests/test_hip_elastic.py), exactly symmetric, twice the same bits"""
    fcs = fold_inputs()
    rc, phis, status = call_fold(fcs)
    rc2, again, _ = call_fold(fcs)
    assert rc == rc2 == OK and status.tolist() == [0] * len(fcs)
    for (n, c), fc, phi, rep in zip(FOLD_SPECS, fcs, phis, again):
        assert same_bits(phi, rep)
        if n == 0:
            assert phi.numel() == 0
            continue
        d = 3 * n
        got = phi.cpu().numpy().reshape(d, d)
        s = fc.astype(np.float64).reshape(n, 3, c, n, 3).sum(axis=2).reshape(d, d)
        want = 0.5 * (s + s.T)
        terms = np.abs(fc.astype(np.float64)).reshape(n, 3, c, n, 3).sum(axis=2).reshape(d, d)
        bound = EPS32 * np.abs(want) + 2.0 ** -52 * c * (terms + terms.T)
        assert np.array_equal(got, got.T), f'n = {n}, {c} copies: Phi0 not exactly symmetric'
        ratio = float((np.abs(got - want) / bound).max())
        note('fold', f'{c} copies', ratio)
        print(f'STAGE-RATIO fold [{c} copies] n = {n}: {ratio:.3f}')
        assert ratio <= 1.0, f'n = {n}, {c} copies: fold {ratio:.3f} x the bound'
    assert call_fold(fcs, n_cry=0)[0] == OK and all(untouched(x) for x in call_fold(fcs, n_cry=0)[1])


def test_fold_flags_a_supercell_that_is_no_multiple():
    """the status the Python wrapper never sees (it refuses first): sc_atoms of one crystal is no multiple of its atoms, or below
    them -- NNHIP_ELASTIC_STATUS_SIZE, its Phi0 untouched, the others folded with the bits of the clean call"""
    fcs = fold_inputs()
    _, clean, _ = call_fold(fcs)
    for k, wrong in ((FOLD_SPECS.index((11, 4)), 45), (FOLD_SPECS.index((10, 27)), 5), (FOLD_SPECS.index((32, 1)), 33)):
        sc = [f.shape[2] for f in fcs]
        sc[k] = wrong
        rc, phis, status = call_fold(fcs, sc_atoms=sc)
        assert rc == OK and status.tolist() == [FOLD_SIZE if b == k else 0 for b in range(len(fcs))]
        assert untouched(phis[k])
        assert all(same_bits(a, b) for j, (a, b) in enumerate(zip(phis, clean)) if j != k)


def call_relax(items, n_cry=None):
    """nnhip_elastic_relax on planted (evals, modes, Lambda, threshold) per crystal"""
    ds = [len(it[0]) for it in items]
    sq = np.array([d * d for d in ds], dtype=np.int64)

    def cat(k, width):
        return torch.tensor(np.concatenate([np.asarray(it[k], dtype=np.float32).reshape(-1) for it in items] + [np.zeros(width, np.float32)])).cuda()
    ev, Q, lam = cat(0, 1), cat(1, 1), cat(2, 6)
    blk = torch.tensor(np.cumsum(sq) - sq, dtype=torch.int64).cuda()
    cry = torch.tensor(np.concatenate([[0], np.cumsum([d // 3 for d in ds])]), dtype=torch.int32).cuda()
    thr = torch.tensor([it[3] for it in items], dtype=torch.float32).cuda()
    B = len(items)
    R, nz, nn, st = sentinel((B, 6, 6)), sentinel((B,), torch.int32), sentinel((B,), torch.int32), sentinel((B,), torch.int32)
    rc = hip.lib().nnhip_elastic_relax(ev.data_ptr(), Q.data_ptr(), blk.data_ptr(), cry.data_ptr(), lam.data_ptr(), thr.data_ptr(),
                                       B if n_cry is None else n_cry, R.data_ptr(), nz.data_ptr(), nn.data_ptr(), st.data_ptr(), hip._stream(ev.device))
    torch.cuda.synchronize()
    return rc, R, nz.tolist(), nn.tolist(), st.tolist()


def relax_items():
    """d = 3 (three zeros: nothing to sum), 63 with a mode exactly AT the threshold, 66 with a NaN eigenvalue and a negative mode,
    96 plain, 0, and 66 with a negative mode alone"""
    items, names = [], ['d = 3', 'd = 63, a mode at the threshold', 'd = 66, NaN and negative', 'd = 96', 'd = 0', 'd = 66, negative']
    ev, Q, lam = er.planted_eigenpairs(3, seed=3)
    items.append((ev, Q, lam, np.float32(1e-3)))
    ev, Q, lam = er.planted_eigenpairs(63, seed=63)
    items.append((ev, Q, lam, ev[10]))                          # |lambda_10| == threshold: zero, with the ten below it
    ev, Q, lam = er.planted_eigenpairs(66, seed=66, negative=True)
    ev = ev.copy()
    ev[30] = np.nan
    items.append((ev, Q, lam, np.float32(1e-3)))
    ev, Q, lam = er.planted_eigenpairs(96, seed=96)
    items.append((ev, Q, lam, np.float32(1e-3)))
    items.append((np.zeros(0, np.float32), np.zeros((0, 0), np.float32), np.zeros((0, 6), np.float32), np.float32(1e-3)))
    ev, Q, lam = er.planted_eigenpairs(66, seed=67, negative=True)
    items.append((ev, Q, lam, np.float32(1e-3)))
    return items, names


def test_relaxation_alone_on_planted_eigenpairs():
    items, names = relax_items()
    rc, R, nz, nn, st = call_relax(items)
    assert rc == OK
    R = R.cpu().numpy()
    for k, (it, name) in enumerate(zip(items, names)):
        want, wz, wn, bound = er.relaxation_from_eigenpairs(*it)
        assert np.array_equal(R[k], R[k].T) and np.isfinite(R[k]).all(), f'{name}: R not symmetric / not finite'
        assert (nz[k], nn[k]) == (wz, wn), f'{name}: counts {nz[k]}, {nn[k]} against {wz}, {wn}'
        assert st[k] == (el.STATUS_ZERO if wz != 3 else 0) | (el.STATUS_NEGATIVE if wn else 0), f'{name}: status {st[k]}'
        err = np.abs(R[k].astype(np.float64) - want)
        ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
        d = len(it[0])
        note('relaxation', f'd = {d}', ratio)
        print(f'STAGE-RATIO relaxation [d = {d}] {name}: {ratio:.3f}, n_zero {nz[k]}, n_negative {nn[k]}, status {st[k]}')
        assert np.all(err <= bound), f'{name}: |dR| {ratio:.3f} x the bound'
    assert (nz, nn, st) == ([3, 11, 4, 3, 0, 3], [0, 0, 1, 0, 0, 1],
                            [0, el.STATUS_ZERO, el.STATUS_ZERO | el.STATUS_NEGATIVE, 0, el.STATUS_ZERO, el.STATUS_NEGATIVE])
    assert np.count_nonzero(R[0]) == 0 and np.count_nonzero(R[4]) == 0
    # a crystal alone gives the bits it gives in the batch; a second call repeats; no crystals is no work
    for k in (1, 3):
        rc1, R1, nz1, nn1, st1 = call_relax([items[k]])
        assert rc1 == OK and np.array_equal(R1.cpu().numpy()[0].view(np.int32), R[k].view(np.int32)) and (nz1, nn1, st1) == ([nz[k]], [nn[k]], [st[k]])
    assert np.array_equal(call_relax(items)[1].cpu().numpy().view(np.int32), R.view(np.int32))
    rc0, R0, _, _, _ = call_relax(items, n_cry=0)
    assert rc0 == OK and untouched(R0)


def test_zz_ratio_summary():
    assert RATIOS, 'run after the stage tests of this file'
    for (stage, form), v in sorted(RATIOS.items()):
        print(f'STAGE-SUMMARY all | {stage} | {form} | {v:.3f}')
    assert all(v <= 1.0 for v in RATIOS.values())
