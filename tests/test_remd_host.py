"""CPU-side checks of replica exchange (newtonnet_amd/remd.py, csrc/remd.hip): the C ABI exports the kernel and the header's
constant is the Python one, the reference's Philox4x32-10 gives the published known answers and its uniform numbers lie on the
2^-24 grid in [0, 1), arguments are refused before any device work, the exchange the GPU tests compare against
(tests/remd_ref.py) keeps the canonical distribution, and the synthetic input of the GPU kernel test reaches every branch without an
ambiguous decision, so that test can demand every bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import remd_ref as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_symbol_is_declared_listed_and_exported_and_the_constant_agrees():
    from newtonnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'newtonnet_hip.h')).read()
    declared = set(re.findall(r'\b(nnhip_[a-z_0-9]+)\s*\(', header))
    assert 'nnhip_remd_exchange' in declared and 'nnhip_remd_exchange' in hip.EXPORTED_SYMBOLS
    assert hasattr(lib, 'nnhip_remd_exchange')
    with open(os.path.join(ROOT, 'newtonnet_amd', 'csrc', 'build.sh')) as f:
        assert re.search(r'^srcs=\(.*\bremd\b.*\)', f.read(), re.M)
    define = int(re.search(r'#define NNHIP_REMD_MAX_REPLICAS (\S+)', header).group(1))
    assert define == hip.REMD_MAX_REPLICAS == xr.MAX_REPLICAS == 64
    from newtonnet_amd.vibrations import K_BOLTZMANN
    assert K_BOLTZMANN == xr.K_BOLTZMANN


# ---- the random numbers -----------------------------------------------------------------------------------------------------------

KNOWN_ANSWERS = [      # Random123's published vectors for philox4x32-10: counter, key -> output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('counter, key, want', KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    assert xr.philox4x32_10(counter, key) == want
    assert int(xr.philox_word0(*counter, *key)) == want[0]                      # the vectorised form the reference draws from


def test_uniform_numbers_are_in_the_unit_interval_on_the_24_bit_grid():
    rng = np.random.default_rng(0)
    sid, k = rng.integers(0, 2 ** 32, 20000), rng.integers(0, 64, 20000)
    for attempt, seed in ((0, 0), (1, 1), (0xffffffff, 2 ** 64 - 1), (12345, xr.SYN_SEED)):
        u = xr.uniform(attempt, sid, k, seed)
        assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
        scaled = u.astype(np.float64) * 2.0 ** 24
        assert np.array_equal(scaled, np.floor(scaled))
        assert abs(float(u.mean()) - 0.5) < 4.0 / np.sqrt(12 * 20000) and len(np.unique(u)) > 19900
        # the vectorised draw is the scalar one
        for j in (0, 1, 19999):
            w0 = xr.philox4x32_10((attempt, int(sid[j]), int(k[j]), 0), (seed & 0xffffffff, seed >> 32))[0]
            assert float(u[j]) == (w0 >> 8) * 2.0 ** -24
    # the extremes of the map word -> u
    assert (0xffffffff >> 8) * 2.0 ** -24 == float(np.float32((0xffffffff >> 8)) * np.float32(2.0 ** -24)) < 1.0


# ---- arguments ----------------------------------------------------------------------------------------------------------------------

class _FakeModel:
    training = False
    output_properties = ['energy', 'gradient_force']

    def replica_exchange(self, *a, **kw):
        from newtonnet_amd.models import NewtonNet
        return NewtonNet.replica_exchange(self, *a, **kw)


def _inputs(n=3, g=2):
    return (torch.ones(n * g, dtype=torch.long), torch.zeros(n * g, 3), torch.zeros(g, 3, 3), torch.arange(g).repeat_interleave(n))


def test_replica_exchange_validates_before_any_device_work():
    from newtonnet_amd.dynamics import Dynamics
    from newtonnet_amd.remd import ReplicaExchange
    z, pos, cell, batch = _inputs()
    ok = _FakeModel()
    T = [300.0, 350.0, 410.0, 480.0]
    train = _FakeModel()
    train.training = True
    with pytest.raises(ValueError, match='eval'):
        train.replica_exchange(z, pos, cell, batch, T, 5, 0.02)
    energy_only = _FakeModel()
    energy_only.output_properties = ['energy']
    with pytest.raises(ValueError, match='gradient_force'):
        energy_only.replica_exchange(z, pos, cell, batch, T, 5, 0.02)
    with pytest.raises(ValueError, match='pos'):
        ok.replica_exchange(z, torch.zeros(6, 2), cell, batch, T, 5, 0.02)
    with pytest.raises(ValueError, match='fixed'):
        ok.replica_exchange(z, pos, cell, batch, T, 5, 0.02, fixed=torch.zeros(6))
    for bad in ([300.0], np.linspace(300.0, 900.0, 65), [], 300.0):                                   # R outside 2 .. 64
        with pytest.raises(ValueError, match='temperatures'):
            ok.replica_exchange(z, pos, cell, batch, bad, 5, 0.02)
    for bad in ([300.0, 290.0], [0.0, 300.0], [-1.0, 300.0], [300.0, float('nan')], [300.0, float('inf')], ['a', 'b'],
                [[300.0, 350.0], [300.0, 290.0]]):
        with pytest.raises(ValueError, match='temperatures'):
            ok.replica_exchange(z, pos, cell, batch, bad, 5, 0.02)
    for bad in (np.full((3, 4), 300.0), np.full((2, 2, 2), 300.0), torch.full((1, 4), 300.0)):        # a wrong [G, R] shape
        with pytest.raises(ValueError, match='temperatures'):
            ok.replica_exchange(z, pos, cell, batch, bad, 5, 0.02)
    for bad in (0.0, -0.01, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='friction'):
            ok.replica_exchange(z, pos, cell, batch, T, 5, bad)
    for bad in (-1, 2.5, float('nan'), 'x', None, True):
        with pytest.raises(ValueError, match='exchange_every'):
            ok.replica_exchange(z, pos, cell, batch, T, bad, 0.02)
    for bad in (-1, 2 ** 64, 1.5, 'x', None):
        with pytest.raises(ValueError, match='exchange_seed'):
            ok.replica_exchange(z, pos, cell, batch, T, 5, 0.02, exchange_seed=bad)
    with pytest.raises(ValueError, match='timestep'):
        ok.replica_exchange(z, pos, cell, batch, T, 5, 0.02, timestep=0.0)
    for good in (T, np.array(T), torch.tensor(T), [T, T], np.array([T, [t + 5 for t in T]]), [300.0, 300.0]):
        with pytest.raises(RuntimeError, match='MI355X'):                                            # CPU tensors: no CPU path
            ok.replica_exchange(z, pos, cell, batch, good, 5, 0.02)
    with pytest.raises(RuntimeError, match='MI355X'):
        ReplicaExchange(ok, z, pos, cell, batch, T, 0, 0.02, exchange_seed=2 ** 64 - 1)
    # run takes Dynamics's checks of its two numbers, before anything else
    assert ReplicaExchange._recorded_steps is Dynamics._recorded_steps
    for bad in ((-1, 0), (2.5, 0), (3, -1), (3, 1.5)):
        with pytest.raises(ValueError):
            ReplicaExchange._recorded_steps(*bad)
    import inspect
    assert inspect.getsource(ReplicaExchange.run).index('_recorded_steps') < inspect.getsource(ReplicaExchange.run).index('_ensure_state')


def test_calculator_run_remd_validates_before_any_device_work():
    from newtonnet_amd.utils.ase_interface import MLAseCalculator
    from tests.test_ase_calculator import FakeAtoms
    calc = MLAseCalculator.__new__(MLAseCalculator)
    calc.device, calc.dtype = torch.device('cpu'), torch.float32
    calc.model = _FakeModel()
    a, b = FakeAtoms([8, 1, 1], np.zeros((3, 3))), FakeAtoms([6, 1], np.zeros((2, 3)))
    T = [300.0, 400.0]
    with pytest.raises(ValueError, match='at least one'):
        calc.run_remd([], T, 10, 5, 0.02)
    with pytest.raises(ValueError, match='sizes'):
        calc.run_remd([a, b], T, 10, 5, 0.02)
    for bad in ([300.0], [400.0, 300.0], [0.0, 1.0], [300.0, float('nan')], np.full((2, 2), 300.0), np.linspace(1, 2, 65)):
        with pytest.raises(ValueError, match='temperatures'):
            calc.run_remd(a, bad, 10, 5, 0.02)
    with pytest.raises(ValueError, match='friction'):
        calc.run_remd(a, T, 10, 5, 0.0)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match='exchange_every'):
            calc.run_remd(a, T, 10, bad, 0.02)
        with pytest.raises(ValueError, match='n_steps'):
            calc.run_remd(a, T, bad, 5, 0.02)
        with pytest.raises(ValueError, match='record_every'):
            calc.run_remd(a, T, 10, 5, 0.02, record_every=bad)
    with pytest.raises(ValueError, match='exchange_seed'):
        calc.run_remd(a, T, 10, 5, 0.02, exchange_seed=-1)
    with pytest.raises(ValueError, match='timestep'):
        calc.run_remd(a, T, 10, 5, 0.02, timestep=0.0)
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.run_remd(a, T, 10, 5, 0.02)
    with pytest.raises(RuntimeError, match='MI355X'):
        calc.run_remd([a, a], [T, T], 10, 5, 0.02)


def test_ladder_coefficients_are_the_references_and_rounded_once():
    from newtonnet_amd.remd import check_temperatures, ladder_coefficients
    T = check_temperatures([[300.0, 350.0, 410.0, 480.0], [250.0, 250.0, 900.0, 901.0]], 2)
    dbeta, up, down = ladder_coefficients(T)
    for g in range(2):
        for got, want in zip((dbeta[g], up[g], down[g]), xr.coefficients(T[g])):
            assert got.dtype == np.float32 and np.array_equal(got, want)
    assert dbeta[1, 0] == 0.0 and up[1, 0] == down[1, 0] == 1.0 and np.all(dbeta[:, -1] == 0.0) and np.all(up[:, -1] == 1.0)
    k = 1
    want = 1.0 / (xr.K_BOLTZMANN * 350.0) - 1.0 / (xr.K_BOLTZMANN * 410.0)
    assert dbeta[0, k] == np.float32(want) and up[0, k] == np.float32(np.sqrt(410.0 / 350.0))
    assert check_temperatures([300.0, 400.0], 3).shape == (3, 2)


# ---- the exchange keeps the canonical distribution ------------------------------------------------------------------------------------

def _two_attempts(E, dbeta, u_even, u_odd):
    L, R = E.shape
    sor = np.tile(np.arange(R), (L, 1))
    first = xr.attempt_many(E, sor, dbeta, 0, u_even)
    second = xr.attempt_many(E, first['slot_of_rank'], dbeta, 1, u_odd)
    assert not first['ambiguous'].any() and not second['ambiguous'].any()
    return first, second


def test_the_exchange_keeps_the_canonical_distribution():
    """20 000 ladders of R = 4 with independent energies E_k ~ Gamma(10, k_B T_k) -- the canonical distribution of a system with a
    density of states ~ E^9, at every temperature -- go through one even and one odd attempt.  Detailed balance keeps the product
    distribution invariant: the energy found at rank k afterwards still has mean 10 k_B T_k (within 4 standard errors, sigma =
    sqrt(10) k_B T_k), and the acceptance per pair agrees with the same procedure driven by numpy's own fp64 uniforms (within 4
    standard errors of the difference of two proportions).  With the sign of delta flipped in remd_ref.pair_delta this test fails
    (checked by hand: the means move by more than 20 standard errors)."""
    L, R, shape = 20000, 4, 10.0
    T = np.array([300.0, 350.0, 410.0, 480.0])
    rng = np.random.default_rng(20261019)
    E = rng.gamma(shape, xr.K_BOLTZMANN * T, (L, R)).astype(np.float32)
    dbeta = xr.coefficients(T)[0]
    ks, ladder = np.arange(R)[None, :], np.arange(L)[:, None]
    first, second = _two_attempts(E, dbeta, xr.uniform(0, ladder, ks, 7), xr.uniform(1, ladder, ks, 7))
    at_rank = E[ladder, second['slot_of_rank']].astype(np.float64)
    mean, se = at_rank.mean(0), np.sqrt(shape) * xr.K_BOLTZMANN * T / np.sqrt(L)
    dev = (mean - shape * xr.K_BOLTZMANN * T) / se
    moved = float(first['accepted'].mean() + second['accepted'].mean())
    print(f'energy at each rank after two attempts: (mean - 10 k_B T) / standard error = {dev}; swaps per ladder {moved * R:.3f}')
    assert np.all(np.abs(dev) <= 4.0)
    plain, plain2 = _two_attempts(E, dbeta, rng.random((L, R)).astype(np.float32), rng.random((L, R)).astype(np.float32))
    for name, got, ref, pairs in (('even', first, plain, (0, 2)), ('odd', second, plain2, (1,))):
        for k in pairs:
            p, q = got['accepted'][:, k].mean(), ref['accepted'][:, k].mean()
            se_pq = np.sqrt((p * (1 - p) + q * (1 - q)) / L)
            print(f'{name} pair {k}: acceptance {p:.4f} with Philox, {q:.4f} with numpy uniforms, difference {(p - q) / se_pq:+.2f} SE')
            assert 0.05 < p < 0.95 and abs(p - q) <= 4.0 * se_pq
        assert not got['accepted'][:, [k for k in range(R) if k not in pairs]].any()
    # the test has power: an exchange that always accepts breaks the means
    always = xr.attempt_many(E, np.tile(np.arange(R), (L, 1)), dbeta, 0, np.zeros((L, R), dtype=np.float32))
    wrong = E[ladder, always['slot_of_rank']].astype(np.float64).mean(0)
    assert np.abs((wrong - shape * xr.K_BOLTZMANN * T) / se).max() > 20.0


# ---- the fixtures of the device tests -------------------------------------------------------------------------------------------------

def test_synthetic_kernel_input_reaches_every_branch_without_an_ambiguous_decision():
    ladders = xr.synthetic_batch()
    assert len(ladders) == 42 and {(b['R'], b['n']) for b in ladders} == {(R, n) for R in xr.SYN_REPLICAS for n in xr.SYN_SIZES}
    assert {b['kind'] for b in ladders} == set(xr.SYN_KINDS)
    assert [a & 1 for a in xr.SYN_ATTEMPTS] == [0, 1] and xr.SYN_ATTEMPTS[1] >= 2 ** 31 and xr.SYN_SEED >= 2 ** 63
    assert any(b['stream_id'] >= 2 ** 31 for b in ladders) and len({b['stream_id'] for b in ladders}) == 42
    seen = set()
    for attempt in xr.SYN_ATTEMPTS:
        for b, r in zip(ladders, xr.reference(ladders, attempt)):
            assert not r['ambiguous'].any(), (b['kind'], b['R'], b['n'], attempt)
            kind, R = b['kind'], b['R']
            scrambled = not np.array_equal(b['slot_of_rank'], np.arange(R))
            if kind == 'corrupt':
                assert r['skipped'] and np.isnan(r['delta']).all() and not r['accepted'].any()
                assert np.array_equal(r['vel'], b['vel']) and np.array_equal(r['n_attempt'], b['n_attempt'])
                seen.add('skipped')
                continue
            ks = np.arange(attempt & 1, R - 1, 2)
            rest = np.setdiff1d(np.arange(R), ks)
            assert not r['skipped'] and xr.maps_valid(r['rank_of_slot'], r['slot_of_rank'])
            assert not r['delta'][rest].any() and not r['u'][rest].any() and not r['accepted'][rest].any()
            assert np.array_equal(r['n_attempt'] - b['n_attempt'], np.isin(np.arange(R), ks).astype(np.int32))
            assert np.array_equal(r['n_accept'] - b['n_accept'], r['accepted'])
            acc, d = r['accepted'][ks].astype(bool), r['delta'][ks]
            if kind == 'accept':
                assert acc.all() and (d > 0).all()
            elif kind == 'reject':
                assert not acc.any() and (np.exp(d.astype(np.float64)).astype(np.float32) == 0).all()
            elif kind in ('tie_energy', 'tie_temperature'):
                assert acc.all() and (d == 0).all()
                if kind == 'tie_temperature' and len(ks):
                    assert len(set(b['E'].tolist())) == R and (b['scale_up'] == 1).all()
                    seen.add(('tie_temperature', bool(np.signbit(d).any())))
            for k, a_, d_ in zip(ks, acc, d):
                seen.add((kind, bool(a_)))
                if np.isnan(d_):
                    seen.add('nan delta rejects')
                    assert not a_
                if np.isinf(d_):
                    seen.add(('inf delta', bool(a_)))
                    assert a_ == (d_ > 0)
                if -10 < d_ < 0:
                    seen.add(('stochastic', bool(a_)))
            moved = np.zeros(R, dtype=bool)
            for k in ks[acc]:
                moved[b['slot_of_rank'][k]] = moved[b['slot_of_rank'][k + 1]] = True
            # a slot that is not swapped keeps every bit; a swapped one holds its new row, a fixed atom stays at rest
            assert np.array_equal(r['vel'][~moved], b['vel'][~moved]) and np.array_equal(r['sigma'][~moved], b['sigma'][~moved])
            for s in np.nonzero(moved)[0]:
                assert np.array_equal(r['sigma'][s], b['sigma_table'][r['rank_of_slot'][s], s])
                assert r['rank_of_slot'][s] != b['rank_of_slot'][s]
            assert not r['vel'][:, b['fixed']].any() and not r['sigma'][:, b['fixed']].any()
            if kind == 'fixed' and moved.any() and b['fixed'].any():
                seen.add('fixed atoms in a swapped slot')
            seen.add(('maps', scrambled, bool(moved.any())))
            if len(ks) == 0:
                seen.add('a ladder with no pair of this parity')
    want = [('accept', True), ('reject', False), ('tie_energy', True), ('tie_temperature', True), ('stochastic', True),
            ('stochastic', False), ('nan', True), ('nan', False), 'nan delta rejects', ('inf delta', True), ('inf delta', False),
            ('fixed', True), 'fixed atoms in a swapped slot', 'skipped', ('maps', False, True), ('maps', True, True),
            ('maps', True, False), ('maps', False, False), 'a ladder with no pair of this parity',
            ('tie_temperature', True)]
    for w in want:
        assert w in seen, (w, sorted(map(str, seen)))
