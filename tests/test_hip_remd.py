"""Replica exchange on the HIP path (newtonnet_amd/remd.py, csrc/remd.hip).

Kernel alone: nnhip_remd_exchange on the synthetic batch of tests/remd_ref.py against the restatement of the launch, bit for bit
(tests/test_remd_host.py shows that no decision of that batch is ambiguous): maps, counters, per-launch outputs, velocities, sigma, and
every bit a rejected or unattempted pair owns.  Driver: every recorded step is checked ONE step at a time as in
tests/test_hip_md.py -- at an attempt step the reference exchange is applied to the RECORDED energies, ranks and velocities first, and
its delta, u and decisions must be the logged ones bit for bit."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import remd_ref as xr
from tests import util
from tests.test_hip_hessian import cuda, make_model
from tests.test_hip_md import check_stepwise

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 777.0


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _same_or_both_nan(a, b):
    """bitwise, except that a NaN matches a NaN (the sign and payload of an arithmetic NaN are the machine's own)"""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and _same(np.where(nan, np.float32(0), a), np.where(nan, np.float32(0), b))


# ---- 1. the kernel against the reference ------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def syn():
    ladders = xr.synthetic_batch()
    return ladders, {attempt: xr.reference(ladders, attempt) for attempt in xr.SYN_ATTEMPTS}


def _tensors(p):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in p.items()}
    t['mol_ptr_host'], t['ladder_ptr_host'] = torch.from_numpy(p['mol_ptr'].copy()), torch.from_numpy(p['ladder_ptr'].copy())
    B = p['E'].shape[0]
    t['delta_out'], t['u_out'] = torch.full((B,), SENT, device='cuda'), torch.full((B,), SENT, device='cuda')
    t['accepted_out'] = torch.full((B,), 777, dtype=torch.int32, device='cuda')
    return t


def _call(t, attempt, seed=xr.SYN_SEED, **replace):
    from newtonnet_amd import hip
    a = dict(t, **replace)
    hip.remd_exchange(a['E'], a['mol_ptr'], a['mol_ptr_host'], a['ladder_ptr'], a['ladder_ptr_host'], a['stream_id'], a['dbeta'],
                      a['scale_up'], a['scale_down'], a['sigma_table'], a['rank_of_slot'], a['slot_of_rank'], a['vel'], a['sigma'],
                      a['n_attempt'], a['n_accept'], attempt, seed, delta_out=a['delta_out'], u_out=a['u_out'],
                      accepted_out=a['accepted_out'])


WRITTEN = ('rank_of_slot', 'slot_of_rank', 'vel', 'sigma', 'n_attempt', 'n_accept', 'delta_out', 'u_out', 'accepted_out')
READ = ('E', 'mol_ptr', 'ladder_ptr', 'stream_id', 'dbeta', 'scale_up', 'scale_down', 'sigma_table')


def _launch(ladders, attempt):
    """one launch over `ladders`; returns per-ladder dicts of what the kernel left, and checks that the inputs are intact"""
    p = xr.pack(ladders)
    t = _tensors(p)
    _call(t, attempt)
    torch.cuda.synchronize()
    for name in READ:
        assert _same(_np(t[name]), p[name]), name
    out = []
    for g, b in enumerate(ladders):
        m0, m1 = p['ladder_ptr'][g], p['ladder_ptr'][g + 1]
        a0, a1 = p['mol_ptr'][m0], p['mol_ptr'][m1]
        r = {k: _np(t[k][m0:m1]) for k in WRITTEN if k not in ('vel', 'sigma')}
        r['vel'], r['sigma'] = _np(t['vel'][a0:a1]).reshape(b['R'], b['n'], 3), _np(t['sigma'][a0:a1]).reshape(b['R'], b['n'])
        out.append(r)
    return out


def _check_ladder(b, got, ref, what):
    R = b['R']
    for name in ('rank_of_slot', 'slot_of_rank', 'n_attempt', 'n_accept', 'vel', 'sigma'):
        assert _same(got[name], ref[name]), what + (name,)
    assert _same(got['accepted_out'], ref['accepted']), what
    assert _same_or_both_nan(got['delta_out'], ref['delta']), what + (got['delta_out'], ref['delta'])
    if ref['skipped']:
        assert np.all(got['u_out'] == np.float32(SENT)) and np.isnan(got['delta_out']).all(), what     # u_out is not written
        for name in ('rank_of_slot', 'slot_of_rank', 'n_attempt', 'n_accept', 'vel', 'sigma'):
            assert _same(got[name], b[name]), what + (name,)
        return
    assert _same(got['u_out'], ref['u']), what
    # the bits a rejected or unattempted pair owns: its slots' maps, velocities and sigma are the inputs'
    moved = np.zeros(R, dtype=bool)
    for k in np.nonzero(ref['accepted'])[0]:
        moved[b['slot_of_rank'][k]] = moved[b['slot_of_rank'][k + 1]] = True
    keep = ~moved
    assert _same(got['vel'][keep], b['vel'][keep]) and _same(got['sigma'][keep], b['sigma'][keep]), what
    assert _same(got['rank_of_slot'][keep], b['rank_of_slot'][keep]), what
    assert not got['vel'][:, b['fixed']].any() and not got['sigma'][:, b['fixed']].any(), what             # fixed atoms stay at rest


@pytest.mark.parametrize('attempt', xr.SYN_ATTEMPTS)
def test_kernel_against_the_reference_bit_for_bit(syn, attempt):
    ladders, refs = syn
    got = _launch(ladders, attempt)
    n_acc = n_rej = 0
    for g, (b, r, ref) in enumerate(zip(ladders, got, refs[attempt])):
        _check_ladder(b, r, ref, (g, b['kind'], b['R'], b['n'], attempt))
        ks = np.arange(attempt & 1, b['R'] - 1, 2)
        if not ref['skipped']:
            n_acc += int(ref['accepted'][ks].sum())
            n_rej += int(len(ks) - ref['accepted'][ks].sum())
    print(f'attempt {attempt:#x}: {len(ladders)} ladders, {n_acc} accepted and {n_rej} rejected pairs, all bits equal')
    assert n_acc > 50 and n_rej > 50


# ---- 2. independence ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('attempt', xr.SYN_ATTEMPTS)
def test_a_ladder_does_not_depend_on_the_batch_or_its_place_in_it(syn, attempt):
    ladders, _ = syn
    whole = _launch(ladders, attempt)
    backwards = _launch(ladders[::-1], attempt)[::-1]
    for g, b in enumerate(ladders):
        alone = _launch([b], attempt)[0]
        for name in WRITTEN:
            same = _same_or_both_nan if name == 'delta_out' else _same
            assert same(alone[name], whole[g][name]), ('alone', g, b['kind'], name)
            assert same(backwards[g][name], whole[g][name]), ('reversed', g, b['kind'], name)


# ---- 3. refusals and empty batches ----------------------------------------------------------------------------------------------------

def _small():
    ladders = [b for b in xr.synthetic_batch() if b['kind'] in ('stochastic', 'accept', 'fixed') and b['R'] <= 8 and b['n'] <= 21][:2]
    assert len(ladders) == 2
    return ladders


def test_refusals_write_nothing_and_an_empty_batch_succeeds():
    from newtonnet_amd import hip
    ladders = _small()
    p = xr.pack(ladders)
    t = _tensors(p)
    for name in ('n_attempt', 'n_accept'):
        t[name].fill_(777)
    before = {k: t[k].clone() for k in WRITTEN}
    B, G = p['E'].shape[0], len(ladders)

    def host(a):
        return torch.tensor(a, dtype=torch.int32)
    lp, mp = p['ladder_ptr'], p['mol_ptr']
    short = lp.copy()
    short[-1] -= 1
    late = lp.copy()
    late[0] = 1
    one = np.array([0, 1, B], dtype=np.int32)                     # a ladder of one slot
    uneven = mp.copy()
    uneven[1] += 1                                                # the first two slots of ladder 0 differ in size
    not_to_n = mp.copy()
    not_to_n[-1] -= 1
    cases = [('run from 0', dict(ladder_ptr_host=host(short))), ('run from 0', dict(ladder_ptr_host=host(late))),
             ('replicas', dict(ladder_ptr_host=host(one))), ('rows', dict(sigma_table=t['sigma_table'][:lp[1] - 1].contiguous())),
             ('atoms', dict(mol_ptr_host=host(uneven))), ('run from 0', dict(mol_ptr_host=host(not_to_n)))]
    for match, replace in cases:
        with pytest.raises(hip.HipLibraryError, match=match):
            _call(t, 0, **replace)
    # a ladder of more than NNHIP_REMD_MAX_REPLICAS slots: 65 replicas of one atom
    n65 = xr.MAX_REPLICAS + 1
    big = dict(E=torch.zeros(n65, device='cuda'), mol_ptr=torch.arange(n65 + 1, dtype=torch.int32, device='cuda'),
               mol_ptr_host=torch.arange(n65 + 1, dtype=torch.int32), ladder_ptr=torch.tensor([0, n65], dtype=torch.int32, device='cuda'),
               ladder_ptr_host=torch.tensor([0, n65], dtype=torch.int32), stream_id=torch.zeros(1, dtype=torch.int32, device='cuda'),
               dbeta=torch.zeros(n65, device='cuda'), scale_up=torch.ones(n65, device='cuda'), scale_down=torch.ones(n65, device='cuda'),
               sigma_table=torch.zeros(n65, n65, device='cuda'), rank_of_slot=torch.arange(n65, dtype=torch.int32, device='cuda'),
               slot_of_rank=torch.arange(n65, dtype=torch.int32, device='cuda'), vel=torch.full((n65, 3), SENT, device='cuda'),
               sigma=torch.full((n65,), SENT, device='cuda'), n_attempt=torch.zeros(n65, dtype=torch.int32, device='cuda'),
               n_accept=torch.zeros(n65, dtype=torch.int32, device='cuda'), delta_out=torch.full((n65,), SENT, device='cuda'),
               u_out=torch.full((n65,), SENT, device='cuda'), accepted_out=torch.full((n65,), 777, dtype=torch.int32, device='cuda'))
    with pytest.raises(hip.HipLibraryError, match='replicas'):
        _call(big, 0)
    # NULL mandatory pointers, one at a time, straight at the C entry point (the optional outputs may be NULL: not refused)
    names = ('E', 'mol_ptr', 'mol_ptr_host', 'ladder_ptr', 'ladder_ptr_host', 'stream_id', 'dbeta', 'scale_up', 'scale_down',
             'sigma_table', 'rank_of_slot', 'slot_of_rank', 'vel', 'sigma', 'n_attempt', 'n_accept', 'delta_out', 'u_out', 'accepted_out')
    N, rows = p['vel'].shape[0], p['sigma_table'].shape[0]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for missing in names[:16]:
        args = [None if n == missing else C.c_void_p(t[n].data_ptr()) for n in names]
        rc = hip.lib().nnhip_remd_exchange(*args, 0, 0, G, B, N, rows, stream)
        assert rc != 0 and b'null' in hip.lib().nnhip_last_error(), missing
    for bad_counts in ((-1, B, N, rows), (G, -1, N, rows), (G, B, -1, rows), (G, B, N, -1)):
        args = [C.c_void_p(t[n].data_ptr()) for n in names]
        assert hip.lib().nnhip_remd_exchange(*args, 0, 0, *bad_counts, stream) != 0
    torch.cuda.synchronize()
    for k in WRITTEN:
        assert torch.equal(t[k], before[k]), k                                   # nothing was written
    assert torch.all(big['vel'] == SENT) and torch.all(big['delta_out'] == SENT) and torch.all(big['accepted_out'] == 777)
    # the wrapper refuses what would be written into a copy
    with pytest.raises(ValueError, match='vel'):
        _call(t, 0, vel=t['vel'].double())
    with pytest.raises(ValueError, match='attempt'):
        _call(t, 2 ** 32)
    with pytest.raises(ValueError, match='seed'):
        _call(t, 0, seed=-1)
    # an empty batch: success, nothing to write
    e32, ef = torch.zeros(0, dtype=torch.int32, device='cuda'), torch.zeros(0, device='cuda')
    zero = torch.zeros(1, dtype=torch.int32)
    hip.remd_exchange(ef, zero.cuda(), zero, zero.cuda(), zero.clone(), e32, ef, ef, ef, torch.zeros(4, 0, device='cuda'), e32.clone(),
                      e32.clone(), torch.zeros(0, 3, device='cuda'), ef.clone(), e32.clone(), e32.clone(), 0, 0)
    # replicas without atoms: decisions are made, no atom is walked
    hollow = [dict(b, n=0, vel=b['vel'][:, :0], sigma=b['sigma'][:, :0], sigma_table=b['sigma_table'][:, :, :0], fixed=b['fixed'][:0])
              for b in ladders]
    got = _launch(hollow, 0)
    for b, r, ref in zip(hollow, got, xr.reference(hollow, 0)):
        _check_ladder(b, r, ref, ('hollow', b['R']))
    # the valid call still works after all the refusals, and without the optional outputs
    _call(t, 0, delta_out=None, u_out=None, accepted_out=None)
    torch.cuda.synchronize()
    ref = xr.reference(ladders, 0)
    assert _same(_np(t['slot_of_rank']), np.concatenate([r['slot_of_rank'] for r in ref]))
    assert torch.all(t['delta_out'] == SENT) and torch.all(t['u_out'] == SENT)


# ---- 4. the driver, one step at a time ----------------------------------------------------------------------------------------------

TEMPERATURES = [300.0, 400.0, 500.0, 600.0]
FRICTION = 0.02
SEED, EXCHANGE_SEED = 7, 3


def _aspirins(g=2):
    return _bench().synthetic_aspirin(g, 0, 'cuda')


def _replicate(z, pos, cell, batch, G, R):
    """systems of one size, replicated ladder-major by reshaping: independent of the driver's own index arithmetic"""
    n = z.numel() // G
    return (z.view(G, n).repeat_interleave(R, 0).reshape(-1), pos.view(G, n, 3).repeat_interleave(R, 0).reshape(-1, 3),
            cell.repeat_interleave(R, 0), torch.arange(G * R, device=z.device).repeat_interleave(n))


def test_every_recorded_step_follows_from_the_one_before_through_the_exchanges():
    from newtonnet_amd.dynamics import langevin_coefficients
    G, R, n_steps, every = 2, len(TEMPERATURES), 40, 5
    z, pos, cell, batch = _aspirins(G)
    model = make_model(util.load_state('rand'))
    gen = torch.Generator(device='cuda').manual_seed(SEED)
    rex = model.replica_exchange(z, pos, cell, batch, TEMPERATURES, every, FRICTION, generator=gen, exchange_seed=EXCHANGE_SEED)
    zr, pr, cr, br = _replicate(z, pos, cell, batch, G, R)
    assert torch.equal(rex.z, zr) and torch.equal(rex.positions, pr) and torch.equal(rex.cell, cr) and torch.equal(rex.batch, br)
    B, n = G * R, 21
    N = B * n
    p0, v0 = rex.positions, rex.velocities
    before = model.deferred_stats()
    traj = rex.run(n_steps, record_every=1)
    after = model.deferred_stats()
    assert after['repeats_needed'] == before['repeats_needed']
    assert traj.step.tolist() == list(range(1, n_steps + 1)) and traj.exchange_step.tolist() == list(range(every, n_steps + 1, every))
    regen = torch.Generator(device='cuda').manual_seed(SEED)
    torch.randn((N, 3), generator=regen, device='cuda')                              # the Maxwell-Boltzmann draw
    noises = [torch.randn((N, 3), generator=regen, device='cuda') for _ in range(n_steps)]
    T = np.tile(np.array(TEMPERATURES), (G, 1))
    coef = [xr.coefficients(T[g]) for g in range(G)]
    table = _np(rex._sigma_table).reshape(R, G, R, n)
    rank = np.concatenate([np.tile(np.arange(R, dtype=np.int32), G)[None], _np(traj.rank)])       # rank[s]: under which step s was run
    pos_f, vel_f = [p0] + list(traj.pos), [v0] + list(traj.vel)
    energy = _np(traj.potential_energy)
    assert np.array_equal(rank[1], rank[0])
    cur_rank = rank[0].reshape(G, R).copy()
    start_vel, s0 = v0, 0
    n_acc = n_rej = 0
    log_delta, log_u, log_acc = _np(traj.delta), _np(traj.u), _np(traj.accepted)

    def check_segment(s0, s1, start_vel, cur_rank):
        T_slot = torch.tensor(np.take_along_axis(T, cur_rank.astype(np.int64), 1).reshape(-1), dtype=torch.float64, device='cuda')
        sigma = langevin_coefficients(0.5, FRICTION, T_slot, rex.masses, rex.batch)[1]
        rows = np.stack([table[cur_rank[g, s], g, s] for g in range(G) for s in range(R)]).reshape(-1)
        assert _same(_np(sigma), rows), 'a sigma row is not what langevin_coefficients gives at that temperature'
        shim = types.SimpleNamespace(_hk=rex._hk, masses=rex.masses, _sigma=sigma, _c1=rex._c1, _dth=rex._dth)
        check_stepwise(model, shim, zr, cr, br, pos_f[s0:s1 + 1], [start_vel] + vel_f[s0 + 1:s1 + 1], noises[s0:s1],
                       f'remd steps {s0}..{s1}')

    for i, s in enumerate(range(every, n_steps + 1, every)):
        check_segment(s0, s, start_vel, cur_rank)
        # ranks change at attempt steps only: the frames s0 + 1 .. s were all integrated under cur_rank
        for j in range(s0 + 1, s + 1):
            assert np.array_equal(rank[j].reshape(G, R), cur_rank), j
        # the exchange at step s, restated on what was RECORDED at step s
        vel_s = _np(vel_f[s]).reshape(G, R, n, 3).copy()
        for g in range(G):
            ros = cur_rank[g]
            ref = xr.exchange(energy[s - 1, g * R:(g + 1) * R], ros, np.argsort(ros), *coef[g], table[:, g], vel_s[g],
                              table[ros, g, np.arange(R)], np.zeros(R, np.int32), np.zeros(R, np.int32), i, EXCHANGE_SEED, g)
            assert not ref['ambiguous'].any(), 'an ambiguous decision: change EXCHANGE_SEED, never the band'
            assert _same(log_delta[i, g], ref['delta'][:-1]) and _same(log_u[i, g], ref['u'][:-1]), (i, g, log_delta[i, g], ref['delta'])
            assert np.array_equal(log_acc[i, g], ref['accepted'][:-1].astype(bool)), (i, g)
            ks = np.arange(i & 1, R - 1, 2)
            n_acc += int(ref['accepted'][ks].sum())
            n_rej += int(len(ks) - ref['accepted'][ks].sum())
            cur_rank[g] = ref['rank_of_slot']
            vel_s[g] = ref['vel']
            assert sorted(cur_rank[g].tolist()) == list(range(R))
        start_vel, s0 = torch.from_numpy(vel_s.reshape(N, 3)).cuda(), s
    print(f'remd driver: {len(traj.exchange_step)} attempts, {n_acc} accepted and {n_rej} rejected pairs; delta\n{log_delta}\nfinal ranks '
          f'{cur_rank.tolist()}')
    # the state the run left behind is the reference's: maps, velocities, sigma; the counters are the sums of the log
    assert np.array_equal(_np(rex.rank_of_slot), cur_rank) and np.array_equal(_np(rex.slot_of_rank), np.argsort(cur_rank, 1))
    assert _same(_np(rex.velocities), _np(start_vel))
    assert _same(_np(rex._sigma), np.stack([table[cur_rank[g, s], g, s] for g in range(G) for s in range(R)]).reshape(-1))
    attempted = np.array([[k % 2 == i % 2 for k in range(R - 1)] for i in range(len(log_acc))])
    assert np.array_equal(_np(rex.n_attempt), np.tile(attempted.sum(0), (G, 1))) and np.array_equal(_np(rex.n_accept), log_acc.sum(0))
    assert not log_acc[~np.broadcast_to(attempted[:, None, :], log_acc.shape)].any()
    np.testing.assert_array_equal(_np(rex.acceptance), log_acc.sum(0).astype(np.float32) / np.tile(attempted.sum(0), (G, 1)).astype(np.float32))
    assert n_acc >= 1 and n_rej >= 1, 'the set-up shows nothing without an accepted and a rejected exchange'
    # by_temperature is the slot arrays gathered by rank
    by_t = traj.by_temperature()
    f = n_steps - 1
    slot = np.argsort(rank[n_steps].reshape(G, R), 1)
    assert np.array_equal(_np(by_t['slot'][f]), slot)
    for g in range(G):
        for k in range(R):
            assert torch.equal(by_t['pos'][f, g, k], traj.pos[f].view(G, R, n, 3)[g, slot[g, k]])
            assert torch.equal(by_t['vel'][f, g, k], traj.vel[f].view(G, R, n, 3)[g, slot[g, k]])
            assert by_t['potential_energy'][f, g, k] == traj.potential_energy[f].view(G, R)[g, slot[g, k]]
    want_T = np.take_along_axis(T, rank[n_steps].reshape(G, R).astype(np.int64), 1).reshape(-1)
    assert np.array_equal(_np(traj.temperature_of_slot[f]), want_T)


# ---- 5. bitwise properties --------------------------------------------------------------------------------------------------------

NAMES = ('pos', 'vel', 'potential_energy', 'kinetic_energy', 'step', 'rank')
LOG = ('exchange_step', 'delta', 'u', 'accepted')


def test_bitwise_properties():
    z, pos, cell, batch, _ = util.case_inputs('mixed_rand', torch.float32)
    two = batch < 2                                                    # two systems, of whatever sizes the case gives them
    z, pos, cell, batch = cuda(z[two], pos[two], cell[:2], batch[two])
    keep = [t.clone() for t in (z, pos, cell, batch)]
    model = make_model(util.load_state('rand'))
    G, R = 2, 4
    ladders = torch.tensor([TEMPERATURES, [250.0, 250.0, 330.0, 420.0]], dtype=torch.float64)

    def make(every, seed=SEED, xseed=EXCHANGE_SEED):
        gen = torch.Generator(device='cuda').manual_seed(seed)
        return model.replica_exchange(z, pos, cell, batch, ladders, every, FRICTION, generator=gen, exchange_seed=xseed)
    # exchange_every = 0 is model.dynamics on the replicated batch with the same ladder
    never = make(0)
    counts = torch.bincount(batch, minlength=G).tolist()
    parts = [t for g in range(G) for t in [(batch == g).nonzero().flatten()] * R]
    src = torch.cat(parts)
    rep_batch = torch.cat([torch.full((counts[m // R],), m, device='cuda') for m in range(G * R)])
    assert torch.equal(never.z, z[src]) and torch.equal(never.positions, pos[src]) and torch.equal(never.batch, rep_batch)
    t0 = never.run(20, 1)
    gen = torch.Generator(device='cuda').manual_seed(SEED)
    plain = model.dynamics(z[src], pos[src], cell.repeat_interleave(R, 0), rep_batch, temperature=ladders.reshape(-1).cuda(),
                           friction=FRICTION, generator=gen).run(20, 1)
    for name in NAMES[:5]:
        assert torch.equal(getattr(t0, name), getattr(plain, name)), name
    assert t0.exchange_step.numel() == 0 and t0.delta.shape == (0, G, R - 1) and torch.equal(t0.rank, t0.rank[:1].expand(20, -1))
    assert torch.isnan(never.acceptance).all()
    # the same seeds twice; another exchange seed changes u but not the first segment
    a, b, c = make(5).run(20, 1), make(5).run(20, 1), make(5, xseed=EXCHANGE_SEED + 1).run(20, 1)
    for name in NAMES + LOG:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.exchange_step.tolist() == [5, 10, 15, 20] and not torch.equal(a.u, c.u)
    for name in NAMES:
        assert torch.equal(getattr(a, name)[:5], getattr(c, name)[:5]), name
        assert torch.equal(getattr(a, name)[:5], getattr(t0, name)[:5]), name          # ... which is the run without exchanges
    assert torch.equal(a.delta[0], c.delta[0])
    print(f'mixed sizes {counts}: accepted per attempt {a.accepted.sum((1, 2)).tolist()} of {a.accepted.shape[1:]}')
    # run(11, 4); run(9, 0) equals run(20, ...): state, counters and the log's continuation (attempt numbers run on)
    d = make(5)
    first = d.run(11, 4)
    last = d.run(9, 0)
    assert first.step.tolist() == [4, 8, 11] and first.exchange_step.tolist() == [5, 10] and last.exchange_step.tolist() == [15, 20]
    for name in NAMES:
        assert torch.equal(getattr(last, name)[0], getattr(a, name)[-1]), name
        assert torch.equal(getattr(first, name), getattr(a, name)[[3, 7, 10]]), name
    for name in LOG[1:]:
        assert torch.equal(torch.cat([getattr(first, name), getattr(last, name)]), getattr(a, name)), name
    whole = make(5)
    whole.run(20, 0)
    for name in ('positions', 'velocities', 'potential_energy', 'kinetic_energy', 'forces', 'rank_of_slot', 'slot_of_rank', 'n_attempt',
                 'n_accept', '_sigma'):
        assert torch.equal(getattr(d, name), getattr(whole, name)), name
    assert d.step_count == whole.step_count == 20 and d.attempt_count == whole.attempt_count == 4
    # record_every 1 and 5 agree at the common steps
    e5 = make(5).run(20, 5)
    assert e5.step.tolist() == [5, 10, 15, 20]
    for name in NAMES:
        assert torch.equal(getattr(e5, name), getattr(a, name)[4::5]), name
    for name in LOG:
        assert torch.equal(getattr(e5, name), getattr(a, name)), name
    # systems of different sizes: by_temperature gathers the energies and leaves the ragged arrays out
    by_t = a.by_temperature()
    assert by_t['potential_energy'].shape == (20, G, R) and (('pos' in by_t) == (counts[0] == counts[1]))
    assert torch.equal(by_t['potential_energy'], torch.gather(a.potential_energy.view(20, G, R), 2, by_t['slot']))
    assert torch.equal(torch.gather(a.rank.view(20, G, R).long(), 2, by_t['slot']), torch.arange(R, device='cuda').expand(20, G, R))
    # the caller's tensors are never modified
    for t, k in zip((z, pos, cell, batch), keep):
        assert torch.equal(t, k)


# ---- 6. interfaces ----------------------------------------------------------------------------------------------------------------

class FakeAtoms:
    """The accessors format_data() and run_remd() use (as in tests/test_ase_calculator.py)"""
    def __init__(self, numbers, positions):
        self.numbers, self.positions = np.asarray(numbers), np.asarray(positions, dtype=np.float64)

    def __len__(self):
        return len(self.numbers)

    def get_atomic_numbers(self):
        return self.numbers

    def get_positions(self, wrap=False):
        return self.positions

    def get_cell(self):
        return np.zeros((3, 3))

    def get_pbc(self):
        return np.zeros(3, dtype=bool)


def test_interfaces_shapes_seed_and_single_structure():
    from newtonnet_amd.remd import ReplicaExchange, ReplicaTrajectory
    from newtonnet_amd.utils import MLAseCalculator
    z, pos, _, _ = _bench().synthetic_aspirin(2, 1, 'cpu')
    model = make_model(util.load_state('rand'))
    calc = MLAseCalculator(model, properties=['energy', 'forces'], device='cuda')
    frames = [FakeAtoms(z[:21].numpy(), pos[21 * k:21 * (k + 1)].numpy()) for k in range(2)]
    keep = [f.positions.copy() for f in frames]
    T = [300.0, 380.0, 470.0]
    kw = dict(friction=FRICTION, record_every=4, seed=5, exchange_seed=9)
    out = calc.run_remd(frames, T, 10, 2, **kw)
    G, R, Rec, A = 2, 3, 3, 5
    assert out['step'].tolist() == [4, 8, 10] and out['step'].dtype == np.int64 and out['exchange_step'].tolist() == [2, 4, 6, 8, 10]
    for k in ('positions', 'velocities', 'positions_by_temperature', 'velocities_by_temperature'):
        assert out[k].shape == (Rec, G, R, 21, 3) and out[k].dtype == np.float32, k
    for k in ('energy', 'kinetic_energy', 'energy_by_temperature', 'kinetic_energy_by_temperature'):
        assert out[k].shape == (Rec, G, R) and out[k].dtype == np.float32, k
    assert out['rank'].shape == (Rec, G, R) and out['rank'].dtype == np.int32 and out['temperature'].shape == (Rec, G, R)
    assert out['delta'].shape == out['u'].shape == out['accepted'].shape == (A, G, R - 1)
    assert out['delta'].dtype == out['u'].dtype == np.float32 and out['accepted'].dtype == np.bool_
    assert out['acceptance'].shape == (G, R - 1)
    # the by-temperature arrays are the slot arrays gathered by rank
    assert np.array_equal(np.sort(out['rank'], axis=2), np.broadcast_to(np.arange(R), (Rec, G, R)))
    assert np.array_equal(out['temperature'], np.array(T)[out['rank']])
    for f in range(Rec):
        for g in range(G):
            for s in range(R):
                k = out['rank'][f, g, s]
                assert np.array_equal(out['positions_by_temperature'][f, g, k], out['positions'][f, g, s])
                assert np.array_equal(out['velocities_by_temperature'][f, g, k], out['velocities'][f, g, s])
                assert out['energy_by_temperature'][f, g, k] == out['energy'][f, g, s]
                assert out['kinetic_energy_by_temperature'][f, g, k] == out['kinetic_energy'][f, g, s]
    again = calc.run_remd(frames, T, 10, 2, **kw)
    other = calc.run_remd(frames, T, 10, 2, **dict(kw, seed=6))
    assert all(np.array_equal(out[k], again[k], equal_nan=True) for k in out) and not np.array_equal(out['positions'], other['positions'])
    assert all(np.array_equal(f.positions, k) for f, k in zip(frames, keep))
    one = calc.run_remd(frames[0], T, 4, 2, friction=FRICTION, seed=5)                  # a single structure drops the G axis
    assert one['positions'].shape == one['positions_by_temperature'].shape == (1, R, 21, 3) and one['energy'].shape == (1, R)
    assert one['rank'].shape == (1, R) and one['delta'].shape == (2, R - 1) and one['acceptance'].shape == (R - 1,)
    assert one['step'].tolist() == [4] and one['exchange_step'].tolist() == [2, 4]
    # model.replica_exchange: a ReplicaExchange (a Dynamics) whose run returns a ReplicaTrajectory of device tensors
    zc, pc = z.cuda(), pos.cuda()
    cell, batch = torch.zeros(2, 3, 3, device='cuda'), torch.repeat_interleave(torch.arange(2), 21).cuda()
    rex = model.replica_exchange(zc, pc, cell, batch, T, 3, FRICTION)
    traj = rex.run(6, 3)
    assert isinstance(rex, ReplicaExchange) and isinstance(traj, ReplicaTrajectory) and traj.step.tolist() == [3, 6]
    assert traj.rank.shape == (2, 6) and traj.rank.dtype == torch.int32 and traj.rank.is_cuda
    assert traj.temperature_of_slot.shape == (2, 6) and traj.pos.shape == (2, 126, 3) and traj.temperature.shape == (2, 6)
    assert rex.acceptance.shape == (2, 2) and rex.n_attempt.tolist() == [[1, 1], [1, 1]] and rex.step_count == 6
    assert rex.run(0).step.tolist() == [6]
    for bad in (dict(n_steps=-1), dict(n_steps=2.5), dict(n_steps=3, record_every=-1)):
        with pytest.raises(ValueError):
            rex.run(**bad)
    # fixed atoms stay where they are through exchanges, bit for bit
    fixed = torch.zeros(42, dtype=torch.bool, device='cuda')
    fixed[::2] = True
    held = model.replica_exchange(zc, pc, cell, batch, [300.0, 300.0, 300.0], 1, FRICTION, fixed=fixed)
    th = held.run(6, 0)
    rep_fixed = fixed.view(2, 21).repeat_interleave(3, 0).reshape(-1)
    assert torch.equal(th.pos[0][rep_fixed], pc.view(2, 21, 3).repeat_interleave(3, 0).reshape(-1, 3)[rep_fixed])
    assert not th.vel[0][rep_fixed].any() and held.n_accept.sum() == held.n_attempt.sum() == 12         # equal temperatures: every swap
