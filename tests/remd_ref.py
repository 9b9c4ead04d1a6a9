"""Restatement of one nnhip_remd_exchange launch (csrc/remd.hip) for the tests (numpy), bit for bit where the kernel is exact.

For one ladder of R slots and attempt number `attempt` (parity p = attempt & 1), pair k = p, p + 2, ... < R - 1:
    a = slot_of_rank[k];  b = slot_of_rank[k + 1]
    dE = fl32(E_a - E_b);  delta = fl32(dbeta_k dE)                                  numpy float32 arithmetic: one rounding each
    u = float32(w0 >> 8) 2^-24,  w0 = Philox4x32-10(counter (attempt, stream_id, k, 0), key (seed low, seed high))[0]      exact
    accepted = delta >= 0 or u < exp(delta)                                          exp in fp64
    accepted:  the ranks of a and b are swapped in both maps;  v_a = fl32(v_a scale_up_k),  v_b = fl32(v_b scale_down_k);
               sigma of both slots = their new rows of sigma_table                   single products and copies: bitwise
Only exp is not bitwise (the kernel calls expf): a decision is reported AMBIGUOUS when delta < 0 and |u - exp(delta)| <= 4 x 2^-24
exp(delta) -- expf is good to about one ulp, u lies on the 2^-24 grid -- and the fixtures of the device tests hold no ambiguous
decision (tests/test_remd_host.py checks that), so those tests can demand every bit.

`attempt_many` is the decision over many ladders at once (the statistical test); `exchange` is one launch for one ladder, built on
it.  `synthetic_batch` is the input of the kernel test."""
import numpy as np

MAX_REPLICAS = 64
K_BOLTZMANN = 8.617333262e-5          # eV / K
AMBIGUITY = 4.0 * 2.0 ** -24
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror and Shaw 2011) on Python ints: counter (4 words), key (2 words) -> 4 words"""
    c0, c1, c2, c3 = (int(c) & _MASK for c in counter)
    k0, k1 = (int(k) & _MASK for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def philox_word0(c0, c1, c2, c3, k0, k1):
    """the first word of philox4x32_10 over numpy arrays (broadcast), as uint64 arrays holding 32-bit values"""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & np.uint64(_MASK) for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(int(k0) & _MASK), np.uint64(int(k1) & _MASK)
    m = np.uint64(_MASK)
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & m, (p0 >> s) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(_W0)) & m, (k1 + np.uint64(_W1)) & m
    return c0


def uniform(attempt, stream_id, k, seed):
    """the uniform number of pair k of ladder stream_id at attempt number `attempt`: float32 on the 2^-24 grid in [0, 1)"""
    seed = int(seed)
    w0 = philox_word0(int(attempt) & _MASK, stream_id, k, 0, seed & _MASK, (seed >> 32) & _MASK)
    return (w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def pair_delta(e_a, e_b, dbeta):
    """delta = fl32(dbeta fl32(E_a - E_b)) in numpy float32"""
    with np.errstate(invalid='ignore', over='ignore'):
        return np.asarray(dbeta, dtype=np.float32) * (np.asarray(e_a, dtype=np.float32) - np.asarray(e_b, dtype=np.float32))


def decide(delta, u):
    """(accepted, ambiguous) of delta, u float32 arrays: accept iff delta >= 0 or u < exp(delta), exp in fp64"""
    d, u = np.asarray(delta, dtype=np.float64), np.asarray(u, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        e = np.exp(d)
        accepted = (d >= 0.0) | (u < e)
        ambiguous = (d < 0.0) & (np.abs(u - e) <= AMBIGUITY * e)
    return accepted, ambiguous


def coefficients(T):
    """(dbeta, scale_up, scale_down) float32 [R] of one ladder T fp64 [R]; the last entry is unused (0, 1, 1)"""
    T = np.asarray(T, dtype=np.float64)
    dbeta, up, down = np.zeros_like(T), np.ones_like(T), np.ones_like(T)
    dbeta[:-1] = 1.0 / (K_BOLTZMANN * T[:-1]) - 1.0 / (K_BOLTZMANN * T[1:])
    up[:-1], down[:-1] = np.sqrt(T[1:] / T[:-1]), np.sqrt(T[:-1] / T[1:])
    return dbeta.astype(np.float32), up.astype(np.float32), down.astype(np.float32)


def maps_valid(rank_of_slot, slot_of_rank):
    """the two maps are inverse permutations of each other"""
    R = len(slot_of_rank)
    for k in range(R):
        s = int(slot_of_rank[k])
        if not 0 <= s < R or int(rank_of_slot[s]) != k:
            return False
    return True


def attempt_many(E, slot_of_rank, dbeta, parity, u):
    """One attempt of parity `parity` over L ladders of R slots: E float32 [L,R] per SLOT, slot_of_rank int [L,R], dbeta float32 [R]
    or [L,R], u float32 [L,R] (entry k: the uniform number of pair k).  Returns dict(slot_of_rank: the new map, delta float32
    [L,R], accepted, ambiguous, attempted bool [L,R]); entries of pairs not attempted hold 0 / False."""
    E, sor = np.asarray(E, dtype=np.float32), np.array(slot_of_rank, dtype=np.int64)
    L, R = sor.shape
    dbeta = np.broadcast_to(np.asarray(dbeta, dtype=np.float32), (L, R))
    ks = np.arange(int(parity) & 1, R - 1, 2)
    delta, accepted = np.zeros((L, R), dtype=np.float32), np.zeros((L, R), dtype=bool)
    ambiguous, attempted = np.zeros((L, R), dtype=bool), np.zeros((L, R), dtype=bool)
    attempted[:, ks] = True
    rows = np.arange(L)[:, None]
    a, b = sor[:, ks], sor[:, ks + 1]
    delta[:, ks] = pair_delta(E[rows, a], E[rows, b], dbeta[:, ks])
    accepted[:, ks], ambiguous[:, ks] = decide(delta[:, ks], np.asarray(u, dtype=np.float32)[:, ks])
    new = sor.copy()
    acc = accepted[:, ks]
    new[:, ks] = np.where(acc, b, a)
    new[:, ks + 1] = np.where(acc, a, b)
    return dict(slot_of_rank=new, delta=delta, accepted=accepted, ambiguous=ambiguous, attempted=attempted)


def exchange(E, rank_of_slot, slot_of_rank, dbeta, scale_up, scale_down, sigma_table, vel, sigma, n_attempt, n_accept, attempt,
             seed, stream_id):
    """One launch for ONE ladder.  E float32 [R] per slot; the maps int [R]; dbeta, scale_up, scale_down float32 [R]; sigma_table
    float32 [n_rows,R,n] (row k: the sigma of every atom of the ladder at rank k); vel float32 [R,n,3]; sigma float32 [R,n];
    n_attempt, n_accept int [R].  Returns the new rank_of_slot, slot_of_rank, vel, sigma, n_attempt, n_accept, the per-launch delta,
    u (float32 [R]), accepted (int32 [R]), ambiguous (bool [R]) and skipped.  A ladder whose maps are not inverse permutations of
    each other is skipped: delta = NaN, accepted = 0, u None (not written), everything else unchanged."""
    R = len(E)
    out = dict(rank_of_slot=np.array(rank_of_slot, dtype=np.int32), slot_of_rank=np.array(slot_of_rank, dtype=np.int32),
               vel=np.array(vel, dtype=np.float32), sigma=np.array(sigma, dtype=np.float32),
               n_attempt=np.array(n_attempt, dtype=np.int32), n_accept=np.array(n_accept, dtype=np.int32))
    if not maps_valid(rank_of_slot, slot_of_rank):
        out.update(delta=np.full(R, np.nan, dtype=np.float32), u=None, accepted=np.zeros(R, dtype=np.int32),
                   ambiguous=np.zeros(R, dtype=bool), skipped=True)
        return out
    ks = np.arange(R)
    u = uniform(attempt, stream_id, ks, seed)
    r = attempt_many(np.asarray(E, dtype=np.float32)[None], np.asarray(slot_of_rank)[None], dbeta, attempt & 1, u[None])
    attempted, accepted = r['attempted'][0], r['accepted'][0]
    u = np.where(attempted, u, np.float32(0.0)).astype(np.float32)
    out['n_attempt'] += attempted
    out['n_accept'] += accepted
    for k in np.nonzero(accepted)[0]:
        a, b = int(slot_of_rank[k]), int(slot_of_rank[k + 1])
        out['rank_of_slot'][a], out['rank_of_slot'][b] = k + 1, k
        out['vel'][a] = out['vel'][a] * np.float32(scale_up[k])
        out['vel'][b] = out['vel'][b] * np.float32(scale_down[k])
        out['sigma'][a], out['sigma'][b] = sigma_table[k + 1, a], sigma_table[k, b]
    out['slot_of_rank'] = r['slot_of_rank'][0].astype(np.int32)
    out.update(delta=r['delta'][0], u=u, accepted=accepted.astype(np.int32), ambiguous=r['ambiguous'][0], skipped=False)
    return out


# ---- the input of the kernel test -------------------------------------------------------------------------------------------------

SYN_REPLICAS = (2, 3, 4, 7, 8, 64)
SYN_SIZES = (1, 2, 21, 63, 64, 65, 200)
SYN_KINDS = ('accept', 'reject', 'tie_energy', 'tie_temperature', 'stochastic', 'nan', 'inf', 'fixed', 'corrupt', 'stochastic')
SYN_ATTEMPTS = (2, 0x80000003)                  # one of each parity; the second has the top bit of the uint32 set
SYN_SEED = 0x9E3779B97F4A7C15                   # the top bit of the uint64 set
SYN_ROWS = 64


def synthetic_batch(seed=0):
    """42 ladders, every (R, n) of SYN_REPLICAS x SYN_SIZES, kinds dealt in turn:
      accept           energies falling with the rank by 1 eV: delta > 0 for every pair
      reject           rising by 1000 eV: exp(delta) underflows (delta < -150 for every pair)
      tie_energy       equal energies: delta = 0;   tie_temperature: equal temperatures, unequal energies: dbeta = 0, delta = +-0
      stochastic       N(0, 0.2^2) eV: |delta| of order 1
      nan, inf         stochastic with a NaN / an infinite energy in one slot
      fixed            stochastic with a third of the atoms fixed (sigma_table 0, vel 0)
      corrupt          a rank map that is no permutation, or two permutations that are not inverses
    every other ladder with scrambled rank maps.  Returns a list of per-ladder dicts and the packed arrays of the launch."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    ladders = []
    i = 0
    for n in SYN_SIZES:
        for R in SYN_REPLICAS:
            kind = SYN_KINDS[i % len(SYN_KINDS)]
            ratio = 1.03 if R == 64 else 1.15
            T = 300.0 * ratio ** np.arange(R)
            if kind == 'tie_temperature':
                T = np.full(R, 350.0)
            sor = rng.permutation(R) if (i // 2) % 2 else np.arange(R)
            ros = np.argsort(sor)
            if kind == 'accept':
                e_rank = -1.0 * np.arange(R)
            elif kind == 'reject':
                e_rank = 1000.0 * np.arange(R)
            elif kind == 'tie_energy':
                e_rank = np.full(R, -3.25)
            else:
                e_rank = rng.normal(0.0, 0.2, R) - 40.0
            E = np.empty(R, dtype=f32)
            E[sor] = e_rank.astype(f32)
            if kind in ('nan', 'inf'):
                E[int(rng.integers(R))] = np.nan if kind == 'nan' else (np.inf if i % 4 < 2 else -np.inf)
            fixed = np.zeros(n, dtype=bool)
            if kind == 'fixed':
                fixed[::3] = True
            m = rng.choice(np.array([1.008, 12.011, 14.007, 15.999]), n)
            table = np.sqrt(0.02 * K_BOLTZMANN * T[:, None] / m[None, :])                           # [R, n]
            table = np.where(fixed[None, :], 0.0, table).astype(f32)
            sigma_table = np.full((SYN_ROWS, R, n), -1.0, dtype=f32)                                # rows >= R are never read
            sigma_table[:R] = table[:, None, :]
            vel = rng.uniform(-0.2, 0.2, (R, n, 3)).astype(f32)
            vel[:, fixed] = 0.0
            sigma = table[ros]                                                                      # [R, n]: each slot's row
            if kind == 'corrupt':
                which = (i // len(SYN_KINDS)) % 3
                if which == 0:
                    sor = sor.copy()
                    sor[0] = sor[-1]                                                                # a duplicate
                elif which == 1:
                    sor = sor.copy()
                    sor[-1] = R                                                                     # out of range
                else:
                    ros = np.roll(ros, 1)                                                           # two permutations, not inverses
            dbeta, up, down = coefficients(T)
            ladders.append(dict(kind=kind, R=R, n=n, T=T, E=E, rank_of_slot=ros.astype(np.int32), slot_of_rank=sor.astype(np.int32),
                                dbeta=dbeta, scale_up=up, scale_down=down, sigma_table=sigma_table, vel=vel, sigma=sigma.copy(),
                                fixed=fixed, n_attempt=rng.integers(0, 50, R).astype(np.int32),
                                n_accept=rng.integers(0, 50, R).astype(np.int32),
                                stream_id=int(1000 + 7 * i + (2 ** 31 if i % 5 == 0 else 0))))
            i += 1
    return ladders


def pack(ladders):
    """the packed arrays of one launch over `ladders`, in that order"""
    cat = np.concatenate
    sizes = cat([[b['n']] * b['R'] for b in ladders])
    out = dict(mol_ptr=cat([[0], np.cumsum(sizes)]).astype(np.int32),
               ladder_ptr=cat([[0], np.cumsum([b['R'] for b in ladders])]).astype(np.int32),
               stream_id=np.array([b['stream_id'] for b in ladders], dtype=np.uint32).view(np.int32),
               sigma_table=cat([b['sigma_table'].reshape(SYN_ROWS, -1) for b in ladders], axis=1),
               vel=cat([b['vel'].reshape(-1, 3) for b in ladders]), sigma=cat([b['sigma'].reshape(-1) for b in ladders]))
    for name in ('E', 'rank_of_slot', 'slot_of_rank', 'dbeta', 'scale_up', 'scale_down', 'n_attempt', 'n_accept'):
        out[name] = cat([b[name] for b in ladders])
    return out


def reference(ladders, attempt, seed=SYN_SEED):
    """exchange() of every ladder, as per-ladder results"""
    return [exchange(b['E'], b['rank_of_slot'], b['slot_of_rank'], b['dbeta'], b['scale_up'], b['scale_down'], b['sigma_table'],
                     b['vel'], b['sigma'], b['n_attempt'], b['n_accept'], attempt, seed, b['stream_id']) for b in ladders]
