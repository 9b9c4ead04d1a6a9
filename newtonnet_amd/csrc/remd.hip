// Replica exchange on the device (gfx950, fp32): one launch per attempt decides every neighbouring pair of one parity in every
// temperature ladder of a batch and, where a pair is accepted, swaps the two temperatures in place.  A ladder is a run of
// consecutive molecules (its slots), all replicas of one system; each slot holds a rank, its index into the ladder's temperature
// list, and an exchange swaps the RANKS of two slots: positions and forces stay where they are, the velocities of the two slots are
// rescaled to their new temperatures and the slots' Langevin sigma rows are copied from a table.  A step of the driver
// (newtonnet_amd/remd.py) at an attempt is  model(pos) -> md_step(finish) -> remd_exchange -> md_step(begin).
// include/newtonnet_hip.h spells the contract out.
//
// One workgroup of four waves per ladder, the ladders of a batch by a grid-stride loop.  Every thread checks the ladder's layout and
// rank maps for itself (at most 64 slots: the same answer in every thread, no communication).  Thread k decides pair (k, k + 1) and
// posts the new rank and the velocity scale of both of its slots in LDS (a slot in no attempted pair is posted "unchanged" by the
// thread of its rank: every LDS word is written by exactly one thread).  ONE barrier, reached by every thread -- a skipped ladder skips
// the work, never the barrier -- then all 256 threads walk the ladder's atoms and thread k writes the two maps of an accepted pair
// (after the barrier: before it every thread may still be reading them).  A second barrier closes the loop body, for the LDS words
// of the next ladder.  No float atomics, no communication between workgroups: the outputs of a ladder depend neither on the rest of
// the batch nor on its place in it (its random numbers are keyed by stream_id[g], not by g).
//
// The chain, every float operation one explicit rounding (tests/remd_ref.py restates it bitwise):
//   pair k (k = p, p + 2, ... < R - 1 with p = attempt & 1):   a = slot_of_rank[k];  b = slot_of_rank[k + 1]
//     dE = __fsub_rn(E_a, E_b);   delta = __fmul_rn(dbeta_k, dE)
//     (w0, w1, w2, w3) = Philox4x32-10(counter (attempt, stream_id[g], k, 0), key (seed_lo, seed_hi));   u = float(w0 >> 8) * 2^-24
//     accept iff  delta >= 0  ||  u < expf(delta)            (NaN delta: rejected; delta == 0: accepted)
//   accepted:  rank_of_slot[a] = k + 1, rank_of_slot[b] = k, slot_of_rank[k] = b, slot_of_rank[k + 1] = a
//              v_a = __fmul_rn(v_a, scale_up_k),  v_b = __fmul_rn(v_b, scale_down_k)     (every component of every atom of the slot)
//              sigma[i] = sigma_table[new rank][i]                                        (a copy)
#include "common.h"

namespace {

constexpr int REMD_THREADS = 256;
constexpr int REMD_MAX_BLOCKS = 2048;

struct RemdArgs {
  const float* energy;
  const int32_t* mol_ptr;
  const int32_t* ladder_ptr;
  const int32_t* stream_id;
  const float* dbeta;
  const float* scale_up;
  const float* scale_down;
  const float* sigma_table;
  int32_t* rank_of_slot;
  int32_t* slot_of_rank;
  float* vel;
  float* sigma;
  int32_t* n_attempt;
  int32_t* n_accept;
  float* delta_out;
  float* u_out;
  int32_t* accepted_out;
  uint32_t attempt, seed_lo, seed_hi;
  int n_ladders, n_mol, n_atoms, n_rows;
};

// Philox4x32-10 (Salmon, Moraes, Dror and Shaw 2011), the first word of the block
__device__ __forceinline__ uint32_t philox4x32_10_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

__global__ void __launch_bounds__(REMD_THREADS)
remd_exchange_kernel(RemdArgs g) {
  __shared__ int s_rank[NNHIP_REMD_MAX_REPLICAS];        // per slot: its new rank, -1 = the slot keeps every bit
  __shared__ float s_scale[NNHIP_REMD_MAX_REPLICAS];
  const int t = threadIdx.x;
  const uint32_t parity = g.attempt & 1u;
  for (int l = blockIdx.x; l < g.n_ladders; l += gridDim.x) {       // (uniform over the workgroup)
    const int m0 = g.ladder_ptr[l], m1 = g.ladder_ptr[l + 1];
    const int R = m1 - m0;
    // ---- the ladder as every thread sees it.  Pointers that leave the arrays: nothing of it is touched.  Replicas of unequal size or
    // rank maps that are not inverse permutations of each other: delta_out = NaN, accepted_out = 0, nothing else is written
    const bool inside = m0 >= 0 && m1 <= g.n_mol && R >= 2 && R <= NNHIP_REMD_MAX_REPLICAS && R <= g.n_rows;
    bool bad = !inside;
    int base = 0, n = 0;
    if (inside) {
      base = g.mol_ptr[m0];
      n = g.mol_ptr[m0 + 1] - base;
      bad = base < 0 || n < 0;
      for (int s = 0; s < R; ++s) {
        const int a0 = g.mol_ptr[m0 + s], a1 = g.mol_ptr[m0 + s + 1];
        bad = bad || a1 - a0 != n || a1 > g.n_atoms;
      }
      for (int k = 0; k < R; ++k) {
        const int s = g.slot_of_rank[m0 + k];
        const bool in_range = s >= 0 && s < R;
        bad = bad || !in_range || g.rank_of_slot[m0 + (in_range ? s : 0)] != k;
      }
    }
    // ---- the decisions: thread k owns pair (k, k + 1) and entry k of every per-pair array
    bool accepted = false;
    int a = 0, b = 0;
    if (inside && t < R) {
      const int k = t;
      const bool lower = (uint32_t)(k & 1) == parity && k < R - 1;           // rank k is the lower half of an attempted pair
      const bool upper = k >= 1 && (uint32_t)((k - 1) & 1) == parity;        // ... the upper half of one
      float delta = 0.f, u = 0.f;
      if (bad) {
        delta = __builtin_nanf("");
      } else if (lower) {
        a = g.slot_of_rank[m0 + k];
        b = g.slot_of_rank[m0 + k + 1];
        const float dE = __fsub_rn(g.energy[m0 + a], g.energy[m0 + b]);
        delta = __fmul_rn(g.dbeta[m0 + k], dE);
        const uint32_t w0 = philox4x32_10_word0(g.attempt, (uint32_t)g.stream_id[l], (uint32_t)k, 0u, g.seed_lo, g.seed_hi);
        u = __fmul_rn((float)(w0 >> 8), 5.9604644775390625e-8f);             // 24 bits times 2^-24: exact, in [0, 1)
        accepted = delta >= 0.f || u < expf(delta);
        s_rank[a] = accepted ? k + 1 : -1;
        s_rank[b] = accepted ? k : -1;
        s_scale[a] = g.scale_up[m0 + k];
        s_scale[b] = g.scale_down[m0 + k];
        g.n_attempt[m0 + k] += 1;
        if (accepted) g.n_accept[m0 + k] += 1;
      } else if (!upper) {
        s_rank[g.slot_of_rank[m0 + k]] = -1;
      }
      if (g.delta_out) g.delta_out[m0 + k] = delta;
      if (g.u_out && !bad) g.u_out[m0 + k] = u;
      if (g.accepted_out) g.accepted_out[m0 + k] = accepted ? 1 : 0;
    }
    __syncthreads();
    if (!bad) {
      // ---- the atoms of the ladder: slot s owns base + s n .. base + (s + 1) n - 1
      const long total = (long)R * n;
      for (long j = t; j < total; j += REMD_THREADS) {
        const int s = (int)(j / n);
        const int rank = s_rank[s];
        if (rank < 0) continue;
        const size_t i = (size_t)base + (size_t)j;
        const float c = s_scale[s];
        g.vel[3 * i] = __fmul_rn(g.vel[3 * i], c);
        g.vel[3 * i + 1] = __fmul_rn(g.vel[3 * i + 1], c);
        g.vel[3 * i + 2] = __fmul_rn(g.vel[3 * i + 2], c);
        g.sigma[i] = g.sigma_table[(size_t)rank * (size_t)g.n_atoms + i];
      }
      if (accepted) {
        g.rank_of_slot[m0 + a] = t + 1;
        g.rank_of_slot[m0 + b] = t;
        g.slot_of_rank[m0 + t] = b;
        g.slot_of_rank[m0 + t + 1] = a;
      }
    }
    __syncthreads();                                       // s_rank / s_scale belong to the next ladder from here
  }
}

}  // namespace

extern "C" int nnhip_remd_exchange(const float* energy, const int32_t* mol_ptr, const int32_t* mol_ptr_host, const int32_t* ladder_ptr,
                                   const int32_t* ladder_ptr_host, const int32_t* stream_id, const float* dbeta,
                                   const float* scale_up, const float* scale_down, const float* sigma_table, int32_t* rank_of_slot,
                                   int32_t* slot_of_rank, float* vel, float* sigma, int32_t* n_attempt, int32_t* n_accept,
                                   float* delta_out, float* u_out, int32_t* accepted_out, int32_t attempt, int64_t seed,
                                   int32_t n_ladders, int32_t n_mol, int32_t n_atoms, int32_t n_rows, void* stream) {
  if (n_ladders < 0 || n_mol < 0 || n_atoms < 0 || n_rows < 0) {
    nnhip_set_error("nnhip_remd_exchange: bad arguments (n_ladders %d, n_mol %d, n_atoms %d, n_rows %d)", n_ladders, n_mol, n_atoms,
                    n_rows);
    return NNHIP_E_INVALID;
  }
  if (n_ladders == 0 && n_mol == 0) return NNHIP_OK;
  if (!energy || !mol_ptr || !mol_ptr_host || !ladder_ptr || !ladder_ptr_host || !stream_id || !dbeta || !scale_up || !scale_down ||
      !rank_of_slot || !slot_of_rank || !n_attempt || !n_accept) {
    nnhip_set_error("nnhip_remd_exchange: null pointer (energy, mol_ptr, mol_ptr_host, ladder_ptr, ladder_ptr_host, stream_id, dbeta, "
                    "scale_up, scale_down, rank_of_slot, slot_of_rank, n_attempt and n_accept are mandatory)");
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && (!sigma_table || !vel || !sigma)) {
    nnhip_set_error("nnhip_remd_exchange: null pointer (sigma_table, vel and sigma are mandatory)");
    return NNHIP_E_INVALID;
  }
  if (ladder_ptr_host[0] != 0 || ladder_ptr_host[n_ladders] != n_mol) {
    nnhip_set_error("nnhip_remd_exchange: ladder_ptr must run from 0 to n_mol = %d (got %d .. %d)", n_mol, ladder_ptr_host[0],
                    ladder_ptr_host[n_ladders]);
    return NNHIP_E_INVALID;
  }
  if (mol_ptr_host[0] != 0 || mol_ptr_host[n_mol] != n_atoms) {
    nnhip_set_error("nnhip_remd_exchange: mol_ptr must run from 0 to n_atoms = %d (got %d .. %d)", n_atoms, mol_ptr_host[0],
                    mol_ptr_host[n_mol]);
    return NNHIP_E_INVALID;
  }
  for (int l = 0; l < n_ladders; ++l) {
    const int m0 = ladder_ptr_host[l];
    const long R = (long)ladder_ptr_host[l + 1] - m0;
    if (R < 2 || R > NNHIP_REMD_MAX_REPLICAS) {
      nnhip_set_error("nnhip_remd_exchange: ladder %d has %ld replicas (2 .. %d expected)", l, R, NNHIP_REMD_MAX_REPLICAS);
      return NNHIP_E_INVALID;
    }
    if (m0 < 0 || m0 + R > n_mol) {
      nnhip_set_error("nnhip_remd_exchange: ladder %d leaves the batch (molecules %d .. %ld of %d)", l, m0, m0 + R - 1, n_mol);
      return NNHIP_E_INVALID;
    }
    if (R > n_rows) {
      nnhip_set_error("nnhip_remd_exchange: ladder %d has %ld replicas, sigma_table only %d rows", l, R, n_rows);
      return NNHIP_E_INVALID;
    }
    const long n = (long)mol_ptr_host[m0 + 1] - mol_ptr_host[m0];
    for (int s = 0; s < R; ++s) {
      const long ns = (long)mol_ptr_host[m0 + s + 1] - mol_ptr_host[m0 + s];
      if (ns != n || ns < 0) {
        nnhip_set_error("nnhip_remd_exchange: ladder %d: replica %d has %ld atoms, replica 0 has %ld (equal counts >= 0 expected)", l, s,
                        ns, n);
        return NNHIP_E_INVALID;
      }
    }
  }
  RemdArgs g;
  g.energy = energy;
  g.mol_ptr = mol_ptr;
  g.ladder_ptr = ladder_ptr;
  g.stream_id = stream_id;
  g.dbeta = dbeta;
  g.scale_up = scale_up;
  g.scale_down = scale_down;
  g.sigma_table = sigma_table;
  g.rank_of_slot = rank_of_slot;
  g.slot_of_rank = slot_of_rank;
  g.vel = vel;
  g.sigma = sigma;
  g.n_attempt = n_attempt;
  g.n_accept = n_accept;
  g.delta_out = delta_out;
  g.u_out = u_out;
  g.accepted_out = accepted_out;
  g.attempt = (uint32_t)attempt;
  g.seed_lo = (uint32_t)((uint64_t)seed & 0xFFFFFFFFu);
  g.seed_hi = (uint32_t)((uint64_t)seed >> 32);
  g.n_ladders = n_ladders;
  g.n_mol = n_mol;
  g.n_atoms = n_atoms;
  g.n_rows = n_rows;
  const int blocks = n_ladders > REMD_MAX_BLOCKS ? REMD_MAX_BLOCKS : n_ladders;
  remd_exchange_kernel<<<blocks, REMD_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
