// The per-molecule L-BFGS step of the optimiser kernels (gfx950, fp32): the one definition that lbfgs_step_kernel (relax.hip, for
// nnhip_lbfgs_step: minima, on the model's forces) and dimer_step_kernel (dimer.hip, for nnhip_dimer_step: the translation of a
// dimer, on the forces with their component along the lowest mode inverted) share, so that "nnhip_lbfgs_step's recursion" is a
// property of the text and not of two texts that agree.
//
// The chain is written once, over a TEAM of threads that works on one molecule [a0, a1) -- WaveTeam: one wave64 (relax.hip,
// cellrelax.hip, dimer.hip); BlockTeam: one workgroup of NNHIP_LBFGS_WG_THREADS threads (the *_wg kernels of relax.hip and
// cellrelax.hip), described where it is defined.  With WaveTeam: lane l owns the atoms l, l + 64, ... in EVERY sweep, so a lane
// only ever re-reads what it wrote itself: no barrier, no LDS.  Every per-molecule reduction is a lane-local sum (or max) in atom order, then the fixed
// butterfly __shfl_xor 32, 16, ..., 1 -- a + b and b + a round alike, so all 64 lanes hold the same bits afterwards and every
// decision is uniform over the wave.  Every multiply-add is an explicit __fmaf_rn and every lone product / sum / quotient an
// explicit __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn (tests/relax_ref.py restates the chain in fp64, one 2^-24 per operation):
//   pair     y_i = f_prev_i - f_i;  ys = sum_l dot3(y_i, s_i), yy = sum_l dot3(y_i, y_i), ss = sum_l dot3(s_i, s_i)   (s = S[head])
//            accept iff ys > 0 and ys ys > (c c) (yy ss)   (c = NNHIP_LBFGS_CURVATURE_MIN; each product one rounding);  rho = 1 / ys
//            (rejected with all m slots taken: the pending s had replaced the oldest pair's, so that pair is gone: n_pairs = m - 1)
//   loop 1   q = -f;  newest pair first:  a = rho (sum_l dot3(s_i, q_i));  q = fma(-a, y, q)
//            z = q / alpha
//   loop 2   oldest pair first:  c = a - rho (sum_l dot3(y_i, z_i));  z = fma(c, s, z)
//   step     l2 = max_i dot3(z_i, z_i);  longest = sqrt(l2);  if longest >= maxstep:  z = z (maxstep / longest)
//            x_out = x + (-z)  (a fixed atom: x itself);  S[head] = x_out - x;  f_prev = f
//
// The caller's side of a step is a policy object P:
//   void force(int i, float* f) const          the force of atom i the optimiser sees, exactly 0 for a fixed atom
//   bool is_free(int i) const
//   void load_x(size_t o, float* x) const      the point the step leaves from (o = 3 i)
//   void store_x(size_t o, const float* x_out, const float* x) const     where the new point goes
#pragma once
#include "common.h"
#include "optim_rows.h"

namespace lbfgs_chain {

struct History {
  float* S;        // [m][N][3]
  float* Y;        // [m][N][3]
  float* rho;      // [B][m]
  float* f_prev;   // [N][3]
  float* work;     // [N][3]: the two-loop vector of molecules above 64 atoms
  float alpha, maxstep;
  int memory, n_atoms;
};

// ---- the teams.  A team gives: STRIDE (its size; member `first()` owns the rows a0 + first(), + STRIDE, ... in EVERY sweep),
// lane() (the place in the wave: the first loop's coefficient a_j lives in lane j of every wave), sum / sum3 / max (the reductions;
// every member holds the same bits afterwards) and share_rows (three rows of three floats from their owners to every member).

// one wave64: the butterfly alone, no barrier, no LDS
struct WaveTeam {
  static constexpr int STRIDE = 64;
  int l;
  __device__ __forceinline__ int first() const { return l; }
  __device__ __forceinline__ int lane() const { return l; }
  __device__ __forceinline__ float sum(float s) { return bfly_sum(s); }
  __device__ __forceinline__ void sum3(float& a, float& b, float& c) {
    a = bfly_sum(a);
    b = bfly_sum(b);
    c = bfly_sum(c);
  }
  __device__ __forceinline__ float max(float s) { return bfly_max(s); }
  __device__ __forceinline__ void share_rows(const int* owner, float (*v)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) v[k][j] = __shfl(v[k][j], owner[k], 64);
  }
};

// one workgroup of NNHIP_LBFGS_WG_THREADS = 1024 threads (16 waves).  Thread t owns the rows a0 + t, + 1024, ... in every sweep, so
// it still only re-reads global rows it wrote itself: the work vector, S, Y and f_prev need no barrier.  A reduction is
//   1. the thread-local sum (or max) in row order (the caller's loop)         2. the butterfly 32 .. 1 within each wave
//   3. lane 0 of wave w writes partial[w] to LDS; ONE barrier
//   4. EVERY thread reads the 16 partials and folds them itself, in the fixed order
//        for (d = 8; d >= 1; d >>= 1) for (i < d) p[i] = p[i] + p[i + d]      (__fadd_rn; fmaxf for the max)
// so all 1024 threads hold the same bits afterwards and every decision taken from a reduced value is uniform over the workgroup by
// construction.  The three sums of the pending pair share one barrier.
//
// One barrier per reduction is enough because consecutive reductions ALTERNATE between two LDS buffers (`phase`, which every
// thread toggles at every reduction, across the systems of the grid-stride loop too): a thread writes buffer X for reduction k + 2
// only after it has passed the barrier of reduction k + 1, and every thread arrives at that barrier only after it has read buffer
// X for reduction k (the reads precede the arrival in program order, and the values are consumed before it).  The `rows` buffer of
// share_rows is read after its own barrier and written again only after at least one reduction barrier of a LATER system (every
// system that reaches share_rows has been through the reductions of its step), which every thread reaches after its reads.
//
// Rules, for the machines this runs on: every __syncthreads() below is reached in control flow that is uniform over the workgroup
// -- the callers branch only on values every thread loaded from the same address or on a reduced value, and that includes every
// `continue` of the grid-stride loop over systems; no communication between workgroups, no cooperative launch, no grid-wide
// barrier; no spin-wait, no atomic; no loop whose trip count depends on data other than n and n_pairs.
struct BlockTeam {
  static constexpr int STRIDE = NNHIP_LBFGS_WG_THREADS;
  static constexpr int WAVES = STRIDE / 64;
  static constexpr int RED_FLOATS = 2 * 3 * WAVES;    // two buffers of three sums
  static constexpr int ROW_FLOATS = 9;
  static_assert(WAVES == 16, "the fold below is written for 16 partials");
  float* red;      // LDS [2][3][WAVES]
  float* rows;     // LDS [3][3]
  int tid, phase;
  __device__ __forceinline__ int first() const { return tid; }
  __device__ __forceinline__ int lane() const { return tid & 63; }
  template <bool MAX>
  __device__ __forceinline__ static float fold(const float* part) {
    float p[WAVES];
#pragma unroll
    for (int i = 0; i < WAVES; ++i) p[i] = part[i];
#pragma unroll
    for (int d = WAVES / 2; d >= 1; d >>= 1)
#pragma unroll
      for (int i = 0; i < d; ++i) p[i] = MAX ? fmaxf(p[i], p[i + d]) : __fadd_rn(p[i], p[i + d]);
    return p[0];
  }
  __device__ __forceinline__ float sum(float s) {
    float* buf = red + phase * 3 * WAVES;
    s = bfly_sum(s);
    if (lane() == 0) buf[tid >> 6] = s;
    __syncthreads();
    phase ^= 1;
    return fold<false>(buf);
  }
  __device__ __forceinline__ void sum3(float& a, float& b, float& c) {
    float* buf = red + phase * 3 * WAVES;
    a = bfly_sum(a);
    b = bfly_sum(b);
    c = bfly_sum(c);
    if (lane() == 0) {
      buf[tid >> 6] = a;
      buf[WAVES + (tid >> 6)] = b;
      buf[2 * WAVES + (tid >> 6)] = c;
    }
    __syncthreads();
    phase ^= 1;
    a = fold<false>(buf);
    b = fold<false>(buf + WAVES);
    c = fold<false>(buf + 2 * WAVES);
  }
  __device__ __forceinline__ float max(float s) {
    float* buf = red + phase * 3 * WAVES;
    s = bfly_max(s);
    if (lane() == 0) buf[tid >> 6] = s;
    __syncthreads();
    phase ^= 1;
    return fold<true>(buf);
  }
  // the owners hold their rows in v; afterwards every thread does (through LDS: no thread re-reads global memory another wrote)
  __device__ __forceinline__ void share_rows(const int* owner, float (*v)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (tid == owner[k]) {
#pragma unroll
        for (int j = 0; j < 3; ++j) rows[3 * k + j] = v[k][j];
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) v[k][j] = rows[3 * k + j];
  }
};

// which kernel a system [a0, a1) belongs to when a launch is the pair of a WaveTeam kernel and a BlockTeam kernel (relax.hip,
// cellrelax.hip): the workgroup kernel takes the systems of at least wg_min_atoms atoms (wg_min_atoms <= 0: all of them, and the
// wave kernel is not launched); a system whose mol_ptr leaves the arrays has no atom count and stays with the wave kernel unless
// that is not launched.  The two kernels own disjoint systems and touch no word of the other's
__device__ __forceinline__ bool wave_owns(int wg_min_atoms, int a0, int a1, bool bad_ptr) {
  return wg_min_atoms > 0 && (bad_ptr || a1 - a0 < wg_min_atoms);
}

// the two-loop work vector of one team member: its single atom's three values in registers (REG: molecules of up to Team::STRIDE
// atoms), or the member's own rows of History::work
template <bool REG>
struct Work {
  float r[3];
  float* w;
  __device__ __forceinline__ void get(size_t o, float* v) const {
    if (REG) {
      v[0] = r[0], v[1] = r[1], v[2] = r[2];
    } else {
      load3(w, o, v);
    }
  }
  __device__ __forceinline__ void put(size_t o, const float* v) {
    if (REG) {
      r[0] = v[0], r[1] = v[1], r[2] = v[2];
    } else {
      store3(w, o, v);
    }
  }
};

// the pending pair of a molecule that has stepped before: s is in slot `head`, y = f_prev - f.  np, head: the state before, and on
// return after, the pair.  fresh_slot (-1: none) is the slot whose rho this launch has just formed: fresh_rho is that value in a
// register of every member (member 0's store of it is not a thing the others may read back)
template <class Team, class P>
__device__ __forceinline__ void pending_pair(const History& h, const P& p, Team& team, int b, int a0, int a1, int& np, int& head,
                                             int& fresh_slot, float& fresh_rho) {
  const int m = h.memory;
  const size_t slot_stride = 3 * (size_t)h.n_atoms;
  const float* Sh = h.S + head * slot_stride;
  float ys = 0.f, yy = 0.f, ss = 0.f;
  for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
    float f[3], fp[3], s[3], y[3];
    p.force(i, f);
    load3(h.f_prev, 3 * (size_t)i, fp);
    load3(Sh, 3 * (size_t)i, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) y[k] = __fsub_rn(fp[k], f[k]);
    ys = __fadd_rn(ys, dot3(y, s));
    yy = __fadd_rn(yy, dot3(y, y));
    ss = __fadd_rn(ss, dot3(s, s));
  }
  team.sum3(ys, yy, ss);
  const float c2 = __fmul_rn(NNHIP_LBFGS_CURVATURE_MIN, NNHIP_LBFGS_CURVATURE_MIN);
  if (ys > 0.f && __fmul_rn(ys, ys) > __fmul_rn(c2, __fmul_rn(yy, ss))) {
    float* Yh = h.Y + head * slot_stride;
    for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
      float f[3], fp[3], y[3];
      p.force(i, f);
      load3(h.f_prev, 3 * (size_t)i, fp);
#pragma unroll
      for (int k = 0; k < 3; ++k) y[k] = __fsub_rn(fp[k], f[k]);
      store3(Yh, 3 * (size_t)i, y);
    }
    fresh_slot = head;
    fresh_rho = __fdiv_rn(1.f, ys);
    if (team.first() == 0) h.rho[(size_t)b * m + head] = fresh_rho;
    np = np + 1 > m ? m : np + 1;
    head = (head + 1) % m;
  } else if (np == m) {
    np = m - 1;                                    // a full ring: the rejected s had overwritten the oldest pair's
  }
}

// the two-loop recursion, the clamp and the step of the molecule [a0, a1) of this team; np, head: the state AFTER the pending pair
template <bool REG, class Team, class P>
__device__ void two_loop_and_step(const History& h, const P& p, Team& team, int b, int a0, int a1, int np, int head, int fresh_slot,
                                  float fresh_rho) {
  const int m = h.memory;
  const size_t slot_stride = 3 * (size_t)h.n_atoms;
  const float* rho = h.rho + (size_t)b * m;
  Work<REG> q;
  q.w = h.work;
  for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
    float f[3];
    p.force(i, f);
    const float v[3] = {-f[0], -f[1], -f[2]};
    q.put(3 * (size_t)i, v);
  }
  float a_lane = 0.f;                                   // lane j (of every wave): the coefficient a of the j-th newest pair
  for (int j = 0; j < np; ++j) {
    const int slot = (head - 1 - j + 2 * m) % m;
    const float* Sj = h.S + slot * slot_stride;
    const float* Yj = h.Y + slot * slot_stride;
    float acc = 0.f;
    for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
      float s[3], v[3];
      load3(Sj, 3 * (size_t)i, s);
      q.get(3 * (size_t)i, v);
      acc = __fadd_rn(acc, dot3(s, v));
    }
    const float a = __fmul_rn(slot == fresh_slot ? fresh_rho : rho[slot], team.sum(acc));
    if (team.lane() == j) a_lane = a;
    for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
      float y[3], v[3];
      load3(Yj, 3 * (size_t)i, y);
      q.get(3 * (size_t)i, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = __fmaf_rn(-a, y[k], v[k]);
      q.put(3 * (size_t)i, v);
    }
  }
  for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
    float v[3];
    q.get(3 * (size_t)i, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = __fdiv_rn(v[k], h.alpha);
    q.put(3 * (size_t)i, v);
  }
  for (int j = np - 1; j >= 0; --j) {
    const int slot = (head - 1 - j + 2 * m) % m;
    const float* Sj = h.S + slot * slot_stride;
    const float* Yj = h.Y + slot * slot_stride;
    float acc = 0.f;
    for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
      float y[3], v[3];
      load3(Yj, 3 * (size_t)i, y);
      q.get(3 * (size_t)i, v);
      acc = __fadd_rn(acc, dot3(y, v));
    }
    const float c = __fsub_rn(__shfl(a_lane, j, 64), __fmul_rn(slot == fresh_slot ? fresh_rho : rho[slot], team.sum(acc)));
    for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
      float s[3], v[3];
      load3(Sj, 3 * (size_t)i, s);
      q.get(3 * (size_t)i, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = __fmaf_rn(c, s[k], v[k]);
      q.put(3 * (size_t)i, v);
    }
  }
  float l2 = 0.f;
  for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
    float v[3];
    q.get(3 * (size_t)i, v);
    l2 = fmaxf(l2, dot3(v, v));
  }
  const float longest = __fsqrt_rn(team.max(l2));
  const bool clamp = longest >= h.maxstep;
  const float scale = clamp ? __fdiv_rn(h.maxstep, longest) : 1.f;
  float* Sh = h.S + head * slot_stride;
  for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
    const size_t o = 3 * (size_t)i;
    float v[3], x[3], f[3], xo[3], s[3];
    q.get(o, v);
    p.load_x(o, x);
    p.force(i, f);
    const bool is_free = p.is_free(i);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float z = clamp ? __fmul_rn(v[k], scale) : v[k];
      xo[k] = is_free ? __fadd_rn(x[k], -z) : x[k];
      s[k] = __fsub_rn(xo[k], x[k]);
    }
    p.store_x(o, xo, x);
    store3(Sh, o, s);
    store3(h.f_prev, o, f);
  }
}

// one whole step: the pending pair when the molecule has stepped before (`stepped`), then the recursion and the step.  np, head:
// the state words before; on return the ones to store
// (`stepped` must be uniform over the team: the pair's reduction holds a barrier in BlockTeam)
template <class Team, class P>
__device__ __forceinline__ void step(const History& h, const P& p, Team& team, int b, int a0, int a1, bool stepped, int& np,
                                     int& head) {
  int fresh_slot = -1;
  float fresh_rho = 0.f;
  if (stepped) pending_pair(h, p, team, b, a0, a1, np, head, fresh_slot, fresh_rho);
  if (a1 - a0 <= Team::STRIDE) {
    two_loop_and_step<true>(h, p, team, b, a0, a1, np, head, fresh_slot, fresh_rho);
  } else {
    two_loop_and_step<false>(h, p, team, b, a0, a1, np, head, fresh_slot, fresh_rho);
  }
}

}  // namespace lbfgs_chain
