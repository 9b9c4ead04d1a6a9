// Geometry relaxation on the device (gfx950, fp32): one launch per optimisation step moves every molecule of a batch by one
// L-BFGS step.  The method is L-BFGS without line search in ASE's convention (ase/optimize/lbfgs.py: fixed H0 = 1 / alpha, the
// longest atomic displacement capped at maxstep), with one stated deviation: a curvature pair is only taken into the history when
// y.s > 0 and cos(y, s) > NNHIP_LBFGS_CURVATURE_MIN (include/newtonnet_hip.h spells the contract out).  A step of the driver
// (newtonnet_amd/relax.py) is  model(pos) -> lbfgs_step.
//
// One wave64 per molecule, four molecules per workgroup (as md_kinetic_kernel).  Lane l owns the atoms l, l + 64, ... of its
// molecule in EVERY sweep, so a lane only ever re-reads what it wrote itself: no barrier, no LDS.  Every per-molecule reduction is
// a lane-local sum (or max) in atom order, then the fixed butterfly __shfl_xor 32, 16, ..., 1 -- a + b and b + a round alike, so
// all 64 lanes hold the same bits afterwards and every decision is uniform over the wave.  No float atomics: a molecule's result
// does not depend on the rest of the batch or on its place in it.  The two-loop work vector (q, then z) of a molecule of up to 64
// atoms is three registers per lane; a larger molecule walks `work` [N,3] (its own rows).  The coefficients a_i of the first loop
// live in lane i of one register (hence memory <= 64).
//
// Every multiply-add is an explicit __fmaf_rn and every lone product / sum / quotient an explicit __fmul_rn / __fadd_rn / __fsub_rn
// / __fdiv_rn, so the rounding chain does not depend on the compiler's contraction; tests/relax_ref.py restates it in fp64 with one
// 2^-24 per operation.  The chain, for one molecule (sum_l: the reduction above; dot3(a, b) = fma(az, bz, fma(ay, by, ax bx))):
//   f_i      = F_i (free) or 0 (fixed);   fmax2 = max_i dot3(f_i, f_i);   fmax_out = sqrt(fmax2)
//   pair     y_i = f_prev_i - f_i;  ys = sum_l dot3(y_i, s_i), yy = sum_l dot3(y_i, y_i), ss = sum_l dot3(s_i, s_i)   (s = S[head])
//            accept iff ys > 0 and ys ys > (c c) (yy ss)   (c = NNHIP_LBFGS_CURVATURE_MIN; each product one rounding);  rho = 1 / ys
//            (rejected with all m slots taken: the pending s had replaced the oldest pair's, so that pair is gone: n_pairs = m - 1)
//   loop 1   q = -f;  newest pair first:  a = rho (sum_l dot3(s_i, q_i));  q = fma(-a, y, q)
//            z = q / alpha
//   loop 2   oldest pair first:  c = a - rho (sum_l dot3(y_i, z_i));  z = fma(c, s, z)
//   step     l2 = max_i dot3(z_i, z_i);  longest = sqrt(l2);  if longest >= maxstep:  z = z (maxstep / longest)
//            pos_out = pos_in + (-z)  (a fixed atom: pos_in itself);  S[head] = pos_out - pos_in;  f_prev = f
// The cost of a molecule of n atoms is about 2 m ceil(n / 64) dependent sweeps of ONE wave: this kernel is for batches of
// molecules, not for one large system (tools/bench_relax.py reports what that costs).
#include "common.h"

namespace {

constexpr int RX_THREADS = 256;
constexpr int RX_MAX_BLOCKS = 2048;

struct RelaxArgs {
  const float* pos_in;
  const float* force;
  const uint8_t* free_mask;
  const int32_t* mol_ptr;
  int32_t* converged;
  int32_t* n_steps;
  int32_t* n_pairs;
  int32_t* head;
  float* S;
  float* Y;
  float* rho;
  float* f_prev;
  float* work;
  float* pos_out;
  float* fmax_out;
  float tol2, alpha, maxstep;
  int flags, n_mol, n_atoms, memory;
};

__device__ __forceinline__ float dot3(const float* a, const float* b) {
  return __fmaf_rn(a[2], b[2], __fmaf_rn(a[1], b[1], __fmul_rn(a[0], b[0])));
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s = __fadd_rn(s, __shfl_xor(s, d, 64));
  return s;
}

__device__ __forceinline__ float wave_max(float s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s = fmaxf(s, __shfl_xor(s, d, 64));
  return s;
}

__device__ __forceinline__ void load3(const float* p, size_t o, float* v) {
  v[0] = p[o];
  v[1] = p[o + 1];
  v[2] = p[o + 2];
}

__device__ __forceinline__ void store3(float* p, size_t o, const float* v) {
  p[o] = v[0];
  p[o + 1] = v[1];
  p[o + 2] = v[2];
}

// the two-loop work vector of one lane: its single atom's three values in registers (REG: molecules of up to 64 atoms), or the
// lane's own rows of g.work
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

__device__ __forceinline__ void masked_force(const RelaxArgs& g, int i, float* f) {
  load3(g.force, 3 * (size_t)i, f);
  if (g.free_mask && !g.free_mask[i]) f[0] = f[1] = f[2] = 0.f;
}

// everything after the frozen / state checks, for the molecule [a0, a1) of this wave; np, head: the state AFTER the pending pair.
// fresh_slot (-1: none) is the slot whose rho this launch has just formed: fresh_rho is that value in a register of every lane
// (lane 0's store of it is not a thing the other lanes may read back)
template <bool REG>
__device__ void two_loop_and_step(const RelaxArgs& g, int b, int a0, int a1, int lane, int np, int head, int fresh_slot,
                                  float fresh_rho) {
  const int m = g.memory;
  const size_t slot_stride = 3 * (size_t)g.n_atoms;
  const float* rho = g.rho + (size_t)b * m;
  Work<REG> q;
  q.w = g.work;
  for (int i = a0 + lane; i < a1; i += 64) {
    float f[3];
    masked_force(g, i, f);
    const float v[3] = {-f[0], -f[1], -f[2]};
    q.put(3 * (size_t)i, v);
  }
  float a_lane = 0.f;                                   // lane j: the coefficient a of the j-th newest pair
  for (int j = 0; j < np; ++j) {
    const int slot = (head - 1 - j + 2 * m) % m;
    const float* Sj = g.S + slot * slot_stride;
    const float* Yj = g.Y + slot * slot_stride;
    float acc = 0.f;
    for (int i = a0 + lane; i < a1; i += 64) {
      float s[3], v[3];
      load3(Sj, 3 * (size_t)i, s);
      q.get(3 * (size_t)i, v);
      acc = __fadd_rn(acc, dot3(s, v));
    }
    const float a = __fmul_rn(slot == fresh_slot ? fresh_rho : rho[slot], wave_sum(acc));
    if (lane == j) a_lane = a;
    for (int i = a0 + lane; i < a1; i += 64) {
      float y[3], v[3];
      load3(Yj, 3 * (size_t)i, y);
      q.get(3 * (size_t)i, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = __fmaf_rn(-a, y[k], v[k]);
      q.put(3 * (size_t)i, v);
    }
  }
  for (int i = a0 + lane; i < a1; i += 64) {
    float v[3];
    q.get(3 * (size_t)i, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = __fdiv_rn(v[k], g.alpha);
    q.put(3 * (size_t)i, v);
  }
  for (int j = np - 1; j >= 0; --j) {
    const int slot = (head - 1 - j + 2 * m) % m;
    const float* Sj = g.S + slot * slot_stride;
    const float* Yj = g.Y + slot * slot_stride;
    float acc = 0.f;
    for (int i = a0 + lane; i < a1; i += 64) {
      float y[3], v[3];
      load3(Yj, 3 * (size_t)i, y);
      q.get(3 * (size_t)i, v);
      acc = __fadd_rn(acc, dot3(y, v));
    }
    const float c = __fsub_rn(__shfl(a_lane, j, 64), __fmul_rn(slot == fresh_slot ? fresh_rho : rho[slot], wave_sum(acc)));
    for (int i = a0 + lane; i < a1; i += 64) {
      float s[3], v[3];
      load3(Sj, 3 * (size_t)i, s);
      q.get(3 * (size_t)i, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = __fmaf_rn(c, s[k], v[k]);
      q.put(3 * (size_t)i, v);
    }
  }
  float l2 = 0.f;
  for (int i = a0 + lane; i < a1; i += 64) {
    float v[3];
    q.get(3 * (size_t)i, v);
    l2 = fmaxf(l2, dot3(v, v));
  }
  const float longest = __fsqrt_rn(wave_max(l2));
  const bool clamp = longest >= g.maxstep;
  const float scale = clamp ? __fdiv_rn(g.maxstep, longest) : 1.f;
  float* Sh = g.S + head * slot_stride;
  for (int i = a0 + lane; i < a1; i += 64) {
    const size_t o = 3 * (size_t)i;
    float v[3], x[3], f[3], xo[3], s[3];
    q.get(o, v);
    load3(g.pos_in, o, x);
    masked_force(g, i, f);
    const bool is_free = !g.free_mask || g.free_mask[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float z = clamp ? __fmul_rn(v[k], scale) : v[k];
      xo[k] = is_free ? __fadd_rn(x[k], -z) : x[k];
      s[k] = __fsub_rn(xo[k], x[k]);
    }
    store3(g.pos_out, o, xo);
    store3(Sh, o, s);
    store3(g.f_prev, o, f);
  }
}

__global__ void __launch_bounds__(RX_THREADS)
lbfgs_step_kernel(RelaxArgs g) {
  const int lane = threadIdx.x & 63;
  const int waves = RX_THREADS / 64;
  const int m = g.memory;
  const size_t slot_stride = 3 * (size_t)g.n_atoms;
  for (int b = blockIdx.x * waves + (threadIdx.x >> 6); b < g.n_mol; b += gridDim.x * waves) {   // (uniform over a wave)
    const int a0 = g.mol_ptr[b], a1 = g.mol_ptr[b + 1];
    const bool bad_ptr = a0 < 0 || a1 < a0 || a1 > g.n_atoms;
    float f2 = 0.f;
    for (int i = a0 + lane; i < a1 && !bad_ptr; i += 64) {
      float f[3];
      masked_force(g, i, f);
      f2 = fmaxf(f2, dot3(f, f));
    }
    const float fmax2 = wave_max(f2);
    const int steps = g.n_steps[b];
    int np = g.n_pairs[b], head = g.head[b];
    // state words no step can have left behind (or a mol_ptr that leaves the arrays): the molecule is not touched, fmax_out = NaN
    const bool bad = bad_ptr || steps < 0 || np < 0 || np > m || head < 0 || head >= m;
    const bool was = g.converged[b] != 0;
    const bool now = !bad && (a1 == a0 || fmax2 < g.tol2);
    if (lane == 0) {
      g.fmax_out[b] = bad ? __builtin_nanf("") : __fsqrt_rn(fmax2);
      if (now && !was) g.converged[b] = 1;
    }
    if (bad) continue;
    if (was || now || (g.flags & NNHIP_LBFGS_CHECK_ONLY)) {
      for (int i = a0 + lane; i < a1; i += 64) {
        float x[3];
        load3(g.pos_in, 3 * (size_t)i, x);
        store3(g.pos_out, 3 * (size_t)i, x);
      }
      continue;
    }
    int fresh_slot = -1;
    float fresh_rho = 0.f;
    if (steps > 0) {                                   // the pending pair: s is in slot `head`, y = f_prev - f
      const float* Sh = g.S + head * slot_stride;
      float ys = 0.f, yy = 0.f, ss = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        float f[3], fp[3], s[3], y[3];
        masked_force(g, i, f);
        load3(g.f_prev, 3 * (size_t)i, fp);
        load3(Sh, 3 * (size_t)i, s);
#pragma unroll
        for (int k = 0; k < 3; ++k) y[k] = __fsub_rn(fp[k], f[k]);
        ys = __fadd_rn(ys, dot3(y, s));
        yy = __fadd_rn(yy, dot3(y, y));
        ss = __fadd_rn(ss, dot3(s, s));
      }
      ys = wave_sum(ys);
      yy = wave_sum(yy);
      ss = wave_sum(ss);
      const float c2 = __fmul_rn(NNHIP_LBFGS_CURVATURE_MIN, NNHIP_LBFGS_CURVATURE_MIN);
      if (ys > 0.f && __fmul_rn(ys, ys) > __fmul_rn(c2, __fmul_rn(yy, ss))) {
        float* Yh = g.Y + head * slot_stride;
        for (int i = a0 + lane; i < a1; i += 64) {
          float f[3], fp[3], y[3];
          masked_force(g, i, f);
          load3(g.f_prev, 3 * (size_t)i, fp);
#pragma unroll
          for (int k = 0; k < 3; ++k) y[k] = __fsub_rn(fp[k], f[k]);
          store3(Yh, 3 * (size_t)i, y);
        }
        fresh_slot = head;
        fresh_rho = __fdiv_rn(1.f, ys);
        if (lane == 0) g.rho[(size_t)b * m + head] = fresh_rho;
        np = np + 1 > m ? m : np + 1;
        head = (head + 1) % m;
      } else if (np == m) {
        np = m - 1;                                    // a full ring: the rejected s had overwritten the oldest pair's
      }
    }
    if (a1 - a0 <= 64) {
      two_loop_and_step<true>(g, b, a0, a1, lane, np, head, fresh_slot, fresh_rho);
    } else {
      two_loop_and_step<false>(g, b, a0, a1, lane, np, head, fresh_slot, fresh_rho);
    }
    if (lane == 0) {
      g.n_steps[b] = steps + 1;
      g.n_pairs[b] = np;
      g.head[b] = head;
    }
  }
}

}  // namespace

extern "C" int nnhip_lbfgs_step(const float* pos_in, const float* force, const uint8_t* free_mask, const int32_t* mol_ptr,
                                int32_t n_mol, int32_t n_atoms, int32_t memory, float tol2, float alpha, float maxstep,
                                int32_t flags, int32_t* converged, int32_t* n_steps, int32_t* n_pairs, int32_t* head, float* S,
                                float* Y, float* rho, float* f_prev, float* work, float* pos_out, float* fmax_out, void* stream) {
  if (n_mol < 0 || n_atoms < 0 || memory < 1 || memory > NNHIP_LBFGS_MAX_MEMORY || (flags & ~NNHIP_LBFGS_CHECK_ONLY)) {
    nnhip_set_error("nnhip_lbfgs_step: bad arguments (n_mol %d, n_atoms %d, memory %d: 1 .. %d, flags %d: 0 or "
                    "NNHIP_LBFGS_CHECK_ONLY)", n_mol, n_atoms, memory, NNHIP_LBFGS_MAX_MEMORY, flags);
    return NNHIP_E_INVALID;
  }
  if (!(tol2 >= 0.f) || !(alpha > 0.f) || !(maxstep > 0.f)) {
    nnhip_set_error("nnhip_lbfgs_step: tol2 >= 0, alpha > 0 and maxstep > 0 expected (got %g, %g, %g)", (double)tol2,
                    (double)alpha, (double)maxstep);
    return NNHIP_E_INVALID;
  }
  if (n_mol == 0) return NNHIP_OK;
  if (!mol_ptr || !converged || !n_steps || !n_pairs || !head || !rho || !fmax_out) {
    nnhip_set_error("nnhip_lbfgs_step: null pointer (mol_ptr, converged, n_steps, n_pairs, head, rho and fmax_out are mandatory)");
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && (!pos_in || !force || !S || !Y || !f_prev || !pos_out || (n_atoms > 64 && !work))) {
    nnhip_set_error("nnhip_lbfgs_step: null pointer (pos_in, force, S, Y, f_prev and pos_out are mandatory; work [N,3] when "
                    "n_atoms > 64)");
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && overlap(pos_in, pos_out, 3 * (size_t)n_atoms)) {
    nnhip_set_error("nnhip_lbfgs_step: pos_out may not alias pos_in (a forward call that has to be repeated reads pos_in again)");
    return NNHIP_E_INVALID;
  }
  RelaxArgs g;
  g.pos_in = pos_in;
  g.force = force;
  g.free_mask = free_mask;
  g.mol_ptr = mol_ptr;
  g.converged = converged;
  g.n_steps = n_steps;
  g.n_pairs = n_pairs;
  g.head = head;
  g.S = S;
  g.Y = Y;
  g.rho = rho;
  g.f_prev = f_prev;
  g.work = work;
  g.pos_out = pos_out;
  g.fmax_out = fmax_out;
  g.tol2 = tol2;
  g.alpha = alpha;
  g.maxstep = maxstep;
  g.flags = flags;
  g.n_mol = n_mol;
  g.n_atoms = n_atoms;
  g.memory = memory;
  const int waves = RX_THREADS / 64;
  int blocks = (n_mol + waves - 1) / waves;
  blocks = blocks > RX_MAX_BLOCKS ? RX_MAX_BLOCKS : blocks;
  lbfgs_step_kernel<<<blocks, RX_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
