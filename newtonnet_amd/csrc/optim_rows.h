// What the optimiser kernels (relax.hip, cellrelax.hip, dimer.hip through lbfgs_chain.h; neb.hip, irc.hip) share below the level
// of a method: rows of three floats, the free-atom mask, and the wave-wide butterfly reductions (gfx950, fp32, every operation an
// explicitly rounded one).
#pragma once
#include "common.h"

__device__ __forceinline__ float dot3(const float* a, const float* b) {
  return __fmaf_rn(a[2], b[2], __fmaf_rn(a[1], b[1], __fmul_rn(a[0], b[0])));
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

// atom i moves (Args: the argument struct of a kernel, with the optional free_mask [N] of its entry point)
template <class Args>
__device__ __forceinline__ bool is_free(const Args& g, int i) {
  return !g.free_mask || g.free_mask[i];
}

// The wave-wide sum and max of the optimisers: the fixed butterfly __shfl_xor 32, 16, ..., 1 -- a + b and b + a round alike, so
// all 64 lanes hold the same bits afterwards.  NOT common.h's wave_sum: that one is the DPP form, which adds the lanes in another
// order and so gives other bits; the fp64 and fp32 references of the optimisers (tests/relax_ref.py, irc_ref.py, neb_ref.py,
// dimer_ref.py) model the butterfly, and the different name keeps a call from binding to the DPP form by accident.
__device__ __forceinline__ float bfly_sum(float s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s = __fadd_rn(s, __shfl_xor(s, d, 64));
  return s;
}

__device__ __forceinline__ float bfly_max(float s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s = fmaxf(s, __shfl_xor(s, d, 64));
  return s;
}
