// The per-atom BAOAB chain of the molecular-dynamics kernels (gfx950, fp32): the one definition that md_step_kernel (md.hip, for
// nnhip_md_step and nnhip_npt_step), npt_barostat_kernel (npt.hip: the kinetic energy of the full-step velocities) and
// md_step_constrained_kernel (rattle.hip: its unconstrained molecules whole, its constrained ones kick, kinetic energy and O step)
// share, so that "the same bits as nnhip_md_step" is a property of the text and not of three texts that agree.
//
// Per atom i and coordinate k, every operation in fp32, every multiply-add an explicit __fmaf_rn and every lone product an explicit
// __fmul_rn: the rounding chain does not depend on the compiler's contraction (tests/md_ref.py and tests/npt_ref.py restate it in
// fp64 with one 2^-24 per operation):
//   half_kick (B):  v = fma(hk_i, F_ik, v)                                              hk_i = dt / (2 m_i)
//   kinetic:        ke_i = (0.5 m_i) * fma(vz, vz, fma(vy, vy, vx * vx))
//   o_step (O):     v = fma(sigma_i, xi_ik, c1 * v)
//   begin:          half_kick;  [x = mu * x_in;  v = inv_mu * v]  x = fma(dth, v, x);  [o_step]  x_out = fma(dth, v, x)
//                   the first bracket (S, the cell rescale of constant-pressure dynamics) only in begin<true>: begin<false> has no
//                   product with 1;  the second only with noise (xi != NULL);  dth = dt / 2
#pragma once
#include "common.h"

namespace md_chain {

__device__ __forceinline__ void half_kick(float v[3], float hk, const float* f) {
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = __fmaf_rn(hk, f[k], v[k]);
}

__device__ __forceinline__ float kinetic(const float v[3], float mass) {
  const float s = __fmaf_rn(v[2], v[2], __fmaf_rn(v[1], v[1], __fmul_rn(v[0], v[0])));
  return __fmul_rn(__fmul_rn(0.5f, mass), s);
}

__device__ __forceinline__ void o_step(float v[3], float sigma, const float* xi, float c1) {
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = __fmaf_rn(sigma, xi[k], __fmul_rn(c1, v[k]));
}

// x_in, x_out, f and xi point at the atom's three values; xi == NULL: no O step; mu and inv_mu are used only when RESCALE
template <bool RESCALE>
__device__ __forceinline__ void begin(float v[3], float hk, const float* f, const float* x_in, float* x_out, float dth, float sigma,
                                      const float* xi, float c1, float mu, float inv_mu) {
  float x[3] = {x_in[0], x_in[1], x_in[2]};
  half_kick(v, hk, f);
  if constexpr (RESCALE) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = __fmul_rn(mu, x[k]);
      v[k] = __fmul_rn(inv_mu, v[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) x[k] = __fmaf_rn(dth, v[k], x[k]);
  if (xi) o_step(v, sigma, xi, c1);
#pragma unroll
  for (int k = 0; k < 3; ++k) x_out[k] = __fmaf_rn(dth, v[k], x[k]);
}

}  // namespace md_chain
