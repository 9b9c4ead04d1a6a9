// Constant-pressure molecular dynamics on the device (gfx950, fp32): isotropic stochastic cell rescaling (Bernetti & Bussi 2020) as a
// first-order step for eps = ln V inside the BAOAB step of csrc/md.hip.  A step of the driver (newtonnet_amd/npt.py) is
//   model(pos, cell) -> npt_barostat -> npt_step(finish | begin):   B(F_k) [full-step v, KE] B(F_k) S A O A
// Two launches: the barostat below, and nnhip_npt_step, which is md_step_kernel<true> of csrc/md.hip (the BAOAB chain with the
// rescale S; the chain is written once, in csrc/md_chain.h).  Every operation in fp32, every multiply-add an explicit __fmaf_rn,
// every lone product, sum, quotient and root an explicit __f*_rn, so that the rounding chain does not depend on the compiler's
// contraction (tests/npt_ref.py restates both kernels in fp64 with one 2^-24 per operation and 2 ulp for expf).
//
// npt_barostat: one 256-thread workgroup per system b.  Thread t takes the atoms t, t + 256, ... of the system in that order:
//     v' = md_chain::half_kick             (v' = v when force == NULL: no kick is pending; v' is NOT stored)
//     ke_i = md_chain::kinetic(v')         nnhip_md_step's ke_out, from the same text
//     acc = acc + ke_i
//   the 256 partial sums meet in a fixed LDS tree (t < d adds the partial of t + d, d = 128, 64, ..., 1); then thread 0:
//     V     = fma(c02, m2, fma(-c01, m1, c00 * m0)),  m0 = fma(c11, c22, -(c12 * c21)), m1 = fma(c10, c22, -(c12 * c20)),
//                                                     m2 = fma(c10, c21, -(c11 * c20))
//     P     = fma(2, K, (W00 + W11) + W22) / (3 * V)
//     deps  = fma(-a_b, P0_b - P, sqrt(s2_b / V) * xi_b)      with noise;     deps = (-a_b) * (P0_b - P)     without
//             (a_b == 0 without noise: system b is not coupled, deps = +0 whatever P is)
//     e     = deps * fl32(1/3);  mu = expf(e);  inv_mu = expf(-e);  cell_out = mu * cell_in  (nine products)
//   The kernel moves 28-40 bytes per atom: nothing here is tuned.
#include "md_chain.h"

namespace {

constexpr int NPT_THREADS = 256;
constexpr float NPT_THIRD = 0.3333333432674407958984375f;        // fl32(1/3) = 0x3eaaaaab

struct BaroArgs {
  const float* vel;
  const float* force;
  const float* hk;
  const float* mass;
  const int* mol_ptr;
  const float* cell_in;
  const float* virial;
  const float* a;
  const float* p0;
  const float* s2;
  const float* noise;
  float* cell_out;
  float* mu;
  float* inv_mu;
  float* ke;
  float* pressure;
  float* volume;
  float* deps;
  int n_atoms;
};

__global__ void __launch_bounds__(NPT_THREADS)
npt_barostat_kernel(BaroArgs g) {
#pragma clang fp contract(off)       // (acc + ke_i below is a product followed by a plain sum, which stays two roundings here)
  __shared__ float part[NPT_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const int a0 = max(g.mol_ptr[b], 0), a1 = min(g.mol_ptr[b + 1], g.n_atoms);       // (never outside the per-atom arrays)
  float acc = 0.f;
  for (int i = a0 + t; i < a1; i += NPT_THREADS) {
    const size_t o = 3 * (size_t)i;
    float v[3] = {g.vel[o], g.vel[o + 1], g.vel[o + 2]};
    if (g.force) md_chain::half_kick(v, g.hk[i], g.force + o);
    const float ke_i = md_chain::kinetic(v, g.mass[i]);
    acc = acc + ke_i;
  }
  part[t] = acc;
  __syncthreads();
#pragma unroll
  for (int d = NPT_THREADS / 2; d >= 1; d >>= 1) {
    if (t < d) part[t] = __fadd_rn(part[t], part[t + d]);
    __syncthreads();
  }
  if (t != 0) return;
  const float K = part[0];
  const float* c = g.cell_in + 9 * (size_t)b;
  const float* w = g.virial + 9 * (size_t)b;
  const float m0 = __fmaf_rn(c[4], c[8], -__fmul_rn(c[5], c[7]));
  const float m1 = __fmaf_rn(c[3], c[8], -__fmul_rn(c[5], c[6]));
  const float m2 = __fmaf_rn(c[3], c[7], -__fmul_rn(c[4], c[6]));
  const float V = __fmaf_rn(c[2], m2, __fmaf_rn(-c[1], m1, __fmul_rn(c[0], m0)));
  const float trw = __fadd_rn(__fadd_rn(w[0], w[4]), w[8]);
  const float P = __fdiv_rn(__fmaf_rn(2.0f, K, trw), __fmul_rn(3.0f, V));
  const float a = g.a[b];
  float de;
  if (g.noise) {
    const float s = __fsqrt_rn(__fdiv_rn(g.s2[b], V));
    de = __fmaf_rn(-a, __fsub_rn(g.p0[b], P), __fmul_rn(s, g.noise[b]));
  } else {
    de = a == 0.f ? 0.f : __fmul_rn(-a, __fsub_rn(g.p0[b], P));
  }
  const float e = __fmul_rn(de, NPT_THIRD);
  const float mu = expf(e), inv_mu = expf(-e);
  float* co = g.cell_out + 9 * (size_t)b;
#pragma unroll
  for (int k = 0; k < 9; ++k) co[k] = __fmul_rn(mu, c[k]);
  g.mu[b] = mu;
  g.inv_mu[b] = inv_mu;
  g.ke[b] = K;
  g.pressure[b] = P;
  g.volume[b] = V;
  g.deps[b] = de;
}

}  // namespace

extern "C" int nnhip_npt_barostat(const float* vel, const float* force, const float* hk, const float* mass, const int32_t* mol_ptr,
                                  int32_t n_mol, int32_t n_atoms, const float* cell_in, const float* virial, const float* a,
                                  const float* p0, const float* s2, const float* noise, float* cell_out, float* mu, float* inv_mu,
                                  float* ke, float* pressure, float* volume, float* deps, void* stream) {
  if (n_mol < 0 || n_atoms < 0) {
    nnhip_set_error("nnhip_npt_barostat: bad arguments (n_mol %d, n_atoms %d)", n_mol, n_atoms);
    return NNHIP_E_INVALID;
  }
  if ((s2 == nullptr) != (noise == nullptr)) {
    nnhip_set_error("nnhip_npt_barostat: s2 and noise come together (both given or both null)");
    return NNHIP_E_INVALID;
  }
  if (n_mol == 0) return NNHIP_OK;
  if (!vel || !mass || !mol_ptr || !cell_in || !virial || !a || !p0 || !cell_out || !mu || !inv_mu || !ke || !pressure || !volume ||
      !deps || (force && !hk)) {
    nnhip_set_error("nnhip_npt_barostat: bad arguments (vel, mass, mol_ptr, cell_in, virial, a, p0 and every output always; hk with "
                    "force)");
    return NNHIP_E_INVALID;
  }
  if (overlap(cell_in, cell_out, 9 * (size_t)n_mol)) {
    nnhip_set_error("nnhip_npt_barostat: cell_out may not alias cell_in (a forward call that has to be repeated reads cell_in again)");
    return NNHIP_E_INVALID;
  }
  BaroArgs g;
  g.vel = vel;
  g.force = force;
  g.hk = hk;
  g.mass = mass;
  g.mol_ptr = mol_ptr;
  g.cell_in = cell_in;
  g.virial = virial;
  g.a = a;
  g.p0 = p0;
  g.s2 = s2;
  g.noise = noise;
  g.cell_out = cell_out;
  g.mu = mu;
  g.inv_mu = inv_mu;
  g.ke = ke;
  g.pressure = pressure;
  g.volume = volume;
  g.deps = deps;
  g.n_atoms = n_atoms;
  npt_barostat_kernel<<<n_mol, NPT_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
