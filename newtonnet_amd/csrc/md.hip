// Molecular dynamics on the device (gfx950, fp32): one launch per MD step integrates every atom of a batch.
//
// The scheme is BAOAB (Leimkuhler & Matthews 2013) with the O step exact; with c1 = 1 and no noise it is velocity Verlet.  A step
// of the driver (newtonnet_amd/dynamics.py) is  model(pos) -> md_step(finish | begin):  the second half kick of the step whose
// forces have just been evaluated and the first half of the next step in one launch.  Per atom i and coordinate k, every operation
// in fp32 and every multiply-add an explicit __fmaf_rn, every lone product an explicit __fmul_rn, so that the rounding chain does not
// depend on the compiler's contraction (tests/md_ref.py restates it in fp64 with one 2^-24 per operation):
//   finish (flag bit 0):  v = fma(hk_i, F_ik, v)                                       hk_i = dt / (2 m_i)
//                         ke_i = (0.5 m_i) * fma(vz, vz, fma(vy, vy, vx * vx))          only when ke_out != NULL
//   begin  (flag bit 1):  v = fma(hk_i, F_ik, v)                                       B
//                         x = fma(dth, v, x_in)                                        A, dth = dt / 2
//                         v = fma(sigma_i, xi_ik, c1 * v)                              O; skipped entirely when noise == NULL
//                         x_out = fma(dth, v, x)                                       A
// One thread per atom (its three coordinates: the kinetic energy needs them together); 256 threads per workgroup = four wave64s,
// at most 2048 workgroups, the rest by a grid-stride loop; the tail is the loop's bound.  The kernel moves 60-90 bytes per atom
// and is one launch of the ~45 of a step: nothing here is tuned.
//
// nnhip_md_kinetic sums ke [N] per molecule: one wave64 per molecule, lane l adds the atoms l, l + 64, ... of the molecule in that
// order, then the 64 partial sums meet in a fixed butterfly (__shfl_xor 32, 16, ..., 1).  No float atomics: bitwise repeatable, for
// thousands of small molecules (four per workgroup) as for one molecule of 100 000 atoms (1563 adds per lane).
#include "common.h"

namespace {

constexpr int MD_THREADS = 256;
constexpr int MD_MAX_BLOCKS = 2048;

struct MdArgs {
  const float* pos_in;
  float* vel;
  const float* force;
  const float* hk;
  const float* mass;
  const float* sigma;
  const float* noise;
  float* pos_out;
  float* ke_out;
  float dth, c1;
  int flags, n_atoms;
};

__global__ void __launch_bounds__(MD_THREADS)
md_step_kernel(MdArgs g) {
  const bool finish = g.flags & NNHIP_MD_FINISH, begin = g.flags & NNHIP_MD_BEGIN;
  for (int i = blockIdx.x * MD_THREADS + threadIdx.x; i < g.n_atoms; i += gridDim.x * MD_THREADS) {
    const size_t o = 3 * (size_t)i;
    const float hk = g.hk[i];
    float v[3] = {g.vel[o], g.vel[o + 1], g.vel[o + 2]};
    const float f[3] = {g.force[o], g.force[o + 1], g.force[o + 2]};
    if (finish) {
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = __fmaf_rn(hk, f[k], v[k]);
      if (g.ke_out) {
        const float s = __fmaf_rn(v[2], v[2], __fmaf_rn(v[1], v[1], __fmul_rn(v[0], v[0])));
        g.ke_out[i] = __fmul_rn(__fmul_rn(0.5f, g.mass[i]), s);
      }
    }
    if (begin) {
      const float sigma = g.noise ? g.sigma[i] : 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[k] = __fmaf_rn(hk, f[k], v[k]);
        float x = __fmaf_rn(g.dth, v[k], g.pos_in[o + k]);
        if (g.noise) v[k] = __fmaf_rn(sigma, g.noise[o + k], __fmul_rn(g.c1, v[k]));
        g.pos_out[o + k] = __fmaf_rn(g.dth, v[k], x);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) g.vel[o + k] = v[k];
  }
}

__global__ void __launch_bounds__(MD_THREADS)
md_kinetic_kernel(const float* __restrict__ ke, const int* __restrict__ mol_ptr, int n_mol, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int waves = MD_THREADS / 64;
  for (int b = blockIdx.x * waves + (threadIdx.x >> 6); b < n_mol; b += gridDim.x * waves) {   // (uniform over a wave)
    const int a0 = mol_ptr[b], a1 = mol_ptr[b + 1];
    float s = 0.f;
    for (int i = a0 + lane; i < a1; i += 64) s += ke[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) out[b] = s;
  }
}

inline bool overlap(const float* a, const float* b, size_t n) { return a < b + n && b < a + n; }

}  // namespace

extern "C" int nnhip_md_step(const float* pos_in, float* vel, const float* force, const float* hk, const float* mass,
                             const float* sigma, const float* noise, float dth, float c1, int32_t flags, int32_t n_atoms,
                             float* pos_out, float* ke_out, void* stream) {
  if (n_atoms < 0 || flags < 1 || flags > (NNHIP_MD_FINISH | NNHIP_MD_BEGIN)) {
    nnhip_set_error("nnhip_md_step: bad arguments (n_atoms %d, flags %d: bit 0 = finish, bit 1 = begin)", n_atoms, flags);
    return NNHIP_E_INVALID;
  }
  if ((sigma == nullptr) != (noise == nullptr)) {
    nnhip_set_error("nnhip_md_step: sigma and noise come together (both given or both null)");
    return NNHIP_E_INVALID;
  }
  if (n_atoms == 0) return NNHIP_OK;
  const bool begin = flags & NNHIP_MD_BEGIN;
  if (!vel || !force || !hk || (begin && (!pos_in || !pos_out)) || (ke_out && (!mass || !(flags & NNHIP_MD_FINISH)))) {
    nnhip_set_error("nnhip_md_step: bad arguments (vel, force and hk always; pos_in and pos_out with begin; ke_out needs mass and "
                    "finish)");
    return NNHIP_E_INVALID;
  }
  const size_t n3 = 3 * (size_t)n_atoms;
  if (begin && overlap(pos_in, pos_out, n3)) {
    nnhip_set_error("nnhip_md_step: pos_out may not alias pos_in (a forward call that has to be repeated reads pos_in again)");
    return NNHIP_E_INVALID;
  }
  MdArgs g;
  g.pos_in = pos_in;
  g.vel = vel;
  g.force = force;
  g.hk = hk;
  g.mass = mass;
  g.sigma = sigma;
  g.noise = noise;
  g.pos_out = pos_out;
  g.ke_out = ke_out;
  g.dth = dth;
  g.c1 = c1;
  g.flags = flags;
  g.n_atoms = n_atoms;
  int blocks = (n_atoms + MD_THREADS - 1) / MD_THREADS;
  blocks = blocks > MD_MAX_BLOCKS ? MD_MAX_BLOCKS : blocks;
  md_step_kernel<<<blocks, MD_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

extern "C" int nnhip_md_kinetic(const float* ke, const int32_t* mol_ptr, int32_t n_mol, float* out, void* stream) {
  if (n_mol < 0 || (n_mol > 0 && (!ke || !mol_ptr || !out))) {
    nnhip_set_error("nnhip_md_kinetic: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_mol == 0) return NNHIP_OK;
  const int waves = MD_THREADS / 64;
  int blocks = (n_mol + waves - 1) / waves;
  blocks = blocks > MD_MAX_BLOCKS ? MD_MAX_BLOCKS : blocks;
  md_kinetic_kernel<<<blocks, MD_THREADS, 0, (hipStream_t)stream>>>(ke, mol_ptr, n_mol, out);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
