// Molecular dynamics on the device (gfx950, fp32): one launch per MD step integrates every atom of a batch.
//
// The scheme is BAOAB (Leimkuhler & Matthews 2013) with the O step exact; with c1 = 1 and no noise it is velocity Verlet.  A step
// of the driver (newtonnet_amd/dynamics.py) is  model(pos) -> md_step(finish | begin):  the second half kick of the step whose
// forces have just been evaluated and the first half of the next step in one launch.  The per-atom chain and its rounding are
// written once, in csrc/md_chain.h:
//   finish (flag bit 0):  half_kick;  ke_i = kinetic                                   ke only when ke_out != NULL
//   begin  (flag bit 1):  begin<RESCALE>:  B [S] A [O] A                               O skipped entirely when noise == NULL
// md_step_kernel<false> is nnhip_md_step.  md_step_kernel<true> is nnhip_npt_step, the integrator of constant-pressure dynamics
// (newtonnet_amd/npt.py; the barostat that writes mu and inv_mu is in csrc/npt.hip): the same chain with S, the rescale
// x = mu_b * x_in, v = inv_mu_b * v  of the atom's system b = mol_of_atom[i], between the begin kick and the first half drift.  A
// product with 1.0f is exact: with every mu = inv_mu = 1 these are nnhip_md_step's bits.
// One thread per atom (its three coordinates: the kinetic energy needs them together); 256 threads per workgroup = four wave64s,
// at most 2048 workgroups, the rest by a grid-stride loop; the tail is the loop's bound.  The kernel moves 60-90 bytes per atom
// and is one launch of the ~45 of a step: nothing here is tuned.
//
// nnhip_md_kinetic sums ke [N] per molecule: one wave64 per molecule, lane l adds the atoms l, l + 64, ... of the molecule in that
// order, then the 64 partial sums meet in a fixed butterfly (__shfl_xor 32, 16, ..., 1).  No float atomics: bitwise repeatable, for
// thousands of small molecules (four per workgroup) as for one molecule of 100 000 atoms (1563 adds per lane).
#include "md_chain.h"

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
  const float* mu;                 // mu, inv_mu [n_mol] and mol_of_atom [n_atoms]: md_step_kernel<true> only
  const float* inv_mu;
  const int32_t* mol_of_atom;
  float* pos_out;
  float* ke_out;
  float dth, c1;
  int flags, n_atoms, n_mol;
};

template <bool RESCALE>
__global__ void __launch_bounds__(MD_THREADS)
md_step_kernel(MdArgs g) {
  const bool finish = g.flags & NNHIP_MD_FINISH, begin = g.flags & NNHIP_MD_BEGIN;
  for (int i = blockIdx.x * MD_THREADS + threadIdx.x; i < g.n_atoms; i += gridDim.x * MD_THREADS) {
    const size_t o = 3 * (size_t)i;
    int b = 0;
    if (RESCALE && begin) {
      b = g.mol_of_atom[i];
      if ((unsigned)b >= (unsigned)g.n_mol) continue;       // (an index outside the tables: the atom is left alone, nothing is read)
    }
    const float hk = g.hk[i];
    float v[3] = {g.vel[o], g.vel[o + 1], g.vel[o + 2]};
    const float f[3] = {g.force[o], g.force[o + 1], g.force[o + 2]};
    if (finish) {
      md_chain::half_kick(v, hk, f);
      if (g.ke_out) g.ke_out[i] = md_chain::kinetic(v, g.mass[i]);
    }
    if (begin) {
      const float sigma = g.noise ? g.sigma[i] : 0.f;
      const float* xi = g.noise ? g.noise + o : nullptr;
      const float mu = RESCALE ? g.mu[b] : 1.f, inv_mu = RESCALE ? g.inv_mu[b] : 1.f;
      md_chain::begin<RESCALE>(v, hk, f, g.pos_in + o, g.pos_out + o, g.dth, sigma, xi, g.c1, mu, inv_mu);
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

// the checks nnhip_md_step and nnhip_npt_step (`who`) share, and the launch
static int md_step_launch(const char* who, const MdArgs& g, bool rescale, void* stream) {
  if (g.n_atoms < 0 || g.flags < 1 || g.flags > (NNHIP_MD_FINISH | NNHIP_MD_BEGIN)) {
    nnhip_set_error("%s: bad arguments (n_atoms %d, flags %d: bit 0 = finish, bit 1 = begin)", who, g.n_atoms, g.flags);
    return NNHIP_E_INVALID;
  }
  if ((g.sigma == nullptr) != (g.noise == nullptr)) {
    nnhip_set_error("%s: sigma and noise come together (both given or both null)", who);
    return NNHIP_E_INVALID;
  }
  if (g.n_atoms == 0) return NNHIP_OK;
  const bool begin = g.flags & NNHIP_MD_BEGIN;
  if (!g.vel || !g.force || !g.hk || (begin && (!g.pos_in || !g.pos_out)) ||
      (g.ke_out && (!g.mass || !(g.flags & NNHIP_MD_FINISH)))) {
    nnhip_set_error("%s: bad arguments (vel, force and hk always; pos_in and pos_out with begin; ke_out needs mass and finish)", who);
    return NNHIP_E_INVALID;
  }
  if (begin && overlap(g.pos_in, g.pos_out, 3 * (size_t)g.n_atoms)) {
    nnhip_set_error("%s: pos_out may not alias pos_in (a forward call that has to be repeated reads pos_in again)", who);
    return NNHIP_E_INVALID;
  }
  int blocks = (g.n_atoms + MD_THREADS - 1) / MD_THREADS;
  blocks = blocks > MD_MAX_BLOCKS ? MD_MAX_BLOCKS : blocks;
  if (rescale)
    md_step_kernel<true><<<blocks, MD_THREADS, 0, (hipStream_t)stream>>>(g);
  else
    md_step_kernel<false><<<blocks, MD_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

}  // namespace

extern "C" int nnhip_md_step(const float* pos_in, float* vel, const float* force, const float* hk, const float* mass,
                             const float* sigma, const float* noise, float dth, float c1, int32_t flags, int32_t n_atoms,
                             float* pos_out, float* ke_out, void* stream) {
  const MdArgs g = {pos_in, vel, force, hk, mass, sigma, noise, nullptr, nullptr, nullptr, pos_out, ke_out, dth, c1, flags, n_atoms, 0};
  return md_step_launch("nnhip_md_step", g, false, stream);
}

extern "C" int nnhip_npt_step(const float* pos_in, float* vel, const float* force, const float* hk, const float* mass,
                              const float* sigma, const float* noise, const float* mu, const float* inv_mu,
                              const int32_t* mol_of_atom, int32_t n_mol, float dth, float c1, int32_t flags, int32_t n_atoms,
                              float* pos_out, float* ke_out, void* stream) {
  if (n_mol < 0 || (n_atoms > 0 && (flags & NNHIP_MD_BEGIN) && (!mu || !inv_mu || !mol_of_atom))) {
    nnhip_set_error("nnhip_npt_step: bad arguments (n_mol %d; mu, inv_mu and mol_of_atom with begin)", n_mol);
    return NNHIP_E_INVALID;
  }
  const MdArgs g = {pos_in, vel, force, hk, mass, sigma, noise, mu, inv_mu, mol_of_atom, pos_out, ke_out, dth, c1, flags, n_atoms, n_mol};
  return md_step_launch("nnhip_npt_step", g, true, stream);
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
