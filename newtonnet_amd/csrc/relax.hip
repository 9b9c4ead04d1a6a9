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
// 2^-24 per operation.  The device code of pair, loops and step is in lbfgs_chain.h, shared with dimer.hip.
// The chain, for one molecule (sum_l: the reduction above; dot3(a, b) = fma(az, bz, fma(ay, by, ax bx))):
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
#include "lbfgs_chain.h"

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

using lbfgs_chain::dot3;
using lbfgs_chain::load3;
using lbfgs_chain::store3;
using lbfgs_chain::wave_max;

// the optimiser's view of this launch (lbfgs_chain.h): the model's forces, masked; the step goes from pos_in to pos_out
struct RelaxPolicy {
  const RelaxArgs& g;
  __device__ __forceinline__ void force(int i, float* f) const {
    load3(g.force, 3 * (size_t)i, f);
    if (g.free_mask && !g.free_mask[i]) f[0] = f[1] = f[2] = 0.f;
  }
  __device__ __forceinline__ bool is_free(int i) const { return !g.free_mask || g.free_mask[i]; }
  __device__ __forceinline__ void load_x(size_t o, float* x) const { load3(g.pos_in, o, x); }
  __device__ __forceinline__ void store_x(size_t o, const float* x_out, const float*) const { store3(g.pos_out, o, x_out); }
};

__global__ void __launch_bounds__(RX_THREADS)
lbfgs_step_kernel(RelaxArgs g) {
  const int lane = threadIdx.x & 63;
  const int waves = RX_THREADS / 64;
  const int m = g.memory;
  const RelaxPolicy policy{g};
  for (int b = blockIdx.x * waves + (threadIdx.x >> 6); b < g.n_mol; b += gridDim.x * waves) {   // (uniform over a wave)
    const int a0 = g.mol_ptr[b], a1 = g.mol_ptr[b + 1];
    const bool bad_ptr = a0 < 0 || a1 < a0 || a1 > g.n_atoms;
    float f2 = 0.f;
    for (int i = a0 + lane; i < a1 && !bad_ptr; i += 64) {
      float f[3];
      policy.force(i, f);
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
    lbfgs_chain::History h;
    h.S = g.S, h.Y = g.Y, h.rho = g.rho, h.f_prev = g.f_prev, h.work = g.work;
    h.alpha = g.alpha, h.maxstep = g.maxstep, h.memory = m, h.n_atoms = g.n_atoms;
    lbfgs_chain::step(h, policy, b, a0, a1, lane, steps > 0, np, head);     // the pending pair, the two-loop, the step
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
