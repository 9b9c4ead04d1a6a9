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
// molecules, not for one large system (tools/bench_relax.py reports what that costs).  For that use there is a second kernel,
// lbfgs_step_wg_kernel (nnhip_lbfgs_step_wg): one workgroup of NNHIP_LBFGS_WG_THREADS threads per system, the same text
// (relax_system below, and the chain of lbfgs_chain.h) instantiated with lbfgs_chain::BlockTeam, which states the method and the
// rules; tools/bench_relax_large.py compares the two.
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
  int wg_min_atoms;      // systems of at least this many atoms belong to lbfgs_step_wg_kernel (<= 0: all)
};


// the optimiser's view of this launch (lbfgs_chain.h): the model's forces, masked; the step goes from pos_in to pos_out
struct RelaxPolicy {
  const RelaxArgs& g;
  __device__ __forceinline__ void force(int i, float* f) const {
    load3(g.force, 3 * (size_t)i, f);
    if (g.free_mask && !g.free_mask[i]) f[0] = f[1] = f[2] = 0.f;
  }
  __device__ __forceinline__ bool is_free(int i) const { return ::is_free(g, i); }
  __device__ __forceinline__ void load_x(size_t o, float* x) const { load3(g.pos_in, o, x); }
  __device__ __forceinline__ void store_x(size_t o, const float* x_out, const float*) const { store3(g.pos_out, o, x_out); }
};

// one system of a launch, by the team that owns it: fmax and the convergence flag, the frozen copy, or the chain's step.  Every
// branch below is taken on values all members of the team loaded from the same address, or on a reduced value (the reductions of
// BlockTeam hold barriers).  The state words are loaded BEFORE the first reduction: member 0 stores them after it (converged) or
// after the reductions of the step (n_steps, n_pairs, head), so no member can read a word of this launch back
template <class Team>
__device__ __forceinline__ void relax_system(const RelaxArgs& g, const RelaxPolicy& policy, Team& team, int b, int a0, int a1,
                                             bool bad_ptr) {
  const int m = g.memory;
  const int steps = g.n_steps[b];
  int np = g.n_pairs[b], head = g.head[b];
  const bool was = g.converged[b] != 0;
  float f2 = 0.f;
  for (int i = a0 + team.first(); i < a1 && !bad_ptr; i += Team::STRIDE) {
    float f[3];
    policy.force(i, f);
    f2 = fmaxf(f2, dot3(f, f));
  }
  const float fmax2 = team.max(f2);
  // state words no step can have left behind (or a mol_ptr that leaves the arrays): the molecule is not touched, fmax_out = NaN
  const bool bad = bad_ptr || steps < 0 || np < 0 || np > m || head < 0 || head >= m;
  const bool now = !bad && (a1 == a0 || fmax2 < g.tol2);
  if (team.first() == 0) {
    g.fmax_out[b] = bad ? __builtin_nanf("") : __fsqrt_rn(fmax2);
    if (now && !was) g.converged[b] = 1;
  }
  if (bad) return;
  if (was || now || (g.flags & NNHIP_LBFGS_CHECK_ONLY)) {
    for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
      float x[3];
      load3(g.pos_in, 3 * (size_t)i, x);
      store3(g.pos_out, 3 * (size_t)i, x);
    }
    return;
  }
  lbfgs_chain::History h;
  h.S = g.S, h.Y = g.Y, h.rho = g.rho, h.f_prev = g.f_prev, h.work = g.work;
  h.alpha = g.alpha, h.maxstep = g.maxstep, h.memory = m, h.n_atoms = g.n_atoms;
  lbfgs_chain::step(h, policy, team, b, a0, a1, steps > 0, np, head);     // the pending pair, the two-loop, the step
  if (team.first() == 0) {
    g.n_steps[b] = steps + 1;
    g.n_pairs[b] = np;
    g.head[b] = head;
  }
}

__global__ void __launch_bounds__(RX_THREADS)
lbfgs_step_kernel(RelaxArgs g) {
  const int waves = RX_THREADS / 64;
  const RelaxPolicy policy{g};
  lbfgs_chain::WaveTeam team{(int)(threadIdx.x & 63)};
  for (int b = blockIdx.x * waves + (threadIdx.x >> 6); b < g.n_mol; b += gridDim.x * waves) {   // (uniform over a wave)
    const int a0 = g.mol_ptr[b], a1 = g.mol_ptr[b + 1];
    const bool bad_ptr = a0 < 0 || a1 < a0 || a1 > g.n_atoms;
    if (!lbfgs_chain::wave_owns(g.wg_min_atoms, a0, a1, bad_ptr)) continue;
    relax_system(g, policy, team, b, a0, a1, bad_ptr);
  }
}

// The workgroup-per-system form: one workgroup of NNHIP_LBFGS_WG_THREADS threads per system, grid-stride over the systems
// (lbfgs_chain.h: BlockTeam has the method, the barrier argument and the rules).  The `continue` below is uniform over the
// workgroup (mol_ptr[b], mol_ptr[b + 1] and the arguments are the same loads in every thread), and so is every return of
// relax_system.  A system larger than one workgroup serves fast is still served by one workgroup
__global__ void __launch_bounds__(NNHIP_LBFGS_WG_THREADS)
lbfgs_step_wg_kernel(RelaxArgs g) {
  __shared__ float red[lbfgs_chain::BlockTeam::RED_FLOATS];
  __shared__ float rows[lbfgs_chain::BlockTeam::ROW_FLOATS];
  const RelaxPolicy policy{g};
  lbfgs_chain::BlockTeam team{red, rows, (int)threadIdx.x, 0};
  for (int b = blockIdx.x; b < g.n_mol; b += gridDim.x) {
    const int a0 = g.mol_ptr[b], a1 = g.mol_ptr[b + 1];
    const bool bad_ptr = a0 < 0 || a1 < a0 || a1 > g.n_atoms;
    if (lbfgs_chain::wave_owns(g.wg_min_atoms, a0, a1, bad_ptr)) continue;
    relax_system(g, policy, team, b, a0, a1, bad_ptr);
  }
}

}  // namespace

// the checks and the launches of both entry points.  wave: launch lbfgs_step_kernel; wg: launch lbfgs_step_wg_kernel
static int lbfgs_step_launch(const char* who, const float* pos_in, const float* force, const uint8_t* free_mask,
                             const int32_t* mol_ptr, int32_t n_mol, int32_t n_atoms, int32_t memory, float tol2, float alpha,
                             float maxstep, int32_t wg_min_atoms, bool wave, bool wg, int32_t flags, int32_t* converged,
                             int32_t* n_steps, int32_t* n_pairs, int32_t* head, float* S, float* Y, float* rho, float* f_prev,
                             float* work, float* pos_out, float* fmax_out, void* stream) {
  if (n_mol < 0 || n_atoms < 0 || memory < 1 || memory > NNHIP_LBFGS_MAX_MEMORY || (flags & ~NNHIP_LBFGS_CHECK_ONLY)) {
    nnhip_set_error("%s: bad arguments (n_mol %d, n_atoms %d, memory %d: 1 .. %d, flags %d: 0 or "
                    "NNHIP_LBFGS_CHECK_ONLY)", who, n_mol, n_atoms, memory, NNHIP_LBFGS_MAX_MEMORY, flags);
    return NNHIP_E_INVALID;
  }
  if (!(tol2 >= 0.f) || !(alpha > 0.f) || !(maxstep > 0.f)) {
    nnhip_set_error("%s: tol2 >= 0, alpha > 0 and maxstep > 0 expected (got %g, %g, %g)", who, (double)tol2,
                    (double)alpha, (double)maxstep);
    return NNHIP_E_INVALID;
  }
  if (n_mol == 0) return NNHIP_OK;
  if (!mol_ptr || !converged || !n_steps || !n_pairs || !head || !rho || !fmax_out) {
    nnhip_set_error("%s: null pointer (mol_ptr, converged, n_steps, n_pairs, head, rho and fmax_out are mandatory)", who);
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && (!pos_in || !force || !S || !Y || !f_prev || !pos_out || (n_atoms > 64 && !work))) {
    nnhip_set_error("%s: null pointer (pos_in, force, S, Y, f_prev and pos_out are mandatory; work [N,3] when "
                    "n_atoms > 64)", who);
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && overlap(pos_in, pos_out, 3 * (size_t)n_atoms)) {
    nnhip_set_error("%s: pos_out may not alias pos_in (a forward call that has to be repeated reads pos_in again)", who);
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
  g.wg_min_atoms = wg_min_atoms;
  if (wave) {
    const int waves = RX_THREADS / 64;
    int blocks = (n_mol + waves - 1) / waves;
    blocks = blocks > RX_MAX_BLOCKS ? RX_MAX_BLOCKS : blocks;
    lbfgs_step_kernel<<<blocks, RX_THREADS, 0, (hipStream_t)stream>>>(g);
    LAUNCH_CHECK();
  }
  if (wg) {
    const int blocks = n_mol > RX_MAX_BLOCKS ? RX_MAX_BLOCKS : n_mol;
    lbfgs_step_wg_kernel<<<blocks, NNHIP_LBFGS_WG_THREADS, 0, (hipStream_t)stream>>>(g);
    LAUNCH_CHECK();
  }
  return NNHIP_OK;
}

extern "C" int nnhip_lbfgs_step(const float* pos_in, const float* force, const uint8_t* free_mask, const int32_t* mol_ptr,
                                int32_t n_mol, int32_t n_atoms, int32_t memory, float tol2, float alpha, float maxstep,
                                int32_t flags, int32_t* converged, int32_t* n_steps, int32_t* n_pairs, int32_t* head, float* S,
                                float* Y, float* rho, float* f_prev, float* work, float* pos_out, float* fmax_out, void* stream) {
  // (a threshold no system reaches: the wave kernel takes every system)
  return lbfgs_step_launch("nnhip_lbfgs_step", pos_in, force, free_mask, mol_ptr, n_mol, n_atoms, memory, tol2, alpha, maxstep,
                           0x7fffffff, true, false, flags, converged, n_steps, n_pairs, head, S, Y, rho, f_prev, work, pos_out,
                           fmax_out, stream);
}

extern "C" int nnhip_lbfgs_step_wg(const float* pos_in, const float* force, const uint8_t* free_mask, const int32_t* mol_ptr,
                                   int32_t n_mol, int32_t n_atoms, int32_t memory, float tol2, float alpha, float maxstep,
                                   int32_t wg_min_atoms, int32_t flags, int32_t* converged, int32_t* n_steps, int32_t* n_pairs,
                                   int32_t* head, float* S, float* Y, float* rho, float* f_prev, float* work, float* pos_out,
                                   float* fmax_out, void* stream) {
  return lbfgs_step_launch("nnhip_lbfgs_step_wg", pos_in, force, free_mask, mol_ptr, n_mol, n_atoms, memory, tol2, alpha, maxstep,
                           wg_min_atoms, wg_min_atoms > 0, true, flags, converged, n_steps, n_pairs, head, S, Y, rho, f_prev, work,
                           pos_out, fmax_out, stream);
}
