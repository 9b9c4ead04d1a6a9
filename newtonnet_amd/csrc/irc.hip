// Intrinsic-reaction-coordinate following on the device (gfx950, fp32): one launch per step moves every path of a batch by one
// step of the damped velocity Verlet scheme (after Hratchian & Schlegel, J. Phys. Chem. A 106, 165 (2002)): a trajectory whose
// speed is reset to the constant v0 after every step moves along M^-1 F, the steepest-descent direction in mass-weighted
// coordinates, and its time step follows an error estimate that costs no force evaluation.  include/newtonnet_hip.h spells the
// contract out.  A step of the driver (newtonnet_amd/irc.py) is  model(pos) -> irc_step.
//
// One wave64 per molecule, four molecules per workgroup (as relax.hip).  Lane l owns the atoms l, l + 64, ... of its molecule in
// EVERY sweep, so a lane only ever re-reads what it wrote itself: no barrier, no LDS.  Every per-molecule reduction is a lane-local
// sum (or max) in atom order, then the fixed butterfly __shfl_xor 32, 16, ..., 1, so all 64 lanes hold the same bits afterwards and
// every decision is uniform over the wave.  No float atomics: a molecule's result does not depend on the rest of the batch or on
// its place in it.
//
// Every multiply-add is an explicit __fmaf_rn and every lone product / sum / quotient an explicit __fmul_rn / __fadd_rn / __fsub_rn
// / __fdiv_rn; tests/irc_ref.py restates the chain in fp64 with one 2^-24 per operation (2 ulp for the roots).  The chain, for one
// molecule (sum_l: the reduction above over the FREE atoms; dot3(a, b) = fma(az, bz, fma(ay, by, ax bx)); c = NNHIP_IRC_ACCEL):
//   sweep 1  f_i = F_i (free) or 0 (fixed);  fmax2 = max_i dot3(f_i, f_i);  P = sum_l dot3(f_i, vel_i)             [n_steps >= 1]
//            a_i = (c f_i) / m_i;  w_i = fma(0.5 (a_prev_i + a_i), dt_prev, vel_i);  vv = sum_l dot3(w_i, w_i)      [n_steps >= 1]
//   damp     nv = sqrt(vv);  nv > 0:  v_i = w_i (v0 / nv);  nv == 0:  v_i = vel_i;      n_steps == 0:  v_i = vel_i
//   sweep 2  x1_i = fma(a_i, h, fma(v_i, dt, x_i)),  h = (0.5 dt) dt;   d_i = x1_i - x_i;  M = sum_l m_i dot3(d_i, d_i)
//            (a lane adds an atom to its M by fma(m_i, dot3(d_i, d_i), acc): one rounding)
//            T = dt_prev + dt;  g = (0.5 T) T;  p_i = fma(a_prev_i, g, fma(v_prev_i, T, x_prev_i));  e_i = x1_i - p_i;
//            D2 = sum_l dot3(e_i, e_i)                                                                               [n_steps >= 1]
//   scalars  arc += sqrt(M);  Delta = sqrt(D2);  Delta > 0:  dt_next = dt cbrt(Delta0 / Delta) clamped into [0.5 dt, 2 dt], then
//            into [dt_min, dt_max];  otherwise dt_next = dt
#include "common.h"
#include "optim_rows.h"

namespace {

constexpr int IRC_THREADS = 256;
constexpr int IRC_MAX_BLOCKS = 2048;

struct IrcArgs {
  const float* pos_in;
  const float* force;
  const uint8_t* free_mask;
  const float* masses;
  const int32_t* mol_ptr;
  int32_t* status;
  int32_t* armed;
  int32_t* n_steps;
  float* dt;
  float* dt_prev;
  float* arc;
  float* vel;
  float* x_prev;
  float* v_prev;
  float* a_prev;
  float* pos_out;
  float* fmax_out;
  float v0, delta0, dt_min, dt_max, tol2;
  int flags, n_mol, n_atoms;
};

// a = (c f) / m of a FREE atom from its force f and mass m and, when `finish`, w = the velocity before damping (else w = vel)
__device__ __forceinline__ void accel_and_velocity(const IrcArgs& g, size_t o, const float* f, float m, const float* vel,
                                                   bool finish, float dt_prev, float* a, float* w) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = __fdiv_rn(__fmul_rn(NNHIP_IRC_ACCEL, f[k]), m);
    w[k] = vel[k];
  }
  if (finish) {
    float ap[3];
    load3(g.a_prev, o, ap);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = __fmaf_rn(__fmul_rn(0.5f, __fadd_rn(ap[k], a[k])), dt_prev, vel[k]);
  }
}

__global__ void __launch_bounds__(IRC_THREADS)
irc_step_kernel(IrcArgs g) {
  const int lane = threadIdx.x & 63;
  const int waves = IRC_THREADS / 64;
  for (int b = blockIdx.x * waves + (threadIdx.x >> 6); b < g.n_mol; b += gridDim.x * waves) {   // (uniform over a wave)
    const int a0 = g.mol_ptr[b], a1 = g.mol_ptr[b + 1];
    const bool bad_ptr = a0 < 0 || a1 < a0 || a1 > g.n_atoms;
    const int status = g.status[b], steps = g.n_steps[b];
    const bool was_armed = g.armed[b] != 0;
    const float dt = g.dt[b], dt_prev = g.dt_prev[b], arc = g.arc[b];
    const bool finish = steps >= 1;
    // ---- sweep 1: the masked forces' maximum and, for a molecule that may move (running, no check-only launch), P = f.vel and
    // the squared norm of the velocity before damping
    const bool check_only = (g.flags & NNHIP_IRC_CHECK_ONLY) != 0;
    const bool may_move = status == 0 && !check_only;
    float f2 = 0.f, p_acc = 0.f, vv_acc = 0.f;
    bool bad_mass = false;
    for (int i = a0 + lane; i < a1 && !bad_ptr; i += 64) {
      if (!is_free(g, i)) continue;
      const float m = g.masses[i];
      if (!(m > 0.f) || m > 3.402823466e38f) {
        bad_mass = true;
        continue;
      }
      const size_t o = 3 * (size_t)i;
      float f[3];
      load3(g.force, o, f);
      f2 = fmaxf(f2, dot3(f, f));
      if (may_move && finish) {
        float v[3], a[3], w[3];
        load3(g.vel, o, v);
        p_acc = __fadd_rn(p_acc, dot3(f, v));
        accel_and_velocity(g, o, f, m, v, true, dt_prev, a, w);
        vv_acc = __fadd_rn(vv_acc, dot3(w, w));
      }
    }
    const float fmax2 = bfly_max(f2);
    const float P = bfly_sum(p_acc);
    const float vv = bfly_sum(vv_acc);
    // state words no step can have left behind, a mol_ptr that leaves the arrays or a free atom without a usable mass: the
    // molecule is not touched, fmax_out = NaN
    const bool bad = bad_ptr || __any(bad_mass) || status < 0 || status > 2 || steps < 0 || !(dt >= g.dt_min && dt <= g.dt_max);
    if (bad) {
      if (lane == 0) g.fmax_out[b] = __builtin_nanf("");
      continue;
    }
    const bool armed = was_armed || (status == 0 && fmax2 >= g.tol2);
    int now = 0;
    if (status == 0 && !check_only) {
      if (finish && P < 0.f) {
        now = 2;
      } else if (armed && fmax2 < g.tol2) {
        now = 1;
      }
    }
    if (lane == 0) {
      g.fmax_out[b] = __fsqrt_rn(fmax2);
      if (armed && !was_armed) g.armed[b] = 1;
      if (now) g.status[b] = now;
    }
    if (status != 0 || now || a1 == a0 || check_only) {
      for (int i = a0 + lane; i < a1; i += 64) {
        float x[3];
        load3(g.pos_in, 3 * (size_t)i, x);
        store3(g.pos_out, 3 * (size_t)i, x);
      }
      continue;
    }
    // ---- damping: the speed is reset to v0 (never dividing by a vanishing norm: the stored velocity stays then)
    const float nv = __fsqrt_rn(vv);
    const bool damp = finish && nv > 0.f;
    const float scale = damp ? __fdiv_rn(g.v0, nv) : 1.f;
    const float h = __fmul_rn(__fmul_rn(0.5f, dt), dt);
    const float T = __fadd_rn(dt_prev, dt);
    const float gT = __fmul_rn(__fmul_rn(0.5f, T), T);
    // ---- sweep 2: drift, arc length, error estimate, and the state of the next step
    float m_acc = 0.f, d_acc = 0.f;
    for (int i = a0 + lane; i < a1; i += 64) {
      const size_t o = 3 * (size_t)i;
      float x[3];
      load3(g.pos_in, o, x);
      if (!is_free(g, i)) {
        store3(g.pos_out, o, x);
        continue;
      }
      float f[3], vel[3], a[3], w[3], v[3], x1[3], d[3];
      const float m = g.masses[i];
      load3(g.force, o, f);
      load3(g.vel, o, vel);
      accel_and_velocity(g, o, f, m, vel, finish, dt_prev, a, w);
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = damp ? __fmul_rn(w[k], scale) : vel[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        x1[k] = __fmaf_rn(a[k], h, __fmaf_rn(v[k], dt, x[k]));
        d[k] = __fsub_rn(x1[k], x[k]);
      }
      m_acc = __fmaf_rn(m, dot3(d, d), m_acc);
      if (finish) {
        float xp[3], vp[3], ap[3], e[3];
        load3(g.x_prev, o, xp);
        load3(g.v_prev, o, vp);
        load3(g.a_prev, o, ap);
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = __fsub_rn(x1[k], __fmaf_rn(ap[k], gT, __fmaf_rn(vp[k], T, xp[k])));
        d_acc = __fadd_rn(d_acc, dot3(e, e));
      }
      store3(g.pos_out, o, x1);
      store3(g.x_prev, o, x);
      store3(g.vel, o, v);
      store3(g.v_prev, o, v);
      store3(g.a_prev, o, a);
    }
    const float ds = __fsqrt_rn(bfly_sum(m_acc));
    const float delta = __fsqrt_rn(bfly_sum(d_acc));
    float dt_next = dt;
    if (finish && delta > 0.f) {
      dt_next = __fmul_rn(dt, cbrtf(__fdiv_rn(g.delta0, delta)));
      dt_next = fminf(fmaxf(dt_next, __fmul_rn(0.5f, dt)), __fmul_rn(2.f, dt));
      dt_next = fminf(fmaxf(dt_next, g.dt_min), g.dt_max);
    }
    if (lane == 0) {
      g.arc[b] = __fadd_rn(arc, ds);
      g.dt_prev[b] = dt;
      g.dt[b] = dt_next;
      g.n_steps[b] = steps + 1;
    }
  }
}

}  // namespace

extern "C" int nnhip_irc_step(const float* pos_in, const float* force, const uint8_t* free_mask, const float* masses,
                              const int32_t* mol_ptr, int32_t n_mol, int32_t n_atoms, float v0, float delta0, float dt_min,
                              float dt_max, float tol2, int32_t flags, int32_t* status, int32_t* armed, int32_t* n_steps, float* dt,
                              float* dt_prev, float* arc, float* vel, float* x_prev, float* v_prev, float* a_prev, float* pos_out,
                              float* fmax_out, void* stream) {
  if (n_mol < 0 || n_atoms < 0 || (flags & ~NNHIP_IRC_CHECK_ONLY)) {
    nnhip_set_error("nnhip_irc_step: bad arguments (n_mol %d, n_atoms %d, flags %d: 0 or NNHIP_IRC_CHECK_ONLY)", n_mol, n_atoms,
                    flags);
    return NNHIP_E_INVALID;
  }
  if (!positive_finite(v0) || !positive_finite(delta0) || !positive_finite(dt_min) || !(dt_max >= dt_min) ||
      !positive_finite(dt_max) || !(tol2 >= 0.f)) {
    nnhip_set_error("nnhip_irc_step: finite v0 > 0, delta0 > 0, dt_min > 0, dt_max >= dt_min and tol2 >= 0 expected (got %g, %g, "
                    "%g, %g, %g)", (double)v0, (double)delta0, (double)dt_min, (double)dt_max, (double)tol2);
    return NNHIP_E_INVALID;
  }
  if (n_mol == 0) return NNHIP_OK;
  if (!mol_ptr || !status || !armed || !n_steps || !dt || !dt_prev || !arc || !fmax_out) {
    nnhip_set_error("nnhip_irc_step: null pointer (mol_ptr, status, armed, n_steps, dt, dt_prev, arc and fmax_out are mandatory)");
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && (!pos_in || !force || !masses || !vel || !x_prev || !v_prev || !a_prev || !pos_out)) {
    nnhip_set_error("nnhip_irc_step: null pointer (pos_in, force, masses, vel, x_prev, v_prev, a_prev and pos_out are mandatory)");
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && overlap(pos_in, pos_out, 3 * (size_t)n_atoms)) {
    nnhip_set_error("nnhip_irc_step: pos_out may not alias pos_in (a forward call that has to be repeated reads pos_in again)");
    return NNHIP_E_INVALID;
  }
  IrcArgs g;
  g.pos_in = pos_in;
  g.force = force;
  g.free_mask = free_mask;
  g.masses = masses;
  g.mol_ptr = mol_ptr;
  g.status = status;
  g.armed = armed;
  g.n_steps = n_steps;
  g.dt = dt;
  g.dt_prev = dt_prev;
  g.arc = arc;
  g.vel = vel;
  g.x_prev = x_prev;
  g.v_prev = v_prev;
  g.a_prev = a_prev;
  g.pos_out = pos_out;
  g.fmax_out = fmax_out;
  g.v0 = v0;
  g.delta0 = delta0;
  g.dt_min = dt_min;
  g.dt_max = dt_max;
  g.tol2 = tol2;
  g.flags = flags;
  g.n_mol = n_mol;
  g.n_atoms = n_atoms;
  const int waves = IRC_THREADS / 64;
  int blocks = (n_mol + waves - 1) / waves;
  blocks = blocks > IRC_MAX_BLOCKS ? IRC_MAX_BLOCKS : blocks;
  irc_step_kernel<<<blocks, IRC_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
