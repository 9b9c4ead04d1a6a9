// Nudged elastic band on the device (gfx950, fp32): one launch per optimisation step moves every band of a batch by one FIRE step
// on its NEB forces.  A band is a chain of images -- consecutive molecules of the batch, all of the same atom count -- between two
// endpoints that never move; the NEB force of an interior image is the true force without its component along the improved tangent
// (Henkelman and Jonsson 2000) plus the spring force along it, and the climbing image (Henkelman, Uberuaga and Jonsson 2000), once
// switched on, gets the true force with its tangent component reversed instead.  The optimiser is FIRE as ase.optimize.FIRE states
// it (mass 1, one step length for the whole band).  A step of the driver (newtonnet_amd/neb.py) is  model(pos) -> neb_step.
// include/newtonnet_hip.h spells the contract out.
//
// One workgroup of four waves per band; image j of the band belongs to wave j % 4 in EVERY sweep and atom l, l + 64, ... of an image
// to lane l of that wave, so a lane only ever re-reads rows it wrote itself (tangent_out, neb_force_out and vel are the kernel's
// working storage for its own rows).  A per-image sum is a lane-local sum in atom order, then the fixed butterfly __shfl_xor 32, 16,
// ..., 1 (a + b and b + a round alike: all 64 lanes hold the same bits).  A band-level sum or maximum goes through ONE LDS slot per
// image and is added by every thread in image order after a barrier: the bits of a band depend neither on the rest of the batch
// nor on how many waves served it.  No float atomics, no communication between workgroups.  Both barriers are reached by every
// thread of the workgroup: a band that is skipped or frozen skips the work between them, never the barrier.
//
// Every multiply-add is an explicit __fmaf_rn and every lone product / sum / quotient an explicit __fmul_rn / __fadd_rn / __fsub_rn
// / __fdiv_rn; tests/neb_ref.py restates the chain in fp64 with one 2^-24 per operation.  The chain, for one band (sum_l: the
// per-image reduction above; SUM_i: the LDS slots added in image order; dot3(a, b) = fma(az, bz, fma(ay, by, ax bx)); every vector
// of a fixed atom is exactly 0 and a fixed atom is in no sum):
//   interior image i:
//     tp = R_{i+1} - R_i;  tm = R_i - R_{i-1};  dEp = E_{i+1} - E_i;  dEm = E_{i-1} - E_i              (one rounding each)
//     E_{i+1} > E_i > E_{i-1}:  tau = tp;     E_{i+1} < E_i < E_{i-1}:  tau = tm;     otherwise, with a = max(|dEp|, |dEm|) and
//     b = min(|dEp|, |dEm|):  tau = fma(cp, tp, cm tm)  with (cp, cm) = (a, b) if E_{i+1} > E_{i-1} else (b, a)
//     tt = sum_l dot3(tau, tau);  nt = sqrt(tt);  that = tau / nt  (tt == 0: that = 0)                  -> tangent_out
//     lp = sqrt(sum_l dot3(tp, tp));  lm = sqrt(sum_l dot3(tm, tm));  fd = sum_l dot3(f, that)
//     c = spring (lp - lm) - fd      (the climbing image, when climbing[k] was set before the launch:  c = -2 fd)
//     F = fma(c, that, f)                                                                               -> neb_force_out
//     slots:  m_i = max_atoms dot3(F, F);  ff_i = sum_l dot3(F, F);  p_i = sum_l dot3(F, v);  vv_i = sum_l dot3(v, v)
//   band:  fmax2 = max_i m_i;  fmax_out = sqrt(fmax2);  FF, P, VV = SUM_i ff_i, p_i, vv_i     (v = 0 in the band's first step)
//   flags (not with CHECK_ONLY, not for a band converged before):  converged iff fmax2 < tol2 and (no CLIMB or climbing was set
//     before);  climbing |= CLIMB and fmax2 < climb2
//   FIRE (not frozen):  first step:  dt = dt_start, a = a_start, n_pos = 0, v = 0;  else
//     P > 0:   c1 = 1 - a;  c2 = (a sqrt(VV)) / sqrt(FF);  v = fma(c2, F, c1 v);  if n_pos > n_min: dt = min(dt f_inc, dt_max), a = a f_a;
//              n_pos += 1
//     P <= 0:  v = 0;  a = a_start;  dt = dt f_dec;  n_pos = 0
//     v = fma(dt, F, v)  -> vel;   dr = dt v;   DD = SUM_i sum_l dot3(dr, dr);  nd = sqrt(DD);  nd > maxstep:  dr = dr (maxstep / nd)
//     pos_out = pos_in + dr   (endpoints and fixed atoms: pos_in itself)
#include "common.h"
#include "optim_rows.h"

namespace {

constexpr int NEB_THREADS = 256;
constexpr int NEB_WAVES = NEB_THREADS / 64;

struct NebArgs {
  const float* pos_in;
  const float* force;
  const float* energy;
  const uint8_t* free_mask;
  const int32_t* mol_ptr;
  const int32_t* band_ptr;
  int32_t* converged;
  int32_t* climbing;
  int32_t* n_steps;
  int32_t* n_pos;
  float* dt;
  float* a;
  float* vel;
  float* pos_out;
  float* neb_force_out;
  float* tangent_out;
  float* fmax_out;
  int32_t* saddle_out;
  float spring, tol2, climb2, dt_start, dt_max, f_inc, f_dec, a_start, f_a, maxstep;
  int n_min, flags, n_bands, n_mol, n_atoms;
};

__global__ void __launch_bounds__(NEB_THREADS)
neb_step_kernel(NebArgs g) {
  __shared__ float s_max[NNHIP_NEB_MAX_IMAGES], s_ff[NNHIP_NEB_MAX_IMAGES], s_p[NNHIP_NEB_MAX_IMAGES], s_vv[NNHIP_NEB_MAX_IMAGES],
      s_dd[NNHIP_NEB_MAX_IMAGES];
  const int k = blockIdx.x;                              // the band (uniform over the workgroup, as is everything up to the sweeps)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = g.band_ptr[k], m1 = g.band_ptr[k + 1];
  const int n_img = m1 - m0;
  // ---- the band as every thread sees it: a band whose images differ in size, whose pointers leave the arrays or whose state words
  // no step can have left behind is not touched and gets fmax_out = NaN
  bool bad = m0 < 0 || m1 > g.n_mol || n_img < 3 || n_img > NNHIP_NEB_MAX_IMAGES;
  int n = 0;
  if (!bad) {
    n = g.mol_ptr[m0 + 1] - g.mol_ptr[m0];
    for (int j = 0; j < n_img; ++j) {
      const int a0 = g.mol_ptr[m0 + j], a1 = g.mol_ptr[m0 + j + 1];
      bad = bad || a0 < 0 || a1 > g.n_atoms || a1 - a0 != n || n < 0;
    }
  }
  const int steps = g.n_steps[k];
  const bool first = steps == 0;
  int n_pos = g.n_pos[k];
  float dt = g.dt[k], a = g.a[k];
  const bool was_conv = g.converged[k] != 0, was_climb = g.climbing[k] != 0;
  bad = bad || steps < 0 || (!first && (n_pos < 0 || !(dt > 0.f) || !(a > 0.f)));
  const bool check_only = (g.flags & NNHIP_NEB_CHECK_ONLY) != 0, climb_req = (g.flags & NNHIP_NEB_CLIMB) != 0;
  // the climbing image: the interior image of highest energy, the lowest index at a tie
  int top = 1;
  if (!bad) {
    float e_top = g.energy[m0 + 1];
    for (int j = 2; j < n_img - 1; ++j) {
      const float e = g.energy[m0 + j];
      if (e > e_top) e_top = e, top = j;
    }
  }
  // ---- sweep 1: tangents and NEB forces, image by image (a wave's own images)
  if (!bad) {
    for (int j = wave; j < n_img; j += NEB_WAVES) {
      const int a0 = g.mol_ptr[m0 + j], a1 = a0 + n;
      if (j == 0 || j == n_img - 1) {                    // an endpoint: no force, no tangent
        const float zero[3] = {0.f, 0.f, 0.f};
        for (int i = a0 + lane; i < a1; i += 64) {
          store3(g.neb_force_out, 3 * (size_t)i, zero);
          store3(g.tangent_out, 3 * (size_t)i, zero);
        }
        if (lane == 0) s_max[j] = s_ff[j] = s_p[j] = s_vv[j] = 0.f;
        continue;
      }
      const long up = 3 * ((long)g.mol_ptr[m0 + j + 1] - a0), down = 3 * ((long)g.mol_ptr[m0 + j - 1] - a0);
      const float e0 = g.energy[m0 + j], ep = g.energy[m0 + j + 1], em = g.energy[m0 + j - 1];
      float cp, cm;
      bool pure = true;
      if (ep > e0 && e0 > em) {
        cp = 1.f, cm = 0.f;
      } else if (ep < e0 && e0 < em) {
        cp = 0.f, cm = 1.f;
      } else {
        const float dp = fabsf(__fsub_rn(ep, e0)), dm = fabsf(__fsub_rn(em, e0));
        const float hi = fmaxf(dp, dm), lo = fminf(dp, dm);
        pure = false;
        if (ep > em) {
          cp = hi, cm = lo;
        } else {
          cp = lo, cm = hi;
        }
      }
      float tt = 0.f, sp = 0.f, sm = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        const size_t o = 3 * (size_t)i;
        float x[3], xp[3], xm[3], tp[3], tm[3], tau[3];
        load3(g.pos_in, o, x);
        load3(g.pos_in, o + up, xp);
        load3(g.pos_in, o + down, xm);
        const bool fr = is_free(g, i);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          tp[c] = fr ? __fsub_rn(xp[c], x[c]) : 0.f;
          tm[c] = fr ? __fsub_rn(x[c], xm[c]) : 0.f;
          tau[c] = pure ? (cp != 0.f ? tp[c] : tm[c]) : __fmaf_rn(cp, tp[c], __fmul_rn(cm, tm[c]));
        }
        store3(g.tangent_out, o, tau);
        tt = __fadd_rn(tt, dot3(tau, tau));
        sp = __fadd_rn(sp, dot3(tp, tp));
        sm = __fadd_rn(sm, dot3(tm, tm));
      }
      tt = bfly_sum(tt);
      sp = bfly_sum(sp);
      sm = bfly_sum(sm);
      const float nt = __fsqrt_rn(tt);
      float fd = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        const size_t o = 3 * (size_t)i;
        float tau[3], f[3];
        load3(g.tangent_out, o, tau);
        load3(g.force, o, f);
        const bool fr = is_free(g, i);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          tau[c] = tt > 0.f ? __fdiv_rn(tau[c], nt) : 0.f;
          f[c] = fr ? f[c] : 0.f;
        }
        store3(g.tangent_out, o, tau);
        fd = __fadd_rn(fd, dot3(f, tau));
      }
      fd = bfly_sum(fd);
      const float coef = (was_climb && j == top)
                             ? __fmul_rn(-2.f, fd)
                             : __fsub_rn(__fmul_rn(g.spring, __fsub_rn(__fsqrt_rn(sp), __fsqrt_rn(sm))), fd);
      float mx = 0.f, ff = 0.f, p = 0.f, vv = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        const size_t o = 3 * (size_t)i;
        float tau[3], f[3], F[3], v[3] = {0.f, 0.f, 0.f};
        load3(g.tangent_out, o, tau);
        load3(g.force, o, f);
        const bool fr = is_free(g, i);
        if (fr && !first) load3(g.vel, o, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) F[c] = fr ? __fmaf_rn(coef, tau[c], f[c]) : 0.f;
        store3(g.neb_force_out, o, F);
        const float F2 = dot3(F, F);
        mx = fmaxf(mx, F2);
        ff = __fadd_rn(ff, F2);
        p = __fadd_rn(p, dot3(F, v));
        vv = __fadd_rn(vv, dot3(v, v));
      }
      mx = bfly_max(mx);
      ff = bfly_sum(ff);
      p = bfly_sum(p);
      vv = bfly_sum(vv);
      if (lane == 0) s_max[j] = mx, s_ff[j] = ff, s_p[j] = p, s_vv[j] = vv;
    }
  }
  __syncthreads();
  // ---- the band's numbers, in every thread alike
  float fmax2 = 0.f, FF = 0.f, P = 0.f, VV = 0.f;
  if (!bad) {
    for (int j = 1; j < n_img - 1; ++j) {
      fmax2 = fmaxf(fmax2, s_max[j]);
      FF = __fadd_rn(FF, s_ff[j]);
      P = __fadd_rn(P, s_p[j]);
      VV = __fadd_rn(VV, s_vv[j]);
    }
  }
  const bool touch_flags = !bad && !check_only && !was_conv;
  const bool conv_now = touch_flags && fmax2 < g.tol2 && (!climb_req || was_climb);
  const bool climb_now = touch_flags && climb_req && fmax2 < g.climb2;
  const bool frozen = was_conv || conv_now || check_only;
  const bool move = !bad && !frozen;
  if (threadIdx.x == 0) {
    g.fmax_out[k] = bad ? __builtin_nanf("") : __fsqrt_rn(fmax2);
    if (!bad) g.saddle_out[k] = m0 + top;
    if (conv_now) g.converged[k] = 1;
    if (climb_now && !was_climb) g.climbing[k] = 1;
  }
  // ---- FIRE: the band's scalars
  float c1 = 0.f, c2 = 0.f;
  bool keep_v = false;
  if (move) {
    if (first) {
      dt = g.dt_start, a = g.a_start, n_pos = 0;
    } else if (P > 0.f) {
      keep_v = true;
      c1 = __fsub_rn(1.f, a);
      c2 = __fdiv_rn(__fmul_rn(a, __fsqrt_rn(VV)), __fsqrt_rn(FF));
      if (n_pos > g.n_min) {
        dt = fminf(__fmul_rn(dt, g.f_inc), g.dt_max);
        a = __fmul_rn(a, g.f_a);
      }
      n_pos += 1;
    } else {
      a = g.a_start, dt = __fmul_rn(dt, g.f_dec), n_pos = 0;
    }
  }
  // ---- sweep 2: velocities, and the squared length of the step
  if (move) {
    for (int j = wave; j < n_img; j += NEB_WAVES) {
      float dd = 0.f;
      if (j > 0 && j < n_img - 1) {
        const int a0 = g.mol_ptr[m0 + j], a1 = a0 + n;
        for (int i = a0 + lane; i < a1; i += 64) {
          if (!is_free(g, i)) continue;
          const size_t o = 3 * (size_t)i;
          float F[3], v[3] = {0.f, 0.f, 0.f}, dr[3];
          load3(g.neb_force_out, o, F);
          if (keep_v) load3(g.vel, o, v);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (keep_v) v[c] = __fmaf_rn(c2, F[c], __fmul_rn(c1, v[c]));
            v[c] = __fmaf_rn(dt, F[c], v[c]);
            dr[c] = __fmul_rn(dt, v[c]);
          }
          store3(g.vel, o, v);
          dd = __fadd_rn(dd, dot3(dr, dr));
        }
        dd = bfly_sum(dd);
      }
      if (lane == 0) s_dd[j] = dd;
    }
  }
  __syncthreads();
  if (bad) return;                                       // (after the last barrier)
  float scale = 1.f;
  bool clamp = false;
  if (move) {
    float DD = 0.f;
    for (int j = 1; j < n_img - 1; ++j) DD = __fadd_rn(DD, s_dd[j]);
    const float nd = __fsqrt_rn(DD);
    clamp = nd > g.maxstep;
    if (clamp) scale = __fdiv_rn(g.maxstep, nd);
  }
  // ---- sweep 3: positions
  for (int j = wave; j < n_img; j += NEB_WAVES) {
    const int a0 = g.mol_ptr[m0 + j], a1 = a0 + n;
    const bool moves = move && j > 0 && j < n_img - 1;
    for (int i = a0 + lane; i < a1; i += 64) {
      const size_t o = 3 * (size_t)i;
      float x[3];
      load3(g.pos_in, o, x);
      if (moves && is_free(g, i)) {
        float v[3];
        load3(g.vel, o, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float dr = __fmul_rn(dt, v[c]);
          if (clamp) dr = __fmul_rn(dr, scale);
          x[c] = __fadd_rn(x[c], dr);
        }
      }
      store3(g.pos_out, o, x);
    }
  }
  if (move && threadIdx.x == 0) {
    g.dt[k] = dt;
    g.a[k] = a;
    g.n_pos[k] = n_pos;
    g.n_steps[k] = steps + 1;
  }
}

}  // namespace

extern "C" int nnhip_neb_step(const float* pos_in, const float* force, const float* energy, const uint8_t* free_mask,
                              const int32_t* mol_ptr, const int32_t* band_ptr, const int32_t* band_ptr_host, int32_t n_bands,
                              int32_t n_mol, int32_t n_atoms, float spring, float tol2, float climb2, float dt_start, float dt_max,
                              int32_t n_min, float f_inc, float f_dec, float a_start, float f_a, float maxstep, int32_t flags,
                              int32_t* converged, int32_t* climbing, int32_t* n_steps, int32_t* n_pos, float* dt, float* a, float* vel,
                              float* pos_out, float* neb_force_out, float* tangent_out, float* fmax_out, int32_t* saddle_out,
                              void* stream) {
  if (n_bands < 0 || n_mol < 0 || n_atoms < 0 || n_min < 0 || (flags & ~(NNHIP_NEB_CHECK_ONLY | NNHIP_NEB_CLIMB))) {
    nnhip_set_error("nnhip_neb_step: bad arguments (n_bands %d, n_mol %d, n_atoms %d, n_min %d, flags %d: NNHIP_NEB_CHECK_ONLY | "
                    "NNHIP_NEB_CLIMB)", n_bands, n_mol, n_atoms, n_min, flags);
    return NNHIP_E_INVALID;
  }
  const float prm[] = {spring, tol2, climb2, dt_start, dt_max, f_inc, f_dec, a_start, f_a, maxstep};
  for (float p : prm) {
    if (!(p > 0.f)) {
      nnhip_set_error("nnhip_neb_step: spring, tol2, climb2, dt, dt_max, f_inc, f_dec, a_start, f_a and maxstep must all be > 0 "
                      "(got %g, %g, %g, %g, %g, %g, %g, %g, %g, %g)", (double)spring, (double)tol2, (double)climb2, (double)dt_start,
                      (double)dt_max, (double)f_inc, (double)f_dec, (double)a_start, (double)f_a, (double)maxstep);
      return NNHIP_E_INVALID;
    }
  }
  if (n_bands == 0) return NNHIP_OK;
  if (!mol_ptr || !band_ptr || !band_ptr_host || !energy || !converged || !climbing || !n_steps || !n_pos || !dt || !a || !fmax_out ||
      !saddle_out) {
    nnhip_set_error("nnhip_neb_step: null pointer (mol_ptr, band_ptr, band_ptr_host, energy, converged, climbing, n_steps, n_pos, dt, "
                    "a, fmax_out and saddle_out are mandatory)");
    return NNHIP_E_INVALID;
  }
  if (band_ptr_host[0] != 0 || band_ptr_host[n_bands] != n_mol) {
    nnhip_set_error("nnhip_neb_step: band_ptr must run from 0 to n_mol = %d (got %d .. %d)", n_mol, band_ptr_host[0],
                    band_ptr_host[n_bands]);
    return NNHIP_E_INVALID;
  }
  for (int k = 0; k < n_bands; ++k) {
    const long n_img = (long)band_ptr_host[k + 1] - band_ptr_host[k];
    if (n_img < 3 || n_img > NNHIP_NEB_MAX_IMAGES) {
      nnhip_set_error("nnhip_neb_step: band %d has %ld images (3 .. %d expected)", k, n_img, NNHIP_NEB_MAX_IMAGES);
      return NNHIP_E_INVALID;
    }
  }
  if (n_atoms > 0 && (!pos_in || !force || !vel || !pos_out || !neb_force_out || !tangent_out)) {
    nnhip_set_error("nnhip_neb_step: null pointer (pos_in, force, vel, pos_out, neb_force_out and tangent_out are mandatory)");
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && overlap(pos_in, pos_out, 3 * (size_t)n_atoms)) {
    nnhip_set_error("nnhip_neb_step: pos_out may not alias pos_in (a forward call that has to be repeated reads pos_in again)");
    return NNHIP_E_INVALID;
  }
  NebArgs g;
  g.pos_in = pos_in;
  g.force = force;
  g.energy = energy;
  g.free_mask = free_mask;
  g.mol_ptr = mol_ptr;
  g.band_ptr = band_ptr;
  g.converged = converged;
  g.climbing = climbing;
  g.n_steps = n_steps;
  g.n_pos = n_pos;
  g.dt = dt;
  g.a = a;
  g.vel = vel;
  g.pos_out = pos_out;
  g.neb_force_out = neb_force_out;
  g.tangent_out = tangent_out;
  g.fmax_out = fmax_out;
  g.saddle_out = saddle_out;
  g.spring = spring;
  g.tol2 = tol2;
  g.climb2 = climb2;
  g.dt_start = dt_start;
  g.dt_max = dt_max;
  g.f_inc = f_inc;
  g.f_dec = f_dec;
  g.a_start = a_start;
  g.f_a = f_a;
  g.maxstep = maxstep;
  g.n_min = n_min;
  g.flags = flags;
  g.n_bands = n_bands;
  g.n_mol = n_mol;
  g.n_atoms = n_atoms;
  neb_step_kernel<<<n_bands, NEB_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
