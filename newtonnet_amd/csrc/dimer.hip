// Dimer-method saddle search on the device (gfx950, fp32): one launch per force evaluation advances the dimer of every molecule of
// a batch by one move of its own state machine -- min-mode following after Henkelman & Jonsson (J. Chem. Phys. 111, 7010 (1999)),
// with the one-evaluation rotations of Heyden, Bell & Keil (J. Chem. Phys. 123, 224101 (2005)) and Kaestner & Sherwood (J. Chem.
// Phys. 128, 014106 (2008)): conjugate-gradient rotation directions, the rotated endpoint's force interpolated instead of evaluated,
// and an L-BFGS translation on the force with its component along the mode inverted.  include/newtonnet_hip.h spells the contract
// out.  A step of the driver (newtonnet_amd/dimer.py) is  model(probe) -> dimer_step; the probe of a molecule is its dimer's
// centre (phase 0), its endpoint centre + delta N (phase 1) or a trial endpoint centre + delta (c1 N + s1 Theta) (phase 2).
//
// One wave64 per molecule, four molecules per workgroup (as relax.hip).  Lane l owns the atoms l, l + 64, ... of its molecule in
// EVERY sweep, so a lane only ever re-reads what it wrote itself: no barrier, no LDS.  Every per-molecule reduction is a lane-local
// sum (or max) in atom order, then the fixed butterfly __shfl_xor 32, 16, ..., 1, so all 64 lanes hold the same bits afterwards and
// every decision is uniform over the wave.  No float atomics: a molecule's result does not depend on the rest of the batch or on
// its place in it.  Vectors live in the caller's rows (vstate), never in registers across sweeps: the register budget is that of one
// sweep, whatever the molecule's size.
//
// Every multiply-add is an explicit __fmaf_rn and every lone product / sum / quotient / root an explicit __fmul_rn / __fadd_rn /
// __fsub_rn / __fdiv_rn / __fsqrt_rn; no atan, sin or cos: the angles exist only as cosines and sines formed by roots and quotients.
// tests/dimer_ref.py restates the chain in fp64 with one 2^-24 per operation.  The chain, for one molecule (sum: the reduction above;
// dot3(a, b) = fma(az, bz, fma(ay, by, ax bx)); a fixed atom has f = 0 and reads as 0 in every vector):
//   always    f = F (free) or 0;  fmax2 = max_i dot3(f_i, f_i)
//   phase 0   F0 = f;  [first launch: center = pos_in]  fmax_out = sqrt(fmax2), energy_out = energy;
//             converged iff n_steps >= 1 and fmax2 < tol2 and C < 0;  else pos_out = fma(delta, N, center)
//   phase 1   F1 = f;  ASSESS
//   phase 2   c1 = sqrt(0.5 (1 + c2));  s1 = s2 / (2 c1);  n* = fma(s1, Theta, c1 N);  C* = (sum dot3(F0 - f, n*)) / delta
//             a1 = fma(b1, s2, C - C*) / (2 (s1 s1));  root = sqrt(fma(a1, a1, b1 b1));  cm2 = -a1 / root, sm2 = -b1 / root
//             (root == 0 or not finite: cm2 = 1, sm2 = 0)
//             cm2 >= 0:  cp = sqrt(0.5 (1 + cm2)), sp = sm2 / (2 cp);   else  sa = sqrt(0.5 (1 - cm2)), sp = copysign(sa, sm2),
//             cp = |sm2| / (2 sa)   (the root that does not cancel; the other from sin 2 phi = 2 sin phi cos phi)
//             k1 = (s1 cp - c1 sp) / s1;  k2 = sp / s1;  k0 = (1 - cp) - sp (s1 / (1 + c1))
//             F1 = fma(k0, F0, fma(k2, f, k1 F1));  theta_rot = fma(cp, Theta, (-sp) N);  n' = fma(sp, Theta, cp N);
//             N = n' / sqrt(sum dot3(n', n'));  ASSESS
//   ASSESS    g = F1 - F0;  gN = sum dot3(g, N);  C = (-gN) / delta;  G = fma(-gN, N, g)
//             after phase 2:  beta = max(0, (sum dot3(G, G - g_old)) / (sum dot3(g_old, g_old)))  (0 when the divisor is 0)
//                             D = fma(beta d_norm, theta_rot, G);  D = fma(-(sum dot3(D, N)), N, D);  D = G unless sum dot3(D, G) > 0
//             after phase 1:  D = G
//             d_norm = sqrt(sum dot3(D, D));  Theta = D / d_norm;  b1 = (-(sum dot3(g, Theta))) / delta;  r = (-b1) / |C|
//             t = fma(r, r, 1);  c2 = 1 / sqrt(t);  s2 = r c2   (C == 0 or t not finite: c2 = 0, s2 = 1, r = +inf)
//             rotation done iff d_norm == 0 or r < rot_tol or n_rot >= max_rotations:  TRANSLATE
//             else  g_old = G;  pos_out = fma(delta, n*, center) with c1, s1, n* as in phase 2
//   TRANSLATE p = sum dot3(F0, N);  Ft = fma(-2 p, N, F0) when C < 0, else (-p) N;  one step of lbfgs_chain.h on (center, Ft) --
//             with C >= 0 without history (n_pairs = 0, no pending pair), with C < 0 the pending pair only after a C < 0 step;
//             x_prev = the centre left, center = pos_out = the new one
#include "common.h"
#include "lbfgs_chain.h"

namespace {

constexpr int DM_THREADS = 256;
constexpr int DM_MAX_BLOCKS = 2048;

struct DimerArgs {
  const float* pos_in;
  const float* force;
  const float* energy;
  const uint8_t* free_mask;
  const int32_t* mol_ptr;
  int32_t* istate;
  float* fstate;
  float* vstate;
  float* S;
  float* Y;
  float* rho;
  float* work;
  float* pos_out;
  float* fmax_out;
  float* energy_out;
  float delta, rot_tol, tol2, alpha, maxstep;
  int max_rotations, flags, n_mol, n_atoms, memory;
};


__device__ __forceinline__ float* vec(const DimerArgs& g, int row) { return g.vstate + row * (3 * (size_t)g.n_atoms); }

// a state vector's row of atom i; a fixed atom reads as 0 whatever the row holds
__device__ __forceinline__ void loadv(const DimerArgs& g, int row, int i, float* v) {
  if (is_free(g, i)) {
    load3(vec(g, row), 3 * (size_t)i, v);
  } else {
    v[0] = v[1] = v[2] = 0.f;
  }
}

__device__ __forceinline__ void storev(const DimerArgs& g, int row, int i, const float* v) { store3(vec(g, row), 3 * (size_t)i, v); }

__device__ __forceinline__ void masked_force(const DimerArgs& g, int i, float* f) {
  if (is_free(g, i)) {
    load3(g.force, 3 * (size_t)i, f);
  } else {
    f[0] = f[1] = f[2] = 0.f;
  }
}

// cosine and sine of half the angle whose cosine and sine are c2, s2 >= 0:  c1 = sqrt(0.5 (1 + c2)),  s1 = s2 / (2 c1)
__device__ __forceinline__ void half_angle(float c2, float s2, float& c1, float& s1) {
  c1 = __fsqrt_rn(__fmul_rn(0.5f, __fadd_rn(1.f, c2)));
  s1 = __fdiv_rn(s2, __fmul_rn(2.f, c1));
}

// the trial direction of atom i:  fma(s1, Theta, c1 N)
__device__ __forceinline__ void trial_direction(const DimerArgs& g, int i, float c1, float s1, float* t) {
  float n[3], th[3];
  loadv(g, NNHIP_DIMER_V_MODE, i, n);
  loadv(g, NNHIP_DIMER_V_THETA, i, th);
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = __fmaf_rn(s1, th[k], __fmul_rn(c1, n[k]));
}

// pos_out = pos_in bitwise
__device__ __forceinline__ void copy_probe(const DimerArgs& g, int a0, int a1, int lane) {
  for (int i = a0 + lane; i < a1; i += 64) {
    float x[3];
    load3(g.pos_in, 3 * (size_t)i, x);
    store3(g.pos_out, 3 * (size_t)i, x);
  }
}

// pos_out = fma(delta, d, center) with d = N (trial == false) or the trial direction; a fixed atom: its centre row
__device__ __forceinline__ void write_endpoint(const DimerArgs& g, int a0, int a1, int lane, bool trial, float c1, float s1) {
  for (int i = a0 + lane; i < a1; i += 64) {
    float x[3], d[3], xo[3];
    load3(vec(g, NNHIP_DIMER_V_CENTER), 3 * (size_t)i, x);
    if (trial) {
      trial_direction(g, i, c1, s1, d);
    } else {
      loadv(g, NNHIP_DIMER_V_MODE, i, d);
    }
    const bool fr = is_free(g, i);
#pragma unroll
    for (int k = 0; k < 3; ++k) xo[k] = fr ? __fmaf_rn(g.delta, d[k], x[k]) : x[k];
    store3(g.pos_out, 3 * (size_t)i, xo);
  }
}

// the translation's view of the molecule (lbfgs_chain.h): the force F0 with its component along N inverted (C < 0) or that
// component alone, inverted (C >= 0); the step goes from the centre to the new centre, which is also the next probe
struct TranslatePolicy {
  const DimerArgs& g;
  float p;          // sum dot3(F0, N)
  bool concave;     // C < 0
  __device__ __forceinline__ void force(int i, float* f) const {
    float f0[3], n[3];
    if (!::is_free(g, i)) {
      f[0] = f[1] = f[2] = 0.f;
      return;
    }
    loadv(g, NNHIP_DIMER_V_F0, i, f0);
    loadv(g, NNHIP_DIMER_V_MODE, i, n);
    const float c = concave ? __fmul_rn(-2.f, p) : -p;
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = concave ? __fmaf_rn(c, n[k], f0[k]) : __fmul_rn(c, n[k]);
  }
  __device__ __forceinline__ bool is_free(int i) const { return ::is_free(g, i); }
  __device__ __forceinline__ void load_x(size_t o, float* x) const { load3(vec(g, NNHIP_DIMER_V_CENTER), o, x); }
  __device__ __forceinline__ void store_x(size_t o, const float* x_out, const float* x) const {
    store3(vec(g, NNHIP_DIMER_V_X_PREV), o, x);
    store3(vec(g, NNHIP_DIMER_V_CENTER), o, x_out);
    store3(g.pos_out, o, x_out);
  }
};

__global__ void __launch_bounds__(DM_THREADS)
dimer_step_kernel(DimerArgs g) {
  const int lane = threadIdx.x & 63;
  const int waves = DM_THREADS / 64;
  const int m = g.memory;
  const size_t B = (size_t)g.n_mol;
  const float inf = __builtin_inff();
  for (int b = blockIdx.x * waves + (threadIdx.x >> 6); b < g.n_mol; b += gridDim.x * waves) {   // (uniform over a wave)
    int32_t* I = g.istate + b;
    float* R = g.fstate + b;
    const int a0 = g.mol_ptr[b], a1 = g.mol_ptr[b + 1];
    const bool bad_ptr = a0 < 0 || a1 < a0 || a1 > g.n_atoms;
    const int status = I[NNHIP_DIMER_I_STATUS * B], phase = I[NNHIP_DIMER_I_PHASE * B], steps = I[NNHIP_DIMER_I_STEPS * B];
    const int evals = I[NNHIP_DIMER_I_EVALS * B], rot_total = I[NNHIP_DIMER_I_ROT_TOTAL * B];
    int n_rot = I[NNHIP_DIMER_I_ROT * B], np = I[NNHIP_DIMER_I_PAIRS * B], head = I[NNHIP_DIMER_I_HEAD * B];
    const int pending = I[NNHIP_DIMER_I_PENDING * B];
    float C = R[NNHIP_DIMER_F_CURVATURE * B];
    // state words no launch can have left behind (or a mol_ptr that leaves the arrays): the molecule is not touched, fmax_out = NaN
    const bool c_known = steps >= 1 || phase == 2;
    const bool bad = bad_ptr || status < 0 || status > 1 || phase < 0 || phase > 2 || steps < 0 || evals < 0 || n_rot < 0 ||
                     rot_total < 0 || np < 0 || np > m || head < 0 || head >= m || pending < 0 || pending > 1 ||
                     (evals == 0 && phase != 0) ||
                     (c_known && !(C >= -3.402823466e38f && C <= 3.402823466e38f));
    if (bad) {
      if (lane == 0) g.fmax_out[b] = __builtin_nanf("");
      continue;
    }
    float f2 = 0.f;
    for (int i = a0 + lane; i < a1; i += 64) {
      float f[3];
      masked_force(g, i, f);
      f2 = fmaxf(f2, dot3(f, f));
    }
    const float fmax2 = bfly_max(f2);
    const bool frozen = status != 0 || a1 == a0 || (g.flags & NNHIP_DIMER_CHECK_ONLY);
    if (phase == 0 && lane == 0) {                           // the probe is the centre: its fmax and energy
      g.fmax_out[b] = __fsqrt_rn(fmax2);
      if (g.energy && g.energy_out) g.energy_out[b] = g.energy[b];
    }
    if (frozen) {
      copy_probe(g, a0, a1, lane);
      continue;
    }
    if (lane == 0) I[NNHIP_DIMER_I_EVALS * B] = evals + 1;
    bool after_trial = false;
    if (phase == 0) {
      for (int i = a0 + lane; i < a1; i += 64) {
        float f[3];
        masked_force(g, i, f);
        storev(g, NNHIP_DIMER_V_F0, i, f);
        if (evals == 0) {
          float x[3];
          load3(g.pos_in, 3 * (size_t)i, x);
          storev(g, NNHIP_DIMER_V_CENTER, i, x);
        }
      }
      if (steps >= 1 && fmax2 < g.tol2 && C < 0.f) {
        if (lane == 0) I[NNHIP_DIMER_I_STATUS * B] = 1;
        copy_probe(g, a0, a1, lane);
        continue;
      }
      write_endpoint(g, a0, a1, lane, false, 0.f, 0.f);
      if (lane == 0) {
        I[NNHIP_DIMER_I_PHASE * B] = 1;
        I[NNHIP_DIMER_I_ROT * B] = 0;
      }
      continue;
    }
    if (phase == 1) {
      for (int i = a0 + lane; i < a1; i += 64) {
        float f[3];
        masked_force(g, i, f);
        storev(g, NNHIP_DIMER_V_F1, i, f);
      }
    } else {
      // ---- the trial endpoint's force: the fitted curvature's minimum in the (N, Theta) plane, F1 there by interpolation
      const float b1 = R[NNHIP_DIMER_F_SLOPE * B], c2 = R[NNHIP_DIMER_F_C2 * B], s2 = R[NNHIP_DIMER_F_S2 * B];
      float c1, s1;
      half_angle(c2, s2, c1, s1);
      float acc = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        float f[3], f0[3], t[3], d[3];
        masked_force(g, i, f);
        loadv(g, NNHIP_DIMER_V_F0, i, f0);
        trial_direction(g, i, c1, s1, t);
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = __fsub_rn(f0[k], f[k]);
        acc = __fadd_rn(acc, dot3(d, t));
      }
      const float Cs = __fdiv_rn(bfly_sum(acc), g.delta);
      const float a1c = __fdiv_rn(__fmaf_rn(b1, s2, __fsub_rn(C, Cs)), __fmul_rn(2.f, __fmul_rn(s1, s1)));   // 1 - c2 = 2 s1^2
      const float root = __fsqrt_rn(__fmaf_rn(a1c, a1c, __fmul_rn(b1, b1)));
      float cm2 = 1.f, sm2 = 0.f;
      if (root > 0.f && root <= 3.402823466e38f) {
        cm2 = __fdiv_rn(-a1c, root);
        sm2 = __fdiv_rn(-b1, root);
      }
      // the half angle: the root that does not cancel, the other from sin 2 phi = 2 sin phi cos phi
      float cp, sp;
      if (cm2 >= 0.f) {
        cp = __fsqrt_rn(__fmul_rn(0.5f, __fadd_rn(1.f, cm2)));
        sp = __fdiv_rn(sm2, __fmul_rn(2.f, cp));
      } else {
        const float sa = __fsqrt_rn(__fmul_rn(0.5f, __fsub_rn(1.f, cm2)));
        sp = copysignf(sa, sm2);
        cp = __fdiv_rn(fabsf(sm2), __fmul_rn(2.f, sa));
      }
      const float k1 = __fdiv_rn(__fsub_rn(__fmul_rn(s1, cp), __fmul_rn(c1, sp)), s1);
      const float k2 = __fdiv_rn(sp, s1);
      const float k0 = __fsub_rn(__fsub_rn(1.f, cp), __fmul_rn(sp, __fdiv_rn(s1, __fadd_rn(1.f, c1))));
      float nn = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        if (!is_free(g, i)) continue;
        float f[3], f0[3], f1[3], n[3], th[3], tr[3], nw[3];
        masked_force(g, i, f);
        loadv(g, NNHIP_DIMER_V_F0, i, f0);
        loadv(g, NNHIP_DIMER_V_F1, i, f1);
        loadv(g, NNHIP_DIMER_V_MODE, i, n);
        loadv(g, NNHIP_DIMER_V_THETA, i, th);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          f1[k] = __fmaf_rn(k0, f0[k], __fmaf_rn(k2, f[k], __fmul_rn(k1, f1[k])));
          tr[k] = __fmaf_rn(cp, th[k], __fmul_rn(-sp, n[k]));
          nw[k] = __fmaf_rn(sp, th[k], __fmul_rn(cp, n[k]));
        }
        nn = __fadd_rn(nn, dot3(nw, nw));
        storev(g, NNHIP_DIMER_V_F1, i, f1);
        storev(g, NNHIP_DIMER_V_THETA_ROT, i, tr);
        storev(g, NNHIP_DIMER_V_MODE, i, nw);
      }
      const float norm = __fsqrt_rn(bfly_sum(nn));
      if (norm > 0.f) {
        for (int i = a0 + lane; i < a1; i += 64) {
          if (!is_free(g, i)) continue;
          float n[3];
          loadv(g, NNHIP_DIMER_V_MODE, i, n);
#pragma unroll
          for (int k = 0; k < 3; ++k) n[k] = __fdiv_rn(n[k], norm);
          storev(g, NNHIP_DIMER_V_MODE, i, n);
        }
      }
      n_rot += 1;
      if (lane == 0) {
        I[NNHIP_DIMER_I_ROT * B] = n_rot;
        I[NNHIP_DIMER_I_ROT_TOTAL * B] = rot_total + 1;
      }
      after_trial = true;
    }
    // ---- ASSESS: curvature along N, the rotation direction Theta, the trial angle
    float acc = 0.f;
    for (int i = a0 + lane; i < a1; i += 64) {
      float f0[3], f1[3], n[3], gg[3];
      loadv(g, NNHIP_DIMER_V_F0, i, f0);
      loadv(g, NNHIP_DIMER_V_F1, i, f1);
      loadv(g, NNHIP_DIMER_V_MODE, i, n);
#pragma unroll
      for (int k = 0; k < 3; ++k) gg[k] = __fsub_rn(f1[k], f0[k]);
      acc = __fadd_rn(acc, dot3(gg, n));
    }
    const float gN = bfly_sum(acc);
    C = __fdiv_rn(-gN, g.delta);
    // G of atom i from the stored rows: fma(-gN, N, F1 - F0)
    auto perp = [&](int i, float* gg, float* G) {
      float f0[3], f1[3], n[3];
      loadv(g, NNHIP_DIMER_V_F0, i, f0);
      loadv(g, NNHIP_DIMER_V_F1, i, f1);
      loadv(g, NNHIP_DIMER_V_MODE, i, n);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        gg[k] = __fsub_rn(f1[k], f0[k]);
        G[k] = __fmaf_rn(-gN, n[k], gg[k]);
      }
    };
    bool plain = !after_trial;                               // D = G
    float dd = 0.f;
    if (after_trial) {
      float num = 0.f, den = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        float gg[3], G[3], go[3], d[3];
        perp(i, gg, G);
        loadv(g, NNHIP_DIMER_V_G_OLD, i, go);
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = __fsub_rn(G[k], go[k]);
        num = __fadd_rn(num, dot3(G, d));
        den = __fadd_rn(den, dot3(go, go));
      }
      num = bfly_sum(num);
      den = bfly_sum(den);
      const float beta = den > 0.f ? fmaxf(0.f, __fdiv_rn(num, den)) : 0.f;
      const float bd = __fmul_rn(beta, R[NNHIP_DIMER_F_DNORM * B]);
      float dn = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        if (!is_free(g, i)) continue;
        float gg[3], G[3], tr[3], n[3], D[3];
        perp(i, gg, G);
        loadv(g, NNHIP_DIMER_V_THETA_ROT, i, tr);
        loadv(g, NNHIP_DIMER_V_MODE, i, n);
#pragma unroll
        for (int k = 0; k < 3; ++k) D[k] = __fmaf_rn(bd, tr[k], G[k]);
        dn = __fadd_rn(dn, dot3(D, n));
        storev(g, NNHIP_DIMER_V_THETA, i, D);
      }
      dn = bfly_sum(dn);
      float dg = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        if (!is_free(g, i)) continue;
        float gg[3], G[3], n[3], D[3];
        perp(i, gg, G);
        loadv(g, NNHIP_DIMER_V_THETA, i, D);
        loadv(g, NNHIP_DIMER_V_MODE, i, n);
#pragma unroll
        for (int k = 0; k < 3; ++k) D[k] = __fmaf_rn(-dn, n[k], D[k]);
        dg = __fadd_rn(dg, dot3(D, G));
        dd = __fadd_rn(dd, dot3(D, D));
        storev(g, NNHIP_DIMER_V_THETA, i, D);
      }
      dg = bfly_sum(dg);
      plain = !(dg > 0.f);
    }
    if (plain) {
      dd = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        if (!is_free(g, i)) continue;
        float gg[3], G[3];
        perp(i, gg, G);
        dd = __fadd_rn(dd, dot3(G, G));
        storev(g, NNHIP_DIMER_V_THETA, i, G);
      }
    }
    const float d_norm = __fsqrt_rn(bfly_sum(dd));
    float b1 = 0.f, r = 0.f, c2 = 1.f, s2 = 0.f;
    if (d_norm > 0.f) {
      float gt = 0.f;
      for (int i = a0 + lane; i < a1; i += 64) {
        if (!is_free(g, i)) continue;
        float gg[3], G[3], th[3];
        perp(i, gg, G);
        loadv(g, NNHIP_DIMER_V_THETA, i, th);
#pragma unroll
        for (int k = 0; k < 3; ++k) th[k] = __fdiv_rn(th[k], d_norm);
        gt = __fadd_rn(gt, dot3(gg, th));
        storev(g, NNHIP_DIMER_V_THETA, i, th);
      }
      b1 = __fdiv_rn(-bfly_sum(gt), g.delta);
      r = __fdiv_rn(-b1, fabsf(C));
      const float t = __fmaf_rn(r, r, 1.f);
      if (C == 0.f || !(t <= 3.402823466e38f)) {
        c2 = 0.f, s2 = 1.f, r = inf;
      } else {
        c2 = __fdiv_rn(1.f, __fsqrt_rn(t));
        s2 = __fmul_rn(r, c2);
      }
    }
    if (lane == 0) {
      R[NNHIP_DIMER_F_CURVATURE * B] = C;
      R[NNHIP_DIMER_F_SLOPE * B] = b1;
      R[NNHIP_DIMER_F_C2 * B] = c2;
      R[NNHIP_DIMER_F_S2 * B] = s2;
      R[NNHIP_DIMER_F_DNORM * B] = d_norm;
    }
    const bool done = !(d_norm > 0.f) || r < g.rot_tol || n_rot >= g.max_rotations;
    if (!done) {
      for (int i = a0 + lane; i < a1; i += 64) {
        if (!is_free(g, i)) continue;
        float gg[3], G[3];
        perp(i, gg, G);
        storev(g, NNHIP_DIMER_V_G_OLD, i, G);
      }
      float c1, s1;
      half_angle(c2, s2, c1, s1);
      write_endpoint(g, a0, a1, lane, true, c1, s1);
      if (lane == 0) I[NNHIP_DIMER_I_PHASE * B] = 2;
      continue;
    }
    // ---- TRANSLATE
    float pa = 0.f;
    for (int i = a0 + lane; i < a1; i += 64) {
      float f0[3], n[3];
      loadv(g, NNHIP_DIMER_V_F0, i, f0);
      loadv(g, NNHIP_DIMER_V_MODE, i, n);
      pa = __fadd_rn(pa, dot3(f0, n));
    }
    // The history holds curvature pairs of CONCAVE translations alone.  While C >= 0 the force -p N is no gradient of anything: it
    // has rank one and turns with N, so the difference of two of them says how N rotated, not how the surface curves, and a pair
    // made of it (|s| tiny, y all rotation, cos(y, s) just above the acceptance threshold) sends the next step to the maxstep cap
    // in a direction without meaning.  A convex translation is therefore the plain step F+ / alpha, drops the history and leaves
    // no pending pair
    const bool concave = C < 0.f;
    if (!concave) np = 0;
    const TranslatePolicy policy{g, bfly_sum(pa), concave};
    lbfgs_chain::History h;
    h.S = g.S, h.Y = g.Y, h.rho = g.rho, h.f_prev = vec(g, NNHIP_DIMER_V_F_PREV), h.work = g.work;
    h.alpha = g.alpha, h.maxstep = g.maxstep, h.memory = m, h.n_atoms = g.n_atoms;
    lbfgs_chain::WaveTeam team{lane};
    lbfgs_chain::step(h, policy, team, b, a0, a1, concave && pending != 0, np, head);
    if (lane == 0) {
      I[NNHIP_DIMER_I_PENDING * B] = concave ? 1 : 0;
      I[NNHIP_DIMER_I_STEPS * B] = steps + 1;
      I[NNHIP_DIMER_I_PAIRS * B] = np;
      I[NNHIP_DIMER_I_HEAD * B] = head;
      I[NNHIP_DIMER_I_PHASE * B] = 0;
    }
  }
}

}  // namespace

extern "C" int nnhip_dimer_step(const float* pos_in, const float* force, const float* energy, const uint8_t* free_mask,
                                const int32_t* mol_ptr, int32_t n_mol, int32_t n_atoms, int32_t memory, float delta, float rot_tol,
                                int32_t max_rotations, float tol2, float alpha, float maxstep, int32_t flags, int32_t* istate,
                                float* fstate, float* vstate, float* S, float* Y, float* rho, float* work, float* pos_out,
                                float* fmax_out, float* energy_out, void* stream) {
  if (n_mol < 0 || n_atoms < 0 || memory < 1 || memory > NNHIP_LBFGS_MAX_MEMORY || (flags & ~NNHIP_DIMER_CHECK_ONLY) ||
      max_rotations < 0) {
    nnhip_set_error("nnhip_dimer_step: bad arguments (n_mol %d, n_atoms %d, memory %d: 1 .. %d, max_rotations %d: >= 0, flags %d: "
                    "0 or NNHIP_DIMER_CHECK_ONLY)", n_mol, n_atoms, memory, NNHIP_LBFGS_MAX_MEMORY, max_rotations, flags);
    return NNHIP_E_INVALID;
  }
  if (!positive_finite(delta) || !positive_finite(rot_tol) || !(tol2 >= 0.f) || !positive_finite(alpha) ||
      !positive_finite(maxstep)) {
    nnhip_set_error("nnhip_dimer_step: finite delta > 0, rot_tol > 0, alpha > 0, maxstep > 0 and tol2 >= 0 expected (got %g, %g, "
                    "%g, %g, %g)", (double)delta, (double)rot_tol, (double)alpha, (double)maxstep, (double)tol2);
    return NNHIP_E_INVALID;
  }
  if (n_mol == 0) return NNHIP_OK;
  if (!mol_ptr || !istate || !fstate || !rho || !fmax_out) {
    nnhip_set_error("nnhip_dimer_step: null pointer (mol_ptr, istate, fstate, rho and fmax_out are mandatory)");
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && (!pos_in || !force || !vstate || !S || !Y || !pos_out || (n_atoms > 64 && !work))) {
    nnhip_set_error("nnhip_dimer_step: null pointer (pos_in, force, vstate, S, Y and pos_out are mandatory; work [N,3] when "
                    "n_atoms > 64)");
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && overlap(pos_in, pos_out, 3 * (size_t)n_atoms)) {
    nnhip_set_error("nnhip_dimer_step: pos_out may not alias pos_in (a forward call that has to be repeated reads pos_in again)");
    return NNHIP_E_INVALID;
  }
  DimerArgs g;
  g.pos_in = pos_in;
  g.force = force;
  g.energy = energy;
  g.free_mask = free_mask;
  g.mol_ptr = mol_ptr;
  g.istate = istate;
  g.fstate = fstate;
  g.vstate = vstate;
  g.S = S;
  g.Y = Y;
  g.rho = rho;
  g.work = work;
  g.pos_out = pos_out;
  g.fmax_out = fmax_out;
  g.energy_out = energy_out;
  g.delta = delta;
  g.rot_tol = rot_tol;
  g.tol2 = tol2;
  g.alpha = alpha;
  g.maxstep = maxstep;
  g.max_rotations = max_rotations;
  g.flags = flags;
  g.n_mol = n_mol;
  g.n_atoms = n_atoms;
  g.memory = memory;
  const int waves = DM_THREADS / 64;
  int blocks = (n_mol + waves - 1) / waves;
  blocks = blocks > DM_MAX_BLOCKS ? DM_MAX_BLOCKS : blocks;
  dimer_step_kernel<<<blocks, DM_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
