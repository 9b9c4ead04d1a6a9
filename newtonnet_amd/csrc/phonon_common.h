// The pieces the two phonon solvers share: csrc/phonon.hip (one workgroup or one wave per (crystal, q) problem, everything in LDS)
// and csrc/phonon_large.hip (block Jacobi over many workgroups, D(q) in HBM / L2).  Both call the SAME device functions for the
// phase weight of a pair, for the Hermitian element and for the in-LDS complex cyclic Jacobi, so the arithmetic of an element of
// D(q) and the rules of the iteration (tolerances, summation orders, rotation formulas) exist once: where both forms serve a
// crystal its D(q) is bitwise the same.  See the head of phonon.hip for the method.
#pragma once
#include "eig_common.h"   // rr_pair, EIG_EPS2, EIG_MAX_SWEEPS: one statement of the ordering and of the stopping rule

#define PH_THREADS 256

namespace {

template <bool ONE_WAVE>
__device__ __forceinline__ void ph_sync() {
  if (ONE_WAVE) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the wave's LDS writes are done and not moved across
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// 1 / sqrt(m) of home atom `a` (fp64): the mass factor of an element is the fp64 product of two of these, rounded once
__device__ __forceinline__ double ph_rsm(const float* masses, int a) { return 1.0 / sqrt((double)(masses ? masses[a] : 1.f)); }

// w(i, J) = (1 / m_iJ) sum_T exp(2 pi i q_frac . x) of the pair whose images are rows ist[ij] .. ist[ij + 1] - 1 of img_off: the
// product q_frac . x formed in fp64, reduced to [-1/2, 1/2] and handed to sincospi, the mean taken in fp64 and rounded once
__device__ __forceinline__ float2 ph_weight(const int* ist, const double* img_off, size_t ij, double q0, double q1, double q2) {
  const int k0 = ist[ij], k1 = ist[ij + 1];
  double sr = 0.0, si = 0.0;
  for (int k = k0; k < k1; ++k) {
    double ph = q0 * img_off[3 * (size_t)k] + q1 * img_off[3 * (size_t)k + 1] + q2 * img_off[3 * (size_t)k + 2];
    ph -= rint(ph);   // [-1/2, 1/2]
    double s, c;
    sincospi(2.0 * ph, &s, &c);
    sr += c;
    si += s;
  }
  const double inv = k1 > k0 ? 1.0 / (double)(k1 - k0) : 0.0;
  return make_float2((float)(sr * inv), (float)(si * inv));
}

// dw_a(i, J) = (1 / m_iJ) sum_T (i r_a) exp(2 pi i q_frac . x), a = x, y, z: the weights of d D / d q_cart (csrc/phonon_velocity.hip).
// The phase is that of ph_weight (the same fp64 product, the same reduction, the same sincospi); r = x @ cell (cell [3][3], the
// primitive lattice vectors as rows, A) in fp64; the mean in fp64, every component rounded once.
__device__ __forceinline__ void ph_dweight(const int* ist, const double* img_off, size_t ij, double q0, double q1, double q2,
                                           const double* cell, float2* dw) {
  const int k0 = ist[ij], k1 = ist[ij + 1];
  double sr[3] = {0.0, 0.0, 0.0}, si[3] = {0.0, 0.0, 0.0};
  for (int k = k0; k < k1; ++k) {
    const double x0 = img_off[3 * (size_t)k], x1 = img_off[3 * (size_t)k + 1], x2 = img_off[3 * (size_t)k + 2];
    double ph = q0 * x0 + q1 * x1 + q2 * x2;
    ph -= rint(ph);   // [-1/2, 1/2]
    double s, c;
    sincospi(2.0 * ph, &s, &c);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double r = x0 * cell[a] + x1 * cell[3 + a] + x2 * cell[6 + a];
      sr[a] -= r * s;   // i r (c + i s) = -r s + i r c
      si[a] += r * c;
    }
  }
  const double inv = k1 > k0 ? 1.0 / (double)(k1 - k0) : 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) dw[a] = make_float2((float)(sr[a] * inv), (float)(si[a] * inv));
}

// the sum over the copies R0 .. R0 + rc - 1 of one element: f points at Phi(i a, (R0, j) b), consecutive copies n atoms apart;
// w(r) at wch[r * w_stride]
__device__ __forceinline__ void ph_accumulate(const float* f, int n, const float2* wch, int w_stride, int rc, float& are, float& aim) {
  for (int r = 0; r < rc; ++r) {
    const float phi = f[(size_t)r * n * 3];
    const float2 w = wch[r * w_stride];
    are = fmaf(phi, w.x, are);
    aim = fmaf(phi, w.y, aim);
  }
}

// (D_ac + conj(D_ca)) / 2 / sqrt(m_a m_c) from the two sums; f = (float)(rsm_a rsm_c); a diagonal element is real
__device__ __forceinline__ void ph_hermitian(float re_ac, float im_ac, float re_ca, float im_ca, float f, bool diagonal, float& re,
                                             float& im) {
  re = 0.5f * (re_ac + re_ca) * f;
  im = diagonal ? 0.f : 0.5f * (im_ac - im_ca) * f;
}

// Step 2 of the method on (Are, Aim)[Mp][ld] in LDS (Mp even, P = Mp / 2 pairs) with T = 64 (ONE_WAVE) or PH_THREADS threads, thread
// index t: W <- I when wanted, then sweeps of the round-robin cyclic Jacobi until off^2 <= eps2 ||A||_F^2 or max_sweeps are done.
// rowo / rowd [Mp] fp64, cst [P] float4, dlt [P] and tab (the tiles k <= l of P pairs as k | l << 8, row by row) are LDS scratch.
// Returns the sweeps used; A's diagonal holds the eigenvalues, row k of W = U^T the vector of A[k][k].
template <bool ONE_WAVE>
__device__ __forceinline__ int ph_jacobi(float* Are, float* Aim, float* Wre, float* Wim, int Mp, int ld, double* rowo, double* rowd,
                                         float4* cst, float* dlt, const unsigned short* tab, bool want_v, double eps2, int max_sweeps,
                                         int t, bool& converged) {
  constexpr int T = ONE_WAVE ? 64 : PH_THREADS;
  const int P = Mp >> 1;
  if (want_v) {
    for (int e = t; e < Mp * Mp; e += T) {
      const int i = e / Mp, j = e - i * Mp;
      Wre[i * ld + j] = i == j ? 1.f : 0.f;
      Wim[i * ld + j] = 0.f;
    }
  }
  const int n_tiles = P * (P + 1) / 2;
  int n_sweeps = 0;
  converged = false;
  for (;;) {
    for (int i = t; i < Mp; i += T) {
      double o = 0.0, dd = 0.0;
      for (int j = 0; j < Mp; ++j) {
        const double re = (double)Are[i * ld + j], im = (double)Aim[i * ld + j];
        const double v = re * re + im * im;
        if (i == j) dd += v; else o += v;
      }
      rowo[i] = o;
      rowd[i] = dd;
    }
    ph_sync<ONE_WAVE>();
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < Mp; ++i) {
      off += rowo[i];
      diag += rowd[i];
    }
    converged = off <= eps2 * (off + diag) && off + diag <= 1.7976931348623157e308;
    if (converged || n_sweeps == max_sweeps) break;   // (uniform: every thread holds the same sums)
    for (int s = 0; s < Mp - 1; ++s) {
      for (int k = t; k < P; k += T) {
        int p, q;
        rr_pair(k, s, Mp, p, q);
        const float ar = Are[p * ld + q], ai = Aim[p * ld + q];
        const float ab = hypotf(ar, ai);
        float c = 1.f, sn = 0.f, ur = 1.f, ui = 0.f, dl = 0.f;
        if (ab != 0.f) {
          // |u| = 1 is what keeps W unitary.  A coupling that has converged into the denormal range (a pair that settles sweeps
          // before the matrix does, as in a graded spectrum) has too few bits left for its modulus to normalise it: scale it
          // up first (exact).  tau below takes the modulus as it is.
          float sr = ar, si = ai, sb = ab;
          if (ab < 0x1p-100f) {
            sr = ar * 0x1p64f;
            si = ai * 0x1p64f;
            sb = hypotf(sr, si);
          }
          ur = sr / sb;
          ui = si / sb;
          const float tau = (Are[q * ld + q] - Are[p * ld + p]) / (2.f * ab);
          const float tn = copysignf(1.f, tau) / (fabsf(tau) + sqrtf(1.f + tau * tau));   // (tau^2 = inf: t = 0, the identity)
          c = 1.f / sqrtf(1.f + tn * tn);
          sn = tn * c;
          dl = tn * ab;
        }
        cst[k] = make_float4(c, sn, ur, ui);
        dlt[k] = dl;
      }
      ph_sync<ONE_WAVE>();
      for (int e = t; e < n_tiles; e += T) {
        const int kl = tab[e];
        const int k = kl & 255, l = kl >> 8;
        int pk, qk, pl, ql;
        rr_pair(k, s, Mp, pk, qk);
        const float4 rk = cst[k];
        if (k == l) {
          const float dl = dlt[k];
          Are[pk * ld + pk] -= dl;
          Are[qk * ld + qk] += dl;
          Are[pk * ld + qk] = 0.f;
          Aim[pk * ld + qk] = 0.f;
          Are[qk * ld + pk] = 0.f;
          Aim[qk * ld + pk] = 0.f;
          continue;
        }
        rr_pair(l, s, Mp, pl, ql);
        const float4 rl = cst[l];
        const float b00r = Are[pk * ld + pl], b00i = Aim[pk * ld + pl], b01r = Are[pk * ld + ql], b01i = Aim[pk * ld + ql];
        float b10r = Are[qk * ld + pl], b10i = Aim[qk * ld + pl], b11r = Are[qk * ld + ql], b11i = Aim[qk * ld + ql];
        // rows q_k times u_k
        float xr = rk.z * b10r - rk.w * b10i, xi = rk.z * b10i + rk.w * b10r;
        b10r = xr;
        b10i = xi;
        xr = rk.z * b11r - rk.w * b11i;
        xi = rk.z * b11i + rk.w * b11r;
        b11r = xr;
        b11i = xi;
        // the real rotation of pair k on the rows
        const float r00r = rk.x * b00r - rk.y * b10r, r00i = rk.x * b00i - rk.y * b10i;
        const float r10r = rk.y * b00r + rk.x * b10r, r10i = rk.y * b00i + rk.x * b10i;
        float r01r = rk.x * b01r - rk.y * b11r, r01i = rk.x * b01i - rk.y * b11i;
        float r11r = rk.y * b01r + rk.x * b11r, r11i = rk.y * b01i + rk.x * b11i;
        // columns q_l times conj(u_l)
        xr = rl.z * r01r + rl.w * r01i;
        xi = rl.z * r01i - rl.w * r01r;
        r01r = xr;
        r01i = xi;
        xr = rl.z * r11r + rl.w * r11i;
        xi = rl.z * r11i - rl.w * r11r;
        r11r = xr;
        r11i = xi;
        // the real rotation of pair l on the columns
        const float n00r = rl.x * r00r - rl.y * r01r, n00i = rl.x * r00i - rl.y * r01i;
        const float n01r = rl.y * r00r + rl.x * r01r, n01i = rl.y * r00i + rl.x * r01i;
        const float n10r = rl.x * r10r - rl.y * r11r, n10i = rl.x * r10i - rl.y * r11i;
        const float n11r = rl.y * r10r + rl.x * r11r, n11i = rl.y * r10i + rl.x * r11i;
        Are[pk * ld + pl] = n00r;
        Aim[pk * ld + pl] = n00i;
        Are[pl * ld + pk] = n00r;
        Aim[pl * ld + pk] = -n00i;
        Are[pk * ld + ql] = n01r;
        Aim[pk * ld + ql] = n01i;
        Are[ql * ld + pk] = n01r;
        Aim[ql * ld + pk] = -n01i;
        Are[qk * ld + pl] = n10r;
        Aim[qk * ld + pl] = n10i;
        Are[pl * ld + qk] = n10r;
        Aim[pl * ld + qk] = -n10i;
        Are[qk * ld + ql] = n11r;
        Aim[qk * ld + ql] = n11i;
        Are[ql * ld + qk] = n11r;
        Aim[ql * ld + qk] = -n11i;
      }
      if (want_v) {
        for (int e = t; e < P * Mp; e += T) {
          const int k = e / Mp, j = e - k * Mp;
          int pk, qk;
          rr_pair(k, s, Mp, pk, qk);
          const float4 rk = cst[k];
          const float vpr = Wre[pk * ld + j], vpi = Wim[pk * ld + j];
          const float wr = Wre[qk * ld + j], wi = Wim[qk * ld + j];
          const float vqr = rk.z * wr + rk.w * wi, vqi = rk.z * wi - rk.w * wr;   // row q_k times conj(u_k)
          Wre[pk * ld + j] = rk.x * vpr - rk.y * vqr;
          Wim[pk * ld + j] = rk.x * vpi - rk.y * vqi;
          Wre[qk * ld + j] = rk.y * vpr + rk.x * vqr;
          Wim[qk * ld + j] = rk.y * vpi + rk.x * vqi;
        }
      }
      ph_sync<ONE_WAVE>();
    }
    ++n_sweeps;
  }
  return n_sweeps;
}

// the phase factor that makes the component of largest magnitude of row (wre, wim)[M] real and positive (lowest index on a tie)
__device__ __forceinline__ float2 ph_phase(const float* wre, const float* wim, int M) {
  float best = -1.f, fr = 1.f, fi = 0.f;
  for (int j = 0; j < M; ++j) {
    const float vr = wre[j], vi = wim[j];
    const float a2 = vr * vr + vi * vi;
    if (a2 > best) {
      best = a2;
      fr = vr;
      fi = vi;
    }
  }
  const float ab = hypotf(fr, fi);
  return ab > 0.f ? make_float2(fr / ab, -fi / ab) : make_float2(1.f, 0.f);
}

}  // namespace
