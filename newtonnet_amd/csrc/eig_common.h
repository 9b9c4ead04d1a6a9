// The pieces the two normal-mode solvers share: csrc/eig.hip (one workgroup per molecule, everything in LDS) and
// csrc/eig_large.hip (block Jacobi over many workgroups, the matrix in HBM / L2).  Both call the SAME device functions for the
// load / mass-weighting / projection and for the in-LDS cyclic Jacobi, so the rules (tolerances, summation orders, rotation
// formulas) exist once.  A and the fp64 scratch are plain pointers: LDS in eig.hip, the workspace in eig_large.hip's prepare
// kernel.  See the head of eig.hip for the method.
#pragma once
#include "common.h"

#define EIG_THREADS 256
#define EIG_MAX_DIM 126        // largest M = 3 n_b served (42 atoms): A and V^T in LDS take 2 x 126 x 127 x 4 = 128 016 bytes of 160 KiB
#define EIG_MAX_SWEEPS 30
#define EIG_DROP_TOL 1e-5      // Gram-Schmidt: a vector whose remainder is not above this fraction of its norm is dropped
#define EIG_EPS2 3.552713678800501e-15   // (2^-24)^2: the stopping rule off(A)^2 <= EIG_EPS2 ||A||_F^2

namespace {

struct EigArgs {
  const float* blocks;
  const int64_t* blk_ptr;
  const int* mol_ptr;
  const float* pos;
  const float* cell;
  const float* masses;
  float* evals;
  float* modes;
  int* n_proj;
  int* sweeps;
  int* status;
  int n_mol, project, mp_max;
};

// the partner indices of pair k at step s of the round-robin on n = 2 P players (n even): p < q
__device__ __forceinline__ void rr_pair(int k, int s, int n, int& p, int& q) {
  const int m = n - 1;
  int a, b;
  if (k == 0) {
    a = m;
    b = s;
  } else {
    a = s + k;
    if (a >= m) a -= m;
    b = s - k;
    if (b < 0) b += m;
  }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// sum of one double per thread in a fixed order (tree over red[EIG_THREADS]); every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();   // (red may still be read from the previous call)
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = EIG_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  return red[0];
}

// the tiles k <= l of P pairs as k | l << 8, row by row: tab[P (P + 1) / 2]
__device__ __forceinline__ void eig_fill_tab(unsigned short* tab, int P) {
  for (int e = threadIdx.x; e < P * P; e += EIG_THREADS) {
    const int k = e / P, l = e - k * P;
    if (k <= l) tab[k * P - k * (k - 1) / 2 + (l - k)] = (unsigned short)(k | l << 8);
  }
}

// Steps 1 and 2 of the method for molecule b (atoms a0 .. a0 + nb - 1, M = 3 nb <= Mp): A[Mp][ld] <- the symmetrised, mass-weighted
// and (g.project) projected block, rows and columns M .. Mp - 1 exactly zero; n_proj[b] written.  rsm[nb], D / U [6][ds] and G[36] are
// fp64 scratch, red[EIG_THREADS] is in LDS.  Returns false, with nothing of A decided, when a mass is not positive and finite (uniform
// over the workgroup).  Ends behind a barrier.
__device__ __forceinline__ bool eig_load_project(const EigArgs& g, int b, int a0, int nb, int Mp, float* A, int ld, double* rsm,
                                                 double* D, double* U, double* G, int ds, double* red) {
  const int t = threadIdx.x;
  const int M = 3 * nb;
  // ---- 1. load, symmetrise, mass-weight -------------------------------------------------------------------------------
  const float* H = g.blocks + g.blk_ptr[b];
  int bad_mass = 0;
  for (int i = t; i < nb; i += EIG_THREADS) {
    const float m = g.masses ? g.masses[a0 + i] : 1.f;
    bad_mass |= !(m > 0.f && m <= 3.4e38f);   // zero, negative, infinite or NaN
    rsm[i] = 1.0 / sqrt((double)m);
  }
  if (__syncthreads_or(bad_mass)) return false;   // (uniform) nothing of this molecule is computed
  for (int e = t; e < Mp * Mp; e += EIG_THREADS) {
    const int i = e / Mp, j = e - i * Mp;
    A[i * ld + j] = i < M && j < M ? H[(size_t)i * M + j] : 0.f;
  }
  __syncthreads();
  for (int e = t; e < M * M; e += EIG_THREADS) {
    const int i = e / M, j = e - i * M;
    if (i > j) continue;   // the thread of (i, j), i <= j, writes both halves: A is exactly symmetric from here on
    const float v = (float)(0.5 * ((double)A[i * ld + j] + (double)A[j * ld + i]) * rsm[i / 3] * rsm[j / 3]);
    A[i * ld + j] = v;
    A[j * ld + i] = v;
  }
  __syncthreads();

  // ---- 2. projection ----------------------------------------------------------------------------------------------------
  int n_kept = 0;
  if (g.project) {
    bool periodic = false;
    for (int c = 0; c < 9; ++c) periodic |= g.cell[9 * (size_t)b + c] != 0.f;
    // centre of mass (fp64, fixed order)
    double sm = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    if (!periodic) {
      for (int i = t; i < nb; i += EIG_THREADS) {
        const double m = g.masses ? (double)g.masses[a0 + i] : 1.0;
        sm += m;
        sx += m * (double)g.pos[3 * (size_t)(a0 + i)];
        sy += m * (double)g.pos[3 * (size_t)(a0 + i) + 1];
        sz += m * (double)g.pos[3 * (size_t)(a0 + i) + 2];
      }
      sm = block_sum(sm, red);
      sx = block_sum(sx, red) / sm;
      sy = block_sum(sy, red) / sm;
      sz = block_sum(sz, red) / sm;
    }
    const int n_cand = periodic ? 3 : 6;
    for (int k = 0; k < n_cand; ++k) {
      double* d = D + n_kept * ds;
      // candidate k: translation along k (k < 3) or rotation about axis k - 3, in mass-weighted coordinates
      double n0 = 0.0;
      for (int e = t; e < M; e += EIG_THREADS) {
        const int i = e / 3, c = e - 3 * i;
        const double sq = 1.0 / rsm[i];
        double v;
        if (k < 3) {
          v = c == k ? sq : 0.0;
        } else {
          const double r[3] = {(double)g.pos[3 * (size_t)(a0 + i)] - sx, (double)g.pos[3 * (size_t)(a0 + i) + 1] - sy,
                               (double)g.pos[3 * (size_t)(a0 + i) + 2] - sz};
          const int ax = k - 3;   // (e_ax x r)_c
          const int c1 = (ax + 1) % 3, c2 = (ax + 2) % 3;
          v = c == c2 ? r[c1] : c == c1 ? -r[c2] : 0.0;
          v *= sq;
        }
        d[e] = v;
        n0 += v * v;
      }
      n0 = sqrt(block_sum(n0, red));
      for (int j = 0; j < n_kept; ++j) {   // modified Gram-Schmidt against the vectors kept so far
        const double* dj = D + j * ds;
        double dot = 0.0;
        for (int e = t; e < M; e += EIG_THREADS) dot += dj[e] * d[e];
        dot = block_sum(dot, red);
        for (int e = t; e < M; e += EIG_THREADS) d[e] -= dot * dj[e];
      }
      double rem = 0.0;
      for (int e = t; e < M; e += EIG_THREADS) rem += d[e] * d[e];
      rem = sqrt(block_sum(rem, red));
      if (!(rem > EIG_DROP_TOL * n0)) continue;   // (uniform: every thread holds the same sums)
      for (int e = t; e < M; e += EIG_THREADS) d[e] /= rem;
      ++n_kept;
      __syncthreads();
    }
    if (n_kept > 0) {
      // W = A D
      for (int e = t; e < n_kept * M; e += EIG_THREADS) {
        const int k = e / M, i = e - k * M;
        const double* d = D + k * ds;
        double w = 0.0;
        for (int j = 0; j < M; ++j) w += (double)A[i * ld + j] * d[j];
        U[k * ds + i] = w;
      }
      __syncthreads();
      // G = D^T W
      if (t < n_kept * n_kept) {
        const int k = t / n_kept, l = t - k * n_kept;
        double s = 0.0;
        for (int i = 0; i < M; ++i) s += D[k * ds + i] * U[l * ds + i];
        G[k * 6 + l] = s;
      }
      __syncthreads();
      // U = W - D G / 2   (G symmetrised: A is)
      double u_new[6];
      for (int e = t; e < M; e += EIG_THREADS) {
        for (int k = 0; k < n_kept; ++k) {
          double s = U[k * ds + e];
          for (int l = 0; l < n_kept; ++l) s -= 0.25 * (G[l * 6 + k] + G[k * 6 + l]) * D[l * ds + e];
          u_new[k] = s;
        }
        for (int k = 0; k < n_kept; ++k) U[k * ds + e] = u_new[k];
      }
      __syncthreads();
      // A <- A - D U^T - U D^T
      for (int e = t; e < M * M; e += EIG_THREADS) {
        const int i = e / M, j = e - i * M;
        if (i > j) continue;
        double v = (double)A[i * ld + j];
        for (int k = 0; k < n_kept; ++k) v -= D[k * ds + i] * U[k * ds + j] + U[k * ds + i] * D[k * ds + j];
        A[i * ld + j] = (float)v;
        A[j * ld + i] = (float)v;
      }
      __syncthreads();
    }
    if (t == 0) g.n_proj[b] = n_kept;
  }
  return true;
}

// off(A)^2 and ||A||_F^2 - off(A)^2 of A[Mp][ld] summed in a fixed order -> the stopping rule off(A)^2 <= eps2 ||A||_F^2.  An Inf
// entry makes both sides +inf: without the second test it would pass as converged; a NaN fails the first.
__device__ __forceinline__ bool eig_converged(const float* A, int Mp, int ld, double eps2, double* red) {
  double off = 0.0, diag = 0.0;
  for (int e = threadIdx.x; e < Mp * Mp; e += EIG_THREADS) {
    const int i = e / Mp, j = e - i * Mp;
    const double a = (double)A[i * ld + j];
    if (i == j) diag += a * a; else off += a * a;
  }
  off = block_sum(off, red);
  diag = block_sum(diag, red);
  return off <= eps2 * (off + diag) && off + diag <= 1.7976931348623157e308;
}

// Step 3 of the method on A[Mp][ld] in LDS (Mp even, P = Mp / 2 pairs): V^T <- I when wanted, then sweeps of the round-robin cyclic
// Jacobi until the stopping rule (eps2) holds or max_sweeps are done.  cst[P][4], tab (eig_fill_tab(P)) and red[EIG_THREADS] are LDS scratch.
// Returns the sweeps used; A's diagonal holds the eigenvalues, row k of V^T the vector of A[k][k].  Ends behind a barrier.
__device__ __forceinline__ int eig_jacobi(float* A, float* Vt, int Mp, int ld, float* cst, const unsigned short* tab, double* red,
                                          bool want_v, double eps2, int max_sweeps, bool& converged) {
  const int t = threadIdx.x;
  const int P = Mp >> 1;
  const int T = P * (P + 1) / 2;
  if (want_v) {
    for (int e = t; e < Mp * Mp; e += EIG_THREADS) {
      const int i = e / Mp, j = e - i * Mp;
      Vt[i * ld + j] = i == j ? 1.f : 0.f;
    }
  }
  const int vk0 = t / Mp, vj0 = t - vk0 * Mp, vkd = EIG_THREADS / Mp, vjd = EIG_THREADS - vkd * Mp;
  int n_sweeps = 0;
  converged = false;
  for (;;) {
    converged = eig_converged(A, Mp, ld, eps2, red);
    if (converged || n_sweeps == max_sweeps) break;
    for (int s = 0; s < Mp - 1; ++s) {
      if (t < P) {
        int p, q;
        rr_pair(t, s, Mp, p, q);
        const float apq = A[p * ld + q];
        float c = 1.f, sn = 0.f, tn = 0.f;
        if (apq != 0.f) {
          const float tau = (A[q * ld + q] - A[p * ld + p]) / (2.f * apq);
          tn = copysignf(1.f, tau) / (fabsf(tau) + sqrtf(1.f + tau * tau));   // (tau^2 = inf: t = 0, the identity)
          c = 1.f / sqrtf(1.f + tn * tn);
          sn = tn * c;
        }
        reinterpret_cast<float4*>(cst)[t] = make_float4(c, sn, tn, 0.f);
      }
      __syncthreads();
      for (int e = t; e < T; e += EIG_THREADS) {
        const int kl = tab[e];
        const int k = kl & 255, l = kl >> 8;
        int pk, qk, pl, ql;
        rr_pair(k, s, Mp, pk, qk);
        rr_pair(l, s, Mp, pl, ql);
        const float4 rk = reinterpret_cast<const float4*>(cst)[k];
        const float b00 = A[pk * ld + pl], b01 = A[pk * ld + ql], b10 = A[qk * ld + pl], b11 = A[qk * ld + ql];
        if (k == l) {
          A[pk * ld + pk] = b00 - rk.z * b01;
          A[qk * ld + qk] = b11 + rk.z * b01;
          A[pk * ld + qk] = 0.f;
          A[qk * ld + pk] = 0.f;
        } else {   // tile (k, l), k < l, and its mirror image: A stays exactly symmetric
          const float4 rl = reinterpret_cast<const float4*>(cst)[l];
          const float r00 = rk.x * b00 - rk.y * b10, r10 = rk.y * b00 + rk.x * b10;
          const float r01 = rk.x * b01 - rk.y * b11, r11 = rk.y * b01 + rk.x * b11;
          const float n00 = rl.x * r00 - rl.y * r01, n01 = rl.y * r00 + rl.x * r01;
          const float n10 = rl.x * r10 - rl.y * r11, n11 = rl.y * r10 + rl.x * r11;
          A[pk * ld + pl] = n00;
          A[pl * ld + pk] = n00;
          A[pk * ld + ql] = n01;
          A[ql * ld + pk] = n01;
          A[qk * ld + pl] = n10;
          A[pl * ld + qk] = n10;
          A[qk * ld + ql] = n11;
          A[ql * ld + qk] = n11;
        }
      }
      if (want_v) {
        for (int k = vk0, j = vj0; k < P;) {   // element (k, j) = t, t + EIG_THREADS, ... of [P][Mp] without a division per element
          int pk, qk;
          rr_pair(k, s, Mp, pk, qk);
          const float4 rk = reinterpret_cast<const float4*>(cst)[k];
          const float vp = Vt[pk * ld + j], vq = Vt[qk * ld + j];
          Vt[pk * ld + j] = rk.x * vp - rk.y * vq;
          Vt[qk * ld + j] = rk.y * vp + rk.x * vq;
          k += vkd;
          j += vjd;
          if (j >= Mp) {
            j -= Mp;
            ++k;
          }
        }
      }
      __syncthreads();
    }
    ++n_sweeps;
  }
  return n_sweeps;
}

// Step 4 for the M real coordinates of one molecule: rank the eigenvalues dg[i] = A[i][i] by counting (index as tie-break), fix each
// mode's sign (largest |component| positive, lowest index on a tie), write evals at `evals` and, when wanted, the modes as rows of
// out[M][M].  dg / rank / sgn [M] are LDS scratch.  Coordinates M .. of A and V^T (padding) are left out by index.
__device__ __forceinline__ void eig_sort_write(const float* A, const float* Vt, int M, int ld, float* dg, int* rank, float* sgn,
                                               float* evals, float* out, bool want_v) {
  const int t = threadIdx.x;
  for (int i = t; i < M; i += EIG_THREADS) dg[i] = A[i * ld + i];
  __syncthreads();
  for (int i = t; i < M; i += EIG_THREADS) {
    const float di = dg[i];
    int r = 0;
    for (int j = 0; j < M; ++j) {
      const float dj = dg[j];
      r += dj < di || (dj == di && j < i) ? 1 : 0;
    }
    rank[i] = r;
    evals[r] = di;
    if (want_v) {
      float best = -1.f, sg = 1.f;
      for (int j = 0; j < M; ++j) {
        const float v = Vt[i * ld + j];
        if (fabsf(v) > best) {
          best = fabsf(v);
          sg = v < 0.f ? -1.f : 1.f;
        }
      }
      sgn[i] = sg;
    }
  }
  if (want_v) {
    __syncthreads();
    for (int e = t; e < M * M; e += EIG_THREADS) {
      const int i = e / M, j = e - i * M;
      out[(size_t)rank[i] * M + j] = sgn[i] * Vt[i * ld + j];
    }
  }
}

}  // namespace
