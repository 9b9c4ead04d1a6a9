// Batched normal-mode analysis (gfx950, fp32): one workgroup per molecule diagonalises its mass-weighted Hessian block in LDS.
//
// nnhip_hessian_blocks (csrc/train_step.hip, csrc/hessian.hip) leaves one small dense symmetric matrix per molecule on the
// device, M = 3 n_b, mutually independent.  What a user wants from it is the spectrum, so this file does in ONE launch per batch:
//   1. load H_b from the packed blocks, symmetrise (H + H^T)/2 (the fp32 Hessian is symmetric only to rounding), mass-weight
//      A[ia][jb] = H[ia][jb] / sqrt(m_i m_j)                                                    (masses == null: unit masses)
//   2. optionally project the translations and rotations out: d_k = the translation / rotation vectors of the molecule in
//      mass-weighted coordinates about the centre of mass, orthonormalised by modified Gram-Schmidt in fp64 (a vector whose remainder
//      is not above 1e-5 of its own norm before is dropped: a linear molecule loses one rotation, one atom all three; a periodic
//      molecule -- any non-zero cell entry -- keeps the translations only), A <- P A P with P = I - sum_k d_k d_k^T, formed as
//      A - D U^T - U D^T with W = A D, G = D^T W, U = W - D G / 2, everything of this step in fp64
//   3. cyclic Jacobi with the round-robin ("tournament") ordering: Mp = M rounded up to even, P = Mp/2 disjoint rotations per step,
//      Mp - 1 steps per sweep.  Step s pairs (Mp - 1, s) and ((s + k) mod (Mp - 1), (s - k) mod (Mp - 1)), k = 1 .. P - 1 (the circle
//      method in closed form: no index tables).  A step is two barrier-separated phases:
//        a. thread k < P forms (c, s, t) of pair k from a_pp, a_qq, a_pq                                 (Rutishauser's formulas)
//        b. A <- J^T A J in 2 x 2 tiles: the thread of tile (k, l), k <= l, reads rows {p_k, q_k} x columns {p_l, q_l}, applies pair
//           k's rotation from the left and pair l's from the right in registers and writes the tile AND its mirror image -- the
//           row and the column phase of the textbook method in one pass over half the matrix, A stays exactly symmetric, no
//           element is touched by two threads; the diagonal tiles are written in closed form (a_pq = 0 exactly).  Rows p_k, q_k
//           of V^T take pair k's rotation in the same phase.
//      A and V^T live in LDS in fp32 with row stride Mp + 1 (odd: the column walks of the tiles, the symmetrisation and the
//      projection hit distinct banks).  V^T is kept rather than V so that its updates are row operations and row k is mode k.
//      After every sweep off(A)^2 and ||A||_F^2 are summed in a fixed order (fp64); stop at off(A) <= 2^-24 ||A||_F or after
//      EIG_MAX_SWEEPS sweeps (status bit 0).  A molecule with a mass that is not positive and finite is not computed (status bit 2).  An odd M idles on the padding index: its row and column are zero, so its rotations are
//      the identity.
//   4. rank the eigenvalues by counting (index as tie-break), fix each mode's sign (largest |component| positive, lowest index on a
//      tie) and write evals at 3 mol_ptr[b] and the modes, ROW k = mode k, at blk_ptr[b].
// No float atomics, every sum in a fixed order: two calls on the same input are bitwise identical.  modes == null skips V^T
// altogether (half the LDS, about half the work); A's arithmetic does not depend on V, so the eigenvalues are bitwise the same.
#include "common.h"

#define EIG_THREADS 256
#define EIG_MAX_DIM 126        // largest M = 3 n_b served (42 atoms): A and V^T in LDS take 2 x 126 x 127 x 4 = 128 016 bytes of 160 KiB
#define EIG_MAX_SWEEPS 30
#define EIG_DROP_TOL 1e-5      // Gram-Schmidt: a vector whose remainder is not above this fraction of its norm is dropped

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

// bytes of the region V^T and the projection scratch share (a multiple of 8)
__host__ __device__ inline size_t eig_x_bytes(int mp_max, bool want_v) {
  const size_t v = want_v ? 4 * (size_t)mp_max * (mp_max + 1) : 0, d = 8 * (12 * (size_t)mp_max + 36);
  return v > d ? v : d;
}

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

__global__ void __launch_bounds__(EIG_THREADS)
eig_kernel(EigArgs g) {
  extern __shared__ __align__(16) double smem_d[];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const int a0 = g.mol_ptr[b];
  const int nb = g.mol_ptr[b + 1] - a0;
  if (nb <= 0) return;   // (uniform over the workgroup)
  if (t == 0) {
    g.n_proj[b] = 0;
    g.sweeps[b] = 0;
    g.status[b] = 0;
  }
  const int M = 3 * nb;
  const int Mp = (M + 1) & ~1;
  if (Mp > g.mp_max) {   // mol_ptr and mol_ptr_host disagree: the LDS of this launch is too small for the molecule (uniform)
    if (t == 0) g.status[b] = NNHIP_EIG_STATUS_SIZE;
    return;
  }
  const int P = Mp >> 1;
  const int ld = Mp + 1;
  const bool want_v = g.modes != nullptr;
  // LDS carve-up, sized by the host for the largest molecule of the batch (g.mp_max).  The fp64 scratch of the projection (D, U,
  // G) shares its space with V^T, which is not needed before the Jacobi sweeps: an aspirin (Mp = 64) with modes takes 38 176
  // bytes, four workgroups per CU.
  const int mpx = g.mp_max;
  double* red = smem_d;                    // [EIG_THREADS]
  double* rsm = red + EIG_THREADS;         // [mpx] 1 / sqrt(m_i) (n_b entries used)
  float* cst = reinterpret_cast<float*>(rsm + mpx);             // [mpx / 2][4]  (c, s, t, -) of the step's pairs
  float* dg = cst + 4 * (mpx / 2);         // [mpx]  eigenvalues before sorting
  int* rank = reinterpret_cast<int*>(dg + mpx);                 // [mpx]
  float* sgn = reinterpret_cast<float*>(rank + mpx);            // [mpx]
  float* A = sgn + mpx;                    // [mpx][mpx + 1] (this molecule uses [Mp][ld])
  float* Vt = A + mpx * (mpx + 1);         // the same again when modes are wanted ...
  double* D = reinterpret_cast<double*>(Vt);   // ... [6][mpx] orthonormal translation / rotation vectors
  double* U = D + 6 * mpx;                 // [6][mpx]  W = A D, then U = W - D G / 2
  double* G = U + 6 * mpx;                 // [36]
  unsigned short* tab = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(Vt) + eig_x_bytes(mpx, want_v));   // [P (P + 1) / 2] tiles k <= l as k | l << 8
  const int T = P * (P + 1) / 2;
  for (int e = t; e < P * P; e += EIG_THREADS) {
    const int k = e / P, l = e - k * P;
    if (k <= l) tab[k * P - k * (k - 1) / 2 + (l - k)] = (unsigned short)(k | l << 8);
  }

  // ---- 1. load, symmetrise, mass-weight -------------------------------------------------------------------------------
  const float* H = g.blocks + g.blk_ptr[b];
  int bad_mass = 0;
  for (int i = t; i < nb; i += EIG_THREADS) {
    const float m = g.masses ? g.masses[a0 + i] : 1.f;
    bad_mass |= !(m > 0.f && m <= 3.4e38f);   // zero, negative, infinite or NaN
    rsm[i] = 1.0 / sqrt((double)m);
  }
  if (__syncthreads_or(bad_mass)) {   // (uniform) nothing of this molecule is computed: its outputs keep what the caller put there
    if (t == 0) g.status[b] = NNHIP_EIG_STATUS_MASS;
    return;
  }
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
      double* d = D + n_kept * mpx;
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
        const double* dj = D + j * mpx;
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
        const double* d = D + k * mpx;
        double w = 0.0;
        for (int j = 0; j < M; ++j) w += (double)A[i * ld + j] * d[j];
        U[k * mpx + i] = w;
      }
      __syncthreads();
      // G = D^T W
      if (t < n_kept * n_kept) {
        const int k = t / n_kept, l = t - k * n_kept;
        double s = 0.0;
        for (int i = 0; i < M; ++i) s += D[k * mpx + i] * U[l * mpx + i];
        G[k * 6 + l] = s;
      }
      __syncthreads();
      // U = W - D G / 2   (G symmetrised: A is)
      double u_new[6];
      for (int e = t; e < M; e += EIG_THREADS) {
        for (int k = 0; k < n_kept; ++k) {
          double s = U[k * mpx + e];
          for (int l = 0; l < n_kept; ++l) s -= 0.25 * (G[l * 6 + k] + G[k * 6 + l]) * D[l * mpx + e];
          u_new[k] = s;
        }
        for (int k = 0; k < n_kept; ++k) U[k * mpx + e] = u_new[k];
      }
      __syncthreads();
      // A <- A - D U^T - U D^T
      for (int e = t; e < M * M; e += EIG_THREADS) {
        const int i = e / M, j = e - i * M;
        if (i > j) continue;
        double v = (double)A[i * ld + j];
        for (int k = 0; k < n_kept; ++k) v -= D[k * mpx + i] * U[k * mpx + j] + U[k * mpx + i] * D[k * mpx + j];
        A[i * ld + j] = (float)v;
        A[j * ld + i] = (float)v;
      }
      __syncthreads();
    }
    if (t == 0) g.n_proj[b] = n_kept;
  }

  // ---- 3. Jacobi ----------------------------------------------------------------------------------------------------------
  if (want_v) {
    for (int e = t; e < Mp * Mp; e += EIG_THREADS) {
      const int i = e / Mp, j = e - i * Mp;
      Vt[i * ld + j] = i == j ? 1.f : 0.f;
    }
  }
  const int vk0 = t / Mp, vj0 = t - vk0 * Mp, vkd = EIG_THREADS / Mp, vjd = EIG_THREADS - vkd * Mp;
  const double eps2 = 3.552713678800501e-15;   // (2^-24)^2
  int n_sweeps = 0;
  bool converged = false;
  for (;;) {
    double off = 0.0, diag = 0.0;
    for (int e = t; e < Mp * Mp; e += EIG_THREADS) {
      const int i = e / Mp, j = e - i * Mp;
      const double a = (double)A[i * ld + j];
      if (i == j) diag += a * a; else off += a * a;
    }
    off = block_sum(off, red);
    diag = block_sum(diag, red);
    // (an Inf entry makes both sides +inf: without the second test it would pass as converged; a NaN fails the first)
    converged = off <= eps2 * (off + diag) && off + diag <= 1.7976931348623157e308;
    if (converged || n_sweeps == EIG_MAX_SWEEPS) break;
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
  if (t == 0) {
    g.sweeps[b] = n_sweeps;
    g.status[b] = converged ? 0 : NNHIP_EIG_STATUS_SWEEPS;
  }

  // ---- 4. sort, fix signs, write ---------------------------------------------------------------------------------------
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
    g.evals[3 * (size_t)a0 + r] = di;
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
    float* out = g.modes + g.blk_ptr[b];
    for (int e = t; e < M * M; e += EIG_THREADS) {
      const int i = e / M, j = e - i * M;
      out[(size_t)rank[i] * M + j] = sgn[i] * Vt[i * ld + j];
    }
  }
}

size_t eig_lds_bytes(int mp_max, bool want_v) {
  const int p = mp_max / 2;
  return 8 * ((size_t)EIG_THREADS + mp_max) + 4 * (5 * (size_t)mp_max + (size_t)mp_max * (mp_max + 1)) + eig_x_bytes(mp_max, want_v) +
         2 * (size_t)(p * (p + 1) / 2);
}

}  // namespace

extern "C" int nnhip_eig_max_dim(void) { return EIG_MAX_DIM; }

extern "C" int nnhip_eig_blocks(const float* blocks, const int64_t* blk_ptr, const int32_t* mol_ptr, const int32_t* mol_ptr_host,
                                int32_t n_mol, const float* pos, const float* cell, const float* masses, int32_t flags, float* evals,
                                float* modes, int32_t* n_proj, int32_t* sweeps, int32_t* status, void* stream) {
  if (n_mol < 0 || (n_mol > 0 && (!blocks || !blk_ptr || !mol_ptr || !mol_ptr_host || !evals || !n_proj || !sweeps || !status)) ||
      ((flags & NNHIP_EIG_PROJECT) && n_mol > 0 && (!pos || !cell)) || (flags & ~NNHIP_EIG_PROJECT)) {
    nnhip_set_error("nnhip_eig_blocks: bad arguments");
    return NNHIP_E_INVALID;
  }
  int m_max = 0;
  for (int b = 0; b < n_mol; ++b) {
    const int m = 3 * (mol_ptr_host[b + 1] - mol_ptr_host[b]);
    if (m < 0) {
      nnhip_set_error("nnhip_eig_blocks: mol_ptr_host decreases at molecule %d", b);
      return NNHIP_E_INVALID;
    }
    if (m > EIG_MAX_DIM) {
      nnhip_set_error("nnhip_eig_blocks: molecule %d has dimension 3 x %d = %d, above the supported %d (one workgroup holds the "
                      "matrix and its eigenvectors in LDS)", b, m / 3, m, EIG_MAX_DIM);
      return NNHIP_E_UNSUPPORTED;
    }
    m_max = m > m_max ? m : m_max;
  }
  if (m_max == 0) return NNHIP_OK;
  EigArgs g;
  g.blocks = blocks;
  g.blk_ptr = blk_ptr;
  g.mol_ptr = mol_ptr;
  g.pos = pos;
  g.cell = cell;
  g.masses = masses;
  g.evals = evals;
  g.modes = modes;
  g.n_proj = n_proj;
  g.sweeps = sweeps;
  g.status = status;
  g.n_mol = n_mol;
  g.project = (flags & NNHIP_EIG_PROJECT) ? 1 : 0;
  g.mp_max = (m_max + 1) & ~1;
  const size_t lds = eig_lds_bytes(g.mp_max, modes != nullptr);
  if (lds > 64 * 1024)   // above the default limit a kernel has to ask for its dynamic LDS
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(eig_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)eig_lds_bytes((EIG_MAX_DIM + 1) & ~1, true)));
  eig_kernel<<<n_mol, EIG_THREADS, lds, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
