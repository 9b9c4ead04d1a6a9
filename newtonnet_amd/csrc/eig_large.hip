// Normal modes above the one-workgroup bound (gfx950, fp32): two-sided BLOCK Jacobi over many workgroups, A and V^T in the caller's
// workspace (HBM / L2).  Opt-in (nnhip_eig_blocks_large); csrc/eig.hip keeps serving M <= 126 unchanged.
//
// The scalar method of eig.hip with blocks of EIGL_B = 32 coordinates in place of scalars.  The order is padded to Mp = a multiple of
// 64, nblk = Mp / 32 blocks (even), P = nblk / 2 disjoint block pairs per step, nblk - 1 steps per sweep on the same round-robin
// ordering (rr_pair).  Every dependency between workgroups is a kernel boundary on the one stream: no cooperative launch, no
// grid barrier, no spin-wait, every device loop has a fixed trip bound.
//   prepare   one workgroup per molecule: steps 1 and 2 of eig.hip by the SAME device function (eig_load_project: symmetrise,
//             mass-weight in fp64, round once to fp32, project in fp64 with fixed-order sums) on A in the workspace; padding rows and
//             columns exactly zero; V^T = I; status bits 1 and 2 decided here (such a molecule is not computed and nothing of it is
//             written).
//   per sweep converge: one workgroup per molecule sums off(A)^2 and ||A||_F^2 in fp64 in a fixed order (eig_converged, the rule of
//             eig.hip: off <= 2^-24 ||A||_F, a NaN or an Inf never passes) and sets the molecule's done flag; the host reads the
//             flags once per sweep and stops when all are set; after EIG_MAX_SWEEPS sweeps status bit 0 is set.  Workgroups of a
//             done molecule leave at their first instruction.
//   per step  pair solve, one workgroup per (molecule, block pair k): gathers the 64 x 64 diagonal sub-problem of blocks (p_k, q_k)
//             into LDS, diagonalises it with the in-LDS cyclic Jacobi of eig.hip (eig_jacobi, at most EIGL_INNER_SWEEPS sweeps),
//             re-orthogonalises the accumulated rotation Qt_k = V^T of the sub-problem (one Newton-Schulz step, fp64 sums) and
//             writes it (64 x 64) to the workspace and the diagonal tile back: the solved diagonal and exact zeros.
//             tile update, one workgroup per (molecule, k < l): T <- Qt_k T Qt_l^T for the 64 x 64 tile rows (p_k, q_k) x columns
//             (p_l, q_l), both factors in LDS, fp32 operands, fp32 fma accumulation in the fixed order m = 0 .. 63; writes the tile AND
//             its mirror image (A stays exactly symmetric, no element has two writers -- phase b of eig.hip on blocks).  In the same
//             launch, one workgroup per (molecule, k, 64-column chunk): rows (p_k, q_k) of V^T <- Qt_k x those rows (skipped
//             without modes: A's arithmetic does not read V, the eigenvalues are bitwise the same).
//   finish    one workgroup per molecule: eig_sort_write over the M real coordinates (padding is identified by INDEX, never by
//             value: the projected zero modes of the molecule stay).
// Padding never mixes with real coordinates: its rows and columns are exactly zero, so in every sub-problem a_pq = 0 -> the identity
// rotation, Qt has the unit row and column there, and products with exact zeros and ones keep the zeros exact.
// A molecule's result does not depend on the rest of the batch: every decision is per molecule; only grid sizes follow the batch.
#include <vector>

#include "eig_common.h"

#define EIGL_B 32               // coordinates per block
#define EIGL_S (2 * EIGL_B)     // order of a pair's sub-problem and of a tile
#define EIGL_LD (EIGL_S + 1)    // its row stride in LDS (odd: column walks hit distinct banks)
#define EIGL_MAX_DIM 1536       // 512 atoms.  Bounds: the accuracy the tests have verified (M = 648 at c < 8 in units of M 2^-24 ||A||_2; the
                                // bound itself grows with M), 8 Mp^2 bytes of workspace per molecule (19 MB here), one workgroup per
                                // molecule in prepare / converge / finish (time ~ Mp^2 / 256 per thread) and dg / rank / sgn of finish in LDS
#define EIGL_INNER_SWEEPS 15    // cap of the in-LDS solve of one sub-problem (a 64 x 64 block converges in 6 - 9; a NaN runs to the cap)
// The sub-problems stop at off <= 2^-27 ||sub||_F, 8 times tighter than the molecule's rule.  Every off-diagonal element of A lies in a
// sub-problem of the sweep and every diagonal block in nblk - 1 <= 47 < 64 of them, so when no sub-problem has anything left to do,
// off(A)^2 <= 2^-54 (nblk - 1) ||A||_F^2 < 2^-48 ||A||_F^2: the molecule's rule holds and the iteration cannot stall short of it.
#define EIGL_INNER_EPS2 (EIG_EPS2 / 64.0)

namespace {

struct LMol {       // one SELECTED molecule with atoms (host copy of the table the kernels read)
  size_t base;      // byte offset of its region in the workspace
  int b;            // molecule index
  int mp;           // padded order (multiple of EIGL_S), by mol_ptr_host
  int n;            // atoms, by mol_ptr_host
  int pad_;
};

struct LArgs {
  char* ws;
  const LMol* tab;  // [n_sel] (in ws)
  int* done;        // [n_sel] 0 = iterating, 1 = finished (converged or at the cap), 2 = not computed
  int want_v;
};

inline int pad_order(int m) { return (m + EIGL_S - 1) / EIGL_S * EIGL_S; }
inline size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t header_bytes(int n_sel) { return round256((size_t)n_sel * sizeof(LMol)) + round256((size_t)n_sel * sizeof(int)); }
// region of one molecule: A [mp][mp] | V^T [mp][mp] (modes) | Qt [mp / 64][64][64] | fp64: rsm [mp], D [6][mp], U [6][mp], G [64]
__host__ __device__ inline size_t off_vt(int mp) { return 4 * (size_t)mp * mp; }
__host__ __device__ inline size_t off_q(int mp, int want_v) { return 4 * (size_t)mp * mp * (want_v ? 2 : 1); }
__host__ __device__ inline size_t off_d(int mp, int want_v) { return off_q(mp, want_v) + 4 * (size_t)(mp / EIGL_S) * EIGL_S * EIGL_S; }
__host__ __device__ inline size_t region_bytes(int mp, int want_v) { return off_d(mp, want_v) + 8 * (13 * (size_t)mp + 64); }

// global coordinate of index i of the sub-problem of blocks (p, q)
__device__ __forceinline__ int sub_coord(int i, int p, int q) { return (i < EIGL_B ? p : q) * EIGL_B + (i & (EIGL_B - 1)); }

__global__ void __launch_bounds__(EIG_THREADS)
eigl_prepare_kernel(EigArgs g, LArgs L) {
  __shared__ double red[EIG_THREADS];
  const LMol m = L.tab[blockIdx.x];
  const int t = threadIdx.x;
  const int b = m.b;
  const int a0 = g.mol_ptr[b];
  const int nb = g.mol_ptr[b + 1] - a0;
  if (nb <= 0) {   // (uniform) empty by mol_ptr: nothing is written, as in eig.hip
    if (t == 0) L.done[blockIdx.x] = 2;
    return;
  }
  if (t == 0) {
    g.n_proj[b] = 0;
    g.sweeps[b] = 0;
    g.status[b] = 0;
  }
  if (nb > m.n) {   // mol_ptr gives the molecule more atoms than mol_ptr_host did: its region is too small (uniform)
    if (t == 0) {
      g.status[b] = NNHIP_EIG_STATUS_SIZE;
      L.done[blockIdx.x] = 2;
    }
    return;
  }
  const int Mp = m.mp;
  char* reg = L.ws + m.base;
  float* A = reinterpret_cast<float*>(reg);
  double* rsm = reinterpret_cast<double*>(reg + off_d(Mp, L.want_v));
  double* D = rsm + Mp;
  double* U = D + 6 * Mp;
  double* G = U + 6 * Mp;
  if (!eig_load_project(g, b, a0, nb, Mp, A, Mp, rsm, D, U, G, Mp, red)) {
    if (t == 0) {
      g.status[b] = NNHIP_EIG_STATUS_MASS;
      L.done[blockIdx.x] = 2;
    }
    return;
  }
  if (L.want_v) {
    float* Vt = reinterpret_cast<float*>(reg + off_vt(Mp));
    for (int e = t; e < Mp * Mp; e += EIG_THREADS) {
      const int i = e / Mp, j = e - i * Mp;
      Vt[e] = i == j ? 1.f : 0.f;
    }
  }
  if (t == 0) L.done[blockIdx.x] = 0;
}

// before sweep `it` (0-based): done when the stopping rule holds; at it == EIG_MAX_SWEEPS the cap is hit
__global__ void __launch_bounds__(EIG_THREADS)
eigl_converge_kernel(EigArgs g, LArgs L, int it) {
  __shared__ double red[EIG_THREADS];
  if (L.done[blockIdx.x]) return;   // (uniform)
  const LMol m = L.tab[blockIdx.x];
  const bool converged = eig_converged(reinterpret_cast<const float*>(L.ws + m.base), m.mp, m.mp, EIG_EPS2, red);
  if (threadIdx.x == 0) {
    if (converged) {
      L.done[blockIdx.x] = 1;
    } else if (it == EIG_MAX_SWEEPS) {
      L.done[blockIdx.x] = 1;
      g.status[m.b] = NNHIP_EIG_STATUS_SWEEPS;
    } else {
      g.sweeps[m.b] = it + 1;   // the sweep that follows
    }
  }
}

__global__ void __launch_bounds__(EIG_THREADS)
eigl_pair_kernel(LArgs L, int s) {
  __shared__ double red[EIG_THREADS];
  __shared__ __align__(16) float cst[4 * EIGL_B];
  __shared__ float As[EIGL_S * EIGL_LD];
  __shared__ float Qs[EIGL_S * EIGL_LD];
  __shared__ unsigned short tab[EIGL_B * (EIGL_B + 1) / 2];
  __shared__ float dgs[EIGL_S];
  if (L.done[blockIdx.x]) return;   // (uniform)
  const LMol m = L.tab[blockIdx.x];
  const int nblk = m.mp / EIGL_B;
  const int k = blockIdx.y;
  if (s >= nblk - 1 || k >= nblk / 2) return;
  const int t = threadIdx.x;
  const int ld = m.mp;
  float* A = reinterpret_cast<float*>(L.ws + m.base);
  int p, q;
  rr_pair(k, s, nblk, p, q);
  for (int e = t; e < EIGL_S * EIGL_S; e += EIG_THREADS) {
    const int i = e / EIGL_S, j = e - i * EIGL_S;
    As[i * EIGL_LD + j] = A[(size_t)sub_coord(i, p, q) * ld + sub_coord(j, p, q)];
  }
  eig_fill_tab(tab, EIGL_B);
  bool converged;   // (not used: a sub-problem short of the rule is met again in the next sweep)
  eig_jacobi(As, Qs, EIGL_S, EIGL_LD, cst, tab, red, true, EIGL_INNER_EPS2, EIGL_INNER_SWEEPS, converged);
  // Qt as accumulated from fp32 rotations is orthogonal to about 3 x 64 x 2^-24 only (each (c, s) has c^2 + s^2 = 1 to rounding, and
  // the defects add up along a row), while the diagonal (Rutishauser's update) is an order of magnitude better.  V^T is a product of
  // some (nblk - 1) x sweeps such factors, so each is brought back to the nearest orthogonal matrix by one Newton-Schulz step
  // Qt <- Qt - E Qt / 2,  E = Qt Qt^T - I  (fp64 accumulation, fixed order; the defect left is |E|^2 ~ 1e-10)
  // before it is used: the tile updates then are orthogonal similarities to rounding, consistent with the solved diagonal.
  if (t < EIGL_S) dgs[t] = As[t * EIGL_LD + t];
  __syncthreads();
  for (int e = t; e < EIGL_S * EIGL_S; e += EIG_THREADS) {
    const int i = e / EIGL_S, j = e - i * EIGL_S;
    double gsum = 0.0;
    for (int mm = 0; mm < EIGL_S; ++mm) gsum += (double)Qs[i * EIGL_LD + mm] * (double)Qs[j * EIGL_LD + mm];
    As[i * EIGL_LD + j] = (float)(gsum - (i == j ? 1.0 : 0.0));
  }
  __syncthreads();
  float* Q = reinterpret_cast<float*>(L.ws + m.base + off_q(m.mp, L.want_v)) + (size_t)k * EIGL_S * EIGL_S;
  for (int e = t; e < EIGL_S * EIGL_S; e += EIG_THREADS) {
    const int i = e / EIGL_S, j = e - i * EIGL_S;
    float acc = 0.f;
    for (int mm = 0; mm < EIGL_S; ++mm) acc = fmaf(As[i * EIGL_LD + mm], Qs[mm * EIGL_LD + j], acc);
    Q[e] = fmaf(-0.5f, acc, Qs[i * EIGL_LD + j]);
    A[(size_t)sub_coord(i, p, q) * ld + sub_coord(j, p, q)] = i == j ? dgs[i] : 0.f;
  }
}

// acc[a][c] = sum_m X[i_a][m] Y(m, j_c), i_a = ti + 16 a, j_c = tj + 16 c, m ascending; Y(m, j) = Ys[m][j] or, transposed, Ys[j][m]
template <bool kTransY>
__device__ __forceinline__ void tile_product(const float* Xs, const float* Ys, int ti, int tj, float acc[4][4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
  for (int mm = 0; mm < EIGL_S; ++mm) {
    float x[4], y[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) x[a] = Xs[(ti + 16 * a) * EIGL_LD + mm];
#pragma unroll
    for (int c = 0; c < 4; ++c) y[c] = kTransY ? Ys[(tj + 16 * c) * EIGL_LD + mm] : Ys[mm * EIGL_LD + tj + 16 * c];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = fmaf(x[a], y[c], acc[a][c]);
  }
}

// blockIdx.y < n_at: tile k < l of A;  else (modes): rows of pair k x 64-column chunk of V^T.  n_at / p_max: grid decoding (batch-wide,
// no arithmetic depends on them)
__global__ void __launch_bounds__(EIG_THREADS)
eigl_update_kernel(LArgs L, int s, int n_at, int p_max) {
  __shared__ float S0[EIGL_S * EIGL_LD];
  __shared__ float S1[EIGL_S * EIGL_LD];
  __shared__ float S2[EIGL_S * EIGL_LD];
  if (L.done[blockIdx.x]) return;   // (uniform)
  const LMol m = L.tab[blockIdx.x];
  const int nblk = m.mp / EIGL_B;
  const int P = nblk / 2;
  if (s >= nblk - 1) return;
  const int t = threadIdx.x;
  const int ti = t >> 4, tj = t & 15;
  const int ld = m.mp;
  const float* Qall = reinterpret_cast<const float*>(L.ws + m.base + off_q(m.mp, L.want_v));
  float acc[4][4];
  if ((int)blockIdx.y < n_at) {
    int k = 0, rem = blockIdx.y;
    if (rem >= P * (P - 1) / 2) return;
    for (; k < P - 1; ++k) {   // row k of the strict upper triangle holds P - 1 - k tiles
      if (rem < P - 1 - k) break;
      rem -= P - 1 - k;
    }
    const int l = k + 1 + rem;
    int pk, qk, pl, ql;
    rr_pair(k, s, nblk, pk, qk);
    rr_pair(l, s, nblk, pl, ql);
    float* A = reinterpret_cast<float*>(L.ws + m.base);
    const float* Qk = Qall + (size_t)k * EIGL_S * EIGL_S;
    const float* Ql = Qall + (size_t)l * EIGL_S * EIGL_S;
    for (int e = t; e < EIGL_S * EIGL_S; e += EIG_THREADS) {
      const int i = e / EIGL_S, j = e - i * EIGL_S;
      S0[i * EIGL_LD + j] = Qk[e];
      S2[i * EIGL_LD + j] = Ql[e];
      S1[i * EIGL_LD + j] = A[(size_t)sub_coord(i, pk, qk) * ld + sub_coord(j, pl, ql)];
    }
    __syncthreads();
    tile_product<false>(S0, S1, ti, tj, acc);   // R = Qt_k T
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) S1[(ti + 16 * a) * EIGL_LD + tj + 16 * c] = acc[a][c];
    __syncthreads();
    tile_product<true>(S1, S2, ti, tj, acc);    // N = R Qt_l^T
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const size_t gi = sub_coord(ti + 16 * a, pk, qk);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t gj = sub_coord(tj + 16 * c, pl, ql);
        A[gi * ld + gj] = acc[a][c];
        A[gj * ld + gi] = acc[a][c];
      }
    }
  } else {
    const int v = blockIdx.y - n_at;
    const int k = v / p_max, ch = v - k * p_max;
    if (!L.want_v || k >= P || ch >= P) return;   // (mp / 64 = P column chunks)
    int pk, qk;
    rr_pair(k, s, nblk, pk, qk);
    float* Vt = reinterpret_cast<float*>(L.ws + m.base + off_vt(m.mp));
    const float* Qk = Qall + (size_t)k * EIGL_S * EIGL_S;
    for (int e = t; e < EIGL_S * EIGL_S; e += EIG_THREADS) {
      const int i = e / EIGL_S, j = e - i * EIGL_S;
      S0[i * EIGL_LD + j] = Qk[e];
      S1[i * EIGL_LD + j] = Vt[(size_t)sub_coord(i, pk, qk) * ld + ch * EIGL_S + j];
    }
    __syncthreads();
    tile_product<false>(S0, S1, ti, tj, acc);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        Vt[(size_t)sub_coord(ti + 16 * a, pk, qk) * ld + ch * EIGL_S + tj + 16 * c] = acc[a][c];
  }
}

__global__ void __launch_bounds__(EIG_THREADS)
eigl_finish_kernel(EigArgs g, LArgs L) {
  __shared__ float dg[EIGL_MAX_DIM];
  __shared__ int rank[EIGL_MAX_DIM];
  __shared__ float sgn[EIGL_MAX_DIM];
  if (L.done[blockIdx.x] != 1) return;   // (uniform) 2: not computed, its outputs keep what the caller put there
  const LMol m = L.tab[blockIdx.x];
  const int a0 = g.mol_ptr[m.b];
  const int M = 3 * (g.mol_ptr[m.b + 1] - a0);   // (<= 3 m.n <= EIGL_MAX_DIM: prepare checked it)
  const float* A = reinterpret_cast<const float*>(L.ws + m.base);
  const float* Vt = reinterpret_cast<const float*>(L.ws + m.base + off_vt(m.mp));
  const bool want_v = L.want_v != 0;
  eig_sort_write(A, Vt, M, m.mp, dg, rank, sgn, g.evals + 3 * (size_t)a0, want_v ? g.modes + g.blk_ptr[m.b] : nullptr, want_v);
}

// the selected molecules with atoms, their regions laid out in order; returns 0 or the error code (message set)
int plan(const char* who, const int32_t* mol_ptr_host, int n_mol, const uint8_t* select_host, int want_v, std::vector<LMol>& mols,
         size_t& total) {
  int n_sel = 0;
  for (int b = 0; b < n_mol; ++b) {
    const int n = mol_ptr_host[b + 1] - mol_ptr_host[b];
    if (n < 0) {
      nnhip_set_error("%s: mol_ptr_host decreases at molecule %d", who, b);
      return NNHIP_E_INVALID;
    }
    if (select_host && !select_host[b]) continue;
    if (3 * (long)n > EIGL_MAX_DIM) {
      nnhip_set_error("%s: molecule %d has dimension 3 x %d = %ld, above the supported %d (nnhip_eig_large_max_dim)", who, b, n,
                      3 * (long)n, EIGL_MAX_DIM);
      return NNHIP_E_UNSUPPORTED;
    }
    if (n > 0) ++n_sel;
  }
  total = header_bytes(n_sel);
  mols.clear();
  for (int b = 0; b < n_mol; ++b) {
    const int n = mol_ptr_host[b + 1] - mol_ptr_host[b];
    if (n <= 0 || (select_host && !select_host[b])) continue;
    LMol m;
    m.base = total;
    m.b = b;
    m.mp = pad_order(3 * n);
    m.n = n;
    m.pad_ = 0;
    mols.push_back(m);
    total += region_bytes(m.mp, want_v);
  }
  return NNHIP_OK;
}

}  // namespace

extern "C" int nnhip_eig_large_max_dim(void) { return EIGL_MAX_DIM; }

extern "C" size_t nnhip_eig_large_ws_bytes(const int32_t* mol_ptr_host, int32_t n_mol, int32_t want_modes) {
  if (!mol_ptr_host || n_mol <= 0) return 0;
  std::vector<LMol> mols;
  size_t total = 0;
  if (plan("nnhip_eig_large_ws_bytes", mol_ptr_host, n_mol, nullptr, want_modes ? 1 : 0, mols, total) != NNHIP_OK) return 0;
  return total;
}

extern "C" int nnhip_eig_blocks_large(const float* blocks, const int64_t* blk_ptr, const int32_t* mol_ptr, const int32_t* mol_ptr_host,
                                      int32_t n_mol, const float* pos, const float* cell, const float* masses, int32_t flags,
                                      float* evals, float* modes, int32_t* n_proj, int32_t* sweeps, int32_t* status,
                                      const uint8_t* select_host, void* ws, size_t ws_bytes, void* stream) {
  if (n_mol < 0 || (n_mol > 0 && (!blocks || !blk_ptr || !mol_ptr || !mol_ptr_host || !evals || !n_proj || !sweeps || !status)) ||
      ((flags & NNHIP_EIG_PROJECT) && n_mol > 0 && (!pos || !cell)) || (flags & ~NNHIP_EIG_PROJECT)) {
    nnhip_set_error("nnhip_eig_blocks_large: bad arguments");
    return NNHIP_E_INVALID;
  }
  const int want_v = modes != nullptr;
  std::vector<LMol> mols;
  size_t total = 0;
  const int rc = plan("nnhip_eig_blocks_large", mol_ptr_host, n_mol, select_host, want_v, mols, total);
  if (rc != NNHIP_OK) return rc;
  const int n_sel = (int)mols.size();
  if (n_sel == 0) return NNHIP_OK;
  if (!ws || ws_bytes < total || (reinterpret_cast<uintptr_t>(ws) & 255)) {
    nnhip_set_error("nnhip_eig_blocks_large: workspace of %zu bytes, 256-byte aligned, needed (got %zu)", total, ws_bytes);
    return NNHIP_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
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
  g.mp_max = 0;
  LArgs L;
  L.ws = static_cast<char*>(ws);
  L.tab = reinterpret_cast<const LMol*>(ws);
  L.done = reinterpret_cast<int*>(L.ws + round256((size_t)n_sel * sizeof(LMol)));
  L.want_v = want_v;
  // the table goes to the device from pageable memory; `mols` outlives the copy (the loop below waits for the stream)
  HIP_TRY(hipMemcpyAsync(ws, mols.data(), (size_t)n_sel * sizeof(LMol), hipMemcpyHostToDevice, st));
  eigl_prepare_kernel<<<n_sel, EIG_THREADS, 0, st>>>(g, L);
  LAUNCH_CHECK();
  std::vector<int> done((size_t)n_sel, 0);
  for (int it = 0; it <= EIG_MAX_SWEEPS; ++it) {
    eigl_converge_kernel<<<n_sel, EIG_THREADS, 0, st>>>(g, L, it);
    LAUNCH_CHECK();
    // the one read-back per sweep: this path is not the steady-state inference step
    HIP_TRY(hipMemcpyAsync(done.data(), L.done, (size_t)n_sel * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int p_max = 0;   // over the molecules still iterating: sizes the grids only
    for (int i = 0; i < n_sel; ++i)
      if (!done[i]) p_max = mols[i].mp / EIGL_S > p_max ? mols[i].mp / EIGL_S : p_max;
    if (p_max == 0) break;   // (it == EIG_MAX_SWEEPS sets every flag)
    const int n_at = p_max * (p_max - 1) / 2;
    const int n_up = n_at + (want_v ? p_max * p_max : 0);
    for (int s = 0; s < 2 * p_max - 1; ++s) {
      eigl_pair_kernel<<<dim3(n_sel, p_max), EIG_THREADS, 0, st>>>(L, s);
      LAUNCH_CHECK();
      if (n_up > 0) {
        eigl_update_kernel<<<dim3(n_sel, n_up), EIG_THREADS, 0, st>>>(L, s, n_at, p_max);
        LAUNCH_CHECK();
      }
    }
  }
  eigl_finish_kernel<<<n_sel, EIG_THREADS, 0, st>>>(g, L);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
