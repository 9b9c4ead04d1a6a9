// Phonons above the one-workgroup bound (gfx950, fp32): two-sided BLOCK Jacobi for the complex Hermitian D(q) over many workgroups, D(q)
// and the modes in the caller's workspace (HBM / L2).  Opt-in (nnhip_phonon_bands_large); csrc/phonon.hip keeps serving d <= 96 unchanged.
//
// The method of csrc/eig_large.hip for the problem of csrc/phonon.hip.  The unit is one (crystal b, wave vector q) PROBLEM; its order
// d = 3 n_b is padded to Mp = a multiple of 64, nblk = Mp / 32 blocks of PHL_B = 32 coordinates (even), P = nblk / 2 disjoint block pairs
// per step, nblk - 1 steps per sweep on the round-robin ordering (rr_pair).  A (real and imaginary plane, [Mp][Mp] each), W (the same, modes
// only) and the P rotations Qt of a step live in the problem's region of the workspace.  Every dependency between workgroups is a
// kernel boundary on the one stream: no cooperative launch, no grid barrier, no spin-wait, every device loop has a fixed trip bound.
//   prepare   one workgroup per problem: status bits 1 and 2 (cry_ptr gives the crystal more atoms than cry_ptr_host did; a mass that
//             is not positive and finite) -- such a problem is not computed and nothing else of it is written.
//   assemble  one workgroup per (problem, 64 x 64 tile k <= l): D(q) by the device functions of phonon.hip's step 1 (phonon_common.h:
//             ph_weight, ph_accumulate over the copies R ascending, ph_hermitian).  The thread of element (a, c) forms BOTH sums D_ac and
//             D_ca in registers and writes the element and its conjugate mirror image: D is exactly Hermitian, no element has two
//             writers, and each element is bitwise that of nnhip_phonon_bands.  The phase factors of PHL_RCHUNK copies are staged in
//             LDS for the (at most 22 x 22) atom pairs the tile touches, in both directions.  Padding rows and columns exactly zero,
//             W = I on the padded order, dmat written from here.
//   per sweep converge: one workgroup per problem sums off(A)^2 and ||A||_F^2 in fp64 in a fixed order (the rule of eig_common.h:
//             off^2 <= EIG_EPS2 ||A||_F^2, a NaN or an Inf never passes) and sets the problem's done flag; the host reads the flags once
//             per sweep and stops when all are set; after EIG_MAX_SWEEPS sweeps status bit 0 is set.  Workgroups of a done problem
//             leave at their first instruction.
//   per step  pair solve, one workgroup per (problem, block pair k): gathers the 64 x 64 diagonal sub-problem of blocks (p_k, q_k) into
//             LDS (real and imaginary planes, row stride 65), diagonalises it with the complex Jacobi of phonon.hip (ph_jacobi, at most
//             PHL_INNER_SWEEPS sweeps), re-unitarises the accumulated W_k (one Newton-Schulz step W (3 I - W^H W) / 2, the Gram matrix
//             summed in fp64) and writes Qt_k = conj(W_k) = U_k^H and the diagonal tile back: the solved diagonal and exact zeros.
//             tile update, one workgroup per (problem, k < l): T <- Qt_k T Qt_l^H for the tile rows (p_k, q_k) x columns (p_l, q_l), all
//             three in LDS, fp32 operands, fp32 fma accumulation in the fixed order m = 0 .. 63; writes the tile AND its conjugate mirror.
//             In the same launch, one workgroup per (problem, k, 64-column chunk): rows (p_k, q_k) of W <- conj(Qt_k) x those rows
//             (skipped without modes: A's arithmetic does not read W, the eigenvalues are bitwise the same).
//   finish    one workgroup per problem: rank the d real coordinates' eigenvalues by counting (index as tie-break), fix each mode's phase
//             (ph_phase), write in the layout of nnhip_phonon_bands.  Padding is identified by INDEX, never by value.
// Padding never mixes with real coordinates: its rows and columns are exactly zero, so in every sub-problem a_pq = 0 -> the identity
// rotation, Qt has the unit row and column there, and products with exact zeros and ones keep the zeros exact.
// A problem's result does not depend on the rest of the launch: every decision is per problem; only grid sizes follow the batch.  No
// float atomics: two calls are bitwise equal.
#include <vector>

#include "phonon_common.h"

#define PHL_B 32               // coordinates per block
#define PHL_S (2 * PHL_B)      // order of a pair's sub-problem and of a tile
#define PHL_LD (PHL_S + 1)     // its row stride in LDS (odd: column walks hit distinct banks)
#define PHL_PLANE (PHL_S * PHL_LD)
#define PHL_MAX_DIM 768        // 256 atoms.  Bounds: the size the accuracy test runs at, 16 Mp^2 bytes of workspace per problem with
                               // modes (9.4 MB here), one workgroup per problem in converge / finish and dg / rank / phs of finish in LDS
#define PHL_RCHUNK 4           // supercell copies whose phase factors are staged at a time (the sums run over R ascending whatever it is)
#define PHL_TILE_ATOMS 22      // 64 consecutive coordinates touch at most 22 atoms
#define PHL_INNER_SWEEPS 15    // cap of the in-LDS solve of one sub-problem (a NaN runs to the cap)
// The sub-problems stop at off^2 <= EIG_EPS2 / 64 ||sub||_F^2.  Every off-diagonal element of A lies in a sub-problem of the sweep and
// every diagonal block in nblk - 1 <= 23 < 64 of them, so when no sub-problem has anything left to do, off(A)^2 <= (EIG_EPS2 / 64)
// (nblk - 1) ||A||_F^2 < EIG_EPS2 ||A||_F^2: the problem's rule holds and the iteration cannot stall short of it.
#define PHL_INNER_EPS2 (EIG_EPS2 / 64.0)

namespace {

struct LProb {      // one problem of a SELECTED crystal with atoms (host copy of the table the kernels read)
  size_t base;      // byte offset of its region in the workspace
  int b;            // crystal index
  int qi;           // wave vector index
  int mp;           // padded order (multiple of PHL_S), by cry_ptr_host
  int n;            // atoms, by cry_ptr_host
};

struct LArgs {
  char* ws;
  const LProb* tab;  // [n_prob] (in ws)
  int* done;         // [n_prob] 0 = iterating, 1 = finished (converged or at the cap), 2 = not computed
  int want_v;
};

struct PhlArgs {
  const float* fc;
  const int64_t* fc_ptr;
  const int* cry_ptr;
  const int* sc_atoms;
  const int64_t* img_ptr;
  const int* img_start;
  const double* img_off;
  const float* masses;
  const double* q;
  const int64_t* out_ptr;
  float* evals;
  float* modes;
  float* dmat;
  int* sweeps;
  int* status;
  int n_q;
};

inline int pad_order(int m) { return (m + PHL_S - 1) / PHL_S * PHL_S; }
inline size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t header_bytes(size_t n_prob) { return round256(n_prob * sizeof(LProb)) + round256(n_prob * sizeof(int)); }
// region of one problem: Are | Aim [mp][mp] | Wre | Wim [mp][mp] (modes) | Qt [mp / 64] x (re | im) [64][64].  A multiple of 256 bytes.
__host__ __device__ inline size_t off_aim(int mp) { return 4 * (size_t)mp * mp; }
__host__ __device__ inline size_t off_w(int mp) { return 8 * (size_t)mp * mp; }
__host__ __device__ inline size_t off_q(int mp, int want_v) { return 8 * (size_t)mp * mp * (want_v ? 2 : 1); }
__host__ __device__ inline size_t region_bytes(int mp, int want_v) { return off_q(mp, want_v) + 8 * (size_t)(mp / PHL_S) * PHL_S * PHL_S; }

// global coordinate of index i of the sub-problem of blocks (p, q)
__device__ __forceinline__ int sub_coord(int i, int p, int q) { return (i < PHL_B ? p : q) * PHL_B + (i & (PHL_B - 1)); }

// tile e of the upper triangle (k <= l, row by row) of P x P tiles; false when e is past the last
__device__ __forceinline__ bool upper_tile(int e, int P, bool strict, int& k, int& l) {
  const int first = strict ? 1 : 0;
  int rem = e;
  for (k = 0; k < P; ++k) {   // row k holds P - k - first tiles
    const int row = P - k - first;
    if (rem < row) {
      l = k + first + rem;
      return true;
    }
    rem -= row;
  }
  return false;
}

__global__ void __launch_bounds__(PH_THREADS)
phl_prepare_kernel(PhlArgs g, LArgs L) {
  const LProb m = L.tab[blockIdx.x];
  const int t = threadIdx.x;
  const int a0 = g.cry_ptr[m.b];
  const int nb = g.cry_ptr[m.b + 1] - a0;
  const size_t prob = (size_t)m.b * g.n_q + m.qi;
  if (nb <= 0) {   // (uniform) empty by cry_ptr: nothing is written, as in phonon.hip
    if (t == 0) L.done[blockIdx.x] = 2;
    return;
  }
  if (nb > m.n) {   // cry_ptr gives the crystal more atoms than cry_ptr_host did: its region is too small (uniform)
    if (t == 0) {
      g.sweeps[prob] = 0;
      g.status[prob] = NNHIP_EIG_STATUS_SIZE;
      L.done[blockIdx.x] = 2;
    }
    return;
  }
  int bad_mass = 0;
  for (int i = t; i < nb; i += PH_THREADS) {
    const float ms = g.masses ? g.masses[a0 + i] : 1.f;
    bad_mass |= !(ms > 0.f && ms <= 3.4e38f);   // zero, negative, infinite or NaN
  }
  bad_mass = __syncthreads_or(bad_mass);
  if (t == 0) {
    g.sweeps[prob] = 0;
    g.status[prob] = bad_mass ? NNHIP_EIG_STATUS_MASS : 0;
    L.done[blockIdx.x] = bad_mass ? 2 : 0;
  }
}

// blockIdx.y: tile k <= l of the problem's Mp / 64 x Mp / 64 tiles
__global__ void __launch_bounds__(PH_THREADS)
phl_assemble_kernel(PhlArgs g, LArgs L) {
  __shared__ float2 wA[PHL_RCHUNK * PHL_TILE_ATOMS * PHL_TILE_ATOMS];   // w(i, (r, j)): i of the tile's rows, j of its columns
  __shared__ float2 wB[PHL_RCHUNK * PHL_TILE_ATOMS * PHL_TILE_ATOMS];   // w(j, (r, i))
  __shared__ double rsI[PHL_TILE_ATOMS], rsJ[PHL_TILE_ATOMS];
  if (L.done[blockIdx.x]) return;   // (uniform)
  const LProb m = L.tab[blockIdx.x];
  const int Mp = m.mp;
  int k, l;
  if (!upper_tile(blockIdx.y, Mp / PHL_S, false, k, l)) return;
  const int t = threadIdx.x;
  const int ti = t >> 4, tj = t & 15;
  const int b = m.b;
  const int a0 = g.cry_ptr[b];
  const int n = g.cry_ptr[b + 1] - a0;   // (0 < n <= m.n: prepare checked it)
  const int M = 3 * n;
  float* Are = reinterpret_cast<float*>(L.ws + m.base);
  float* Aim = reinterpret_cast<float*>(L.ws + m.base + off_aim(Mp));
  float* Wre = reinterpret_cast<float*>(L.ws + m.base + off_w(Mp));
  float* Wim = Wre + (size_t)Mp * Mp;
  float2* dm = g.dmat ? reinterpret_cast<float2*>(g.dmat) + (size_t)g.n_q * g.out_ptr[b] + (size_t)m.qi * M * M : nullptr;
  // the atoms the tile touches: rows [i0, i0 + ni), columns [j0, j0 + nj) (none when the tile is all padding)
  const int ra = k * PHL_S, ca = l * PHL_S;
  const int i0 = ra / 3, j0 = ca / 3;
  const int rlast = ra + PHL_S - 1 < M - 1 ? ra + PHL_S - 1 : M - 1, clast = ca + PHL_S - 1 < M - 1 ? ca + PHL_S - 1 : M - 1;
  const int ni = rlast >= ra ? rlast / 3 - i0 + 1 : 0, nj = clast >= ca ? clast / 3 - j0 + 1 : 0;
  float sre[4][4], sim[4][4], tre[4][4], tim[4][4];   // the sums of D_ac and of D_ca
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) sre[x][y] = sim[x][y] = tre[x][y] = tim[x][y] = 0.f;
  if (ni > 0 && nj > 0) {   // (uniform)
    if (t < ni) rsI[t] = ph_rsm(g.masses, a0 + i0 + t);
    if (t < nj) rsJ[t] = ph_rsm(g.masses, a0 + j0 + t);
    __syncthreads();
    const int N = g.sc_atoms[b];
    const int nR = N / n;
    const float* fc = g.fc + g.fc_ptr[b];
    const int* ist = g.img_start + g.img_ptr[b];
    const double q0 = g.q[3 * (size_t)m.qi], q1 = g.q[3 * (size_t)m.qi + 1], q2 = g.q[3 * (size_t)m.qi + 2];
    const int nij = ni * nj;
    for (int R0 = 0; R0 < nR; R0 += PHL_RCHUNK) {
      const int rc = nR - R0 < PHL_RCHUNK ? nR - R0 : PHL_RCHUNK;
      __syncthreads();   // (the chunk before has been read)
      for (int x = t; x < 2 * rc * nij; x += PH_THREADS) {
        const int half = x / (rc * nij), y = x - half * rc * nij;
        const int r = y / nij, rem = y - r * nij;
        const int i = rem / nj, j = rem - i * nj;
        if (half == 0)
          wA[y] = ph_weight(ist, g.img_off, (size_t)(i0 + i) * N + (size_t)(R0 + r) * n + j0 + j, q0, q1, q2);
        else
          wB[y] = ph_weight(ist, g.img_off, (size_t)(j0 + j) * N + (size_t)(R0 + r) * n + i0 + i, q0, q1, q2);
      }
      __syncthreads();
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int a = ra + ti + 16 * x;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          const int c = ca + tj + 16 * y;
          if (a >= M || c >= M || (k == l && a > c)) continue;
          const int i = a / 3, j = c / 3, alpha = a - 3 * i, beta = c - 3 * j;
          const int w = (i - i0) * nj + (j - j0);
          ph_accumulate(fc + ((size_t)a * N + (size_t)R0 * n + j) * 3 + beta, n, wA + w, nij, rc, sre[x][y], sim[x][y]);
          ph_accumulate(fc + ((size_t)c * N + (size_t)R0 * n + i) * 3 + alpha, n, wB + w, nij, rc, tre[x][y], tim[x][y]);
        }
      }
    }
  }
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int a = ra + ti + 16 * x;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int c = ca + tj + 16 * y;
      if (k == l && a > c) continue;   // the thread of (c, a) writes this element
      float re = 0.f, im = 0.f;
      const bool real_el = a < M && c < M;
      if (real_el) {
        const float f = (float)(rsI[a / 3 - i0] * rsJ[c / 3 - j0]);
        ph_hermitian(sre[x][y], sim[x][y], tre[x][y], tim[x][y], f, a == c, re, im);
      }
      const size_t ac = (size_t)a * Mp + c, cam = (size_t)c * Mp + a;
      Are[ac] = re;
      Aim[ac] = im;
      Are[cam] = re;
      Aim[cam] = real_el ? -im : 0.f;
      if (real_el && dm) {
        dm[(size_t)a * M + c] = make_float2(re, im);
        dm[(size_t)c * M + a] = make_float2(re, -im);
      }
      if (L.want_v) {
        Wre[ac] = a == c ? 1.f : 0.f;
        Wim[ac] = 0.f;
        Wre[cam] = a == c ? 1.f : 0.f;
        Wim[cam] = 0.f;
      }
    }
  }
}

// before sweep `it` (0-based): done when the stopping rule holds; at it == EIG_MAX_SWEEPS the cap is hit
__global__ void __launch_bounds__(PH_THREADS)
phl_converge_kernel(PhlArgs g, LArgs L, int it) {
  __shared__ double red[EIG_THREADS];
  if (L.done[blockIdx.x]) return;   // (uniform)
  const LProb m = L.tab[blockIdx.x];
  const int Mp = m.mp;
  const float* Are = reinterpret_cast<const float*>(L.ws + m.base);
  const float* Aim = reinterpret_cast<const float*>(L.ws + m.base + off_aim(Mp));
  double off = 0.0, diag = 0.0;
  for (int e = threadIdx.x; e < Mp * Mp; e += PH_THREADS) {
    const int i = e / Mp, j = e - i * Mp;
    const double re = (double)Are[e], im = (double)Aim[e];
    const double v = re * re + im * im;
    if (i == j) diag += v; else off += v;
  }
  off = block_sum(off, red);
  diag = block_sum(diag, red);
  const bool converged = off <= EIG_EPS2 * (off + diag) && off + diag <= 1.7976931348623157e308;
  if (threadIdx.x == 0) {
    const size_t prob = (size_t)m.b * g.n_q + m.qi;
    if (converged) {
      L.done[blockIdx.x] = 1;
    } else if (it == EIG_MAX_SWEEPS) {
      L.done[blockIdx.x] = 1;
      g.status[prob] = NNHIP_EIG_STATUS_SWEEPS;
    } else {
      g.sweeps[prob] = it + 1;   // the sweep that follows
    }
  }
}

// LDS of the pair solve: the scratch of ph_jacobi for Mp = 64 and four planes
#define PHL_PAIR_LDS (8 * 2 * PHL_S + 16 * PHL_B + 4 * PHL_S + 4 * PHL_S + 2 * (PHL_B * (PHL_B + 1) / 2) + 4 * 4 * PHL_PLANE)

__global__ void __launch_bounds__(PH_THREADS)
phl_pair_kernel(LArgs L, int s) {
  extern __shared__ __align__(16) char phl_smem[];
  if (L.done[blockIdx.x]) return;   // (uniform)
  const LProb m = L.tab[blockIdx.x];
  const int nblk = m.mp / PHL_B;
  const int k = blockIdx.y;
  if (s >= nblk - 1 || k >= nblk / 2) return;
  double* rowo = reinterpret_cast<double*>(phl_smem);         // [64]
  double* rowd = rowo + PHL_S;                                // [64]
  float4* cst = reinterpret_cast<float4*>(rowd + PHL_S);      // [32]
  float* dlt = reinterpret_cast<float*>(cst + PHL_B);         // [64] (ph_jacobi uses 32)
  float* dgs = dlt + PHL_S;                                   // [64]
  float* Are = dgs + PHL_S;
  float* Aim = Are + PHL_PLANE;
  float* Wre = Aim + PHL_PLANE;
  float* Wim = Wre + PHL_PLANE;
  unsigned short* tab = reinterpret_cast<unsigned short*>(Wim + PHL_PLANE);   // [32 x 33 / 2]
  const int t = threadIdx.x;
  const int ld = m.mp;
  float* Gre = reinterpret_cast<float*>(L.ws + m.base);
  float* Gim = reinterpret_cast<float*>(L.ws + m.base + off_aim(m.mp));
  int p, q;
  rr_pair(k, s, nblk, p, q);
  for (int e = t; e < PHL_S * PHL_S; e += PH_THREADS) {
    const int i = e / PHL_S, j = e - i * PHL_S;
    const size_t ge = (size_t)sub_coord(i, p, q) * ld + sub_coord(j, p, q);
    Are[i * PHL_LD + j] = Gre[ge];
    Aim[i * PHL_LD + j] = Gim[ge];
  }
  for (int e = t; e < PHL_B * PHL_B; e += PH_THREADS) {
    const int kk = e / PHL_B, ll = e - kk * PHL_B;
    if (kk <= ll) tab[kk * PHL_B - kk * (kk - 1) / 2 + (ll - kk)] = (unsigned short)(kk | ll << 8);
  }
  __syncthreads();
  bool converged;   // (not used: a sub-problem short of the rule is met again in the next sweep)
  ph_jacobi<false>(Are, Aim, Wre, Wim, PHL_S, PHL_LD, rowo, rowd, cst, dlt, tab, true, PHL_INNER_EPS2, PHL_INNER_SWEEPS, t, converged);
  // W as accumulated from fp32 rotations is unitary to about 3 x 64 x 2^-24 only, while the diagonal is an order of magnitude better.
  // The modes are a product of some (nblk - 1) x sweeps such factors, so each is brought back to the nearest unitary matrix by one
  // Newton-Schulz step  W <- W - E W / 2,  E = W W^H - I  (= W (3 I - W^H W) / 2; fp64 accumulation, fixed order) before it is used.
  __syncthreads();
  if (t < PHL_S) dgs[t] = Are[t * PHL_LD + t];
  __syncthreads();
  for (int e = t; e < PHL_S * PHL_S; e += PH_THREADS) {
    const int i = e / PHL_S, j = e - i * PHL_S;
    double gr = 0.0, gi = 0.0;
    for (int mm = 0; mm < PHL_S; ++mm) {
      const double ar = (double)Wre[i * PHL_LD + mm], ai = (double)Wim[i * PHL_LD + mm];
      const double br = (double)Wre[j * PHL_LD + mm], bi = (double)Wim[j * PHL_LD + mm];
      gr += ar * br + ai * bi;
      gi += ai * br - ar * bi;
    }
    Are[i * PHL_LD + j] = (float)(gr - (i == j ? 1.0 : 0.0));
    Aim[i * PHL_LD + j] = (float)gi;
  }
  __syncthreads();
  float* Qre = reinterpret_cast<float*>(L.ws + m.base + off_q(m.mp, L.want_v)) + (size_t)k * 2 * PHL_S * PHL_S;
  float* Qim = Qre + PHL_S * PHL_S;
  for (int e = t; e < PHL_S * PHL_S; e += PH_THREADS) {
    const int i = e / PHL_S, j = e - i * PHL_S;
    float ar = 0.f, ai = 0.f;
    for (int mm = 0; mm < PHL_S; ++mm) {
      const float er = Are[i * PHL_LD + mm], ei = Aim[i * PHL_LD + mm];
      const float wr = Wre[mm * PHL_LD + j], wi = Wim[mm * PHL_LD + j];
      ar = fmaf(er, wr, ar);
      ar = fmaf(-ei, wi, ar);
      ai = fmaf(er, wi, ai);
      ai = fmaf(ei, wr, ai);
    }
    Qre[e] = fmaf(-0.5f, ar, Wre[i * PHL_LD + j]);      // Qt = conj(W)
    Qim[e] = -fmaf(-0.5f, ai, Wim[i * PHL_LD + j]);
    const size_t ge = (size_t)sub_coord(i, p, q) * ld + sub_coord(j, p, q);
    Gre[ge] = i == j ? dgs[i] : 0.f;
    Gim[ge] = 0.f;
  }
}

// acc[a][c] = sum_m X(i_a, m) Y(m, j_c), i_a = ti + 16 a, j_c = tj + 16 c, m ascending, complex in two planes.
// kForm 0: X Y;  1: X Y^H (Y(m, j) = conj(Ys[j][m]));  2: conj(X) Y
template <int kForm>
__device__ __forceinline__ void ctile_product(const float* Xr, const float* Xi, const float* Yr, const float* Yi, int ti, int tj,
                                              float accr[4][4], float acci[4][4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) accr[a][c] = acci[a][c] = 0.f;
  for (int mm = 0; mm < PHL_S; ++mm) {
    float xr[4], xi[4], yr[4], yi[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      xr[a] = Xr[(ti + 16 * a) * PHL_LD + mm];
      xi[a] = Xi[(ti + 16 * a) * PHL_LD + mm];
      if (kForm == 2) xi[a] = -xi[a];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int at = kForm == 1 ? (tj + 16 * c) * PHL_LD + mm : mm * PHL_LD + tj + 16 * c;
      yr[c] = Yr[at];
      yi[c] = kForm == 1 ? -Yi[at] : Yi[at];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        accr[a][c] = fmaf(xr[a], yr[c], accr[a][c]);
        accr[a][c] = fmaf(-xi[a], yi[c], accr[a][c]);
        acci[a][c] = fmaf(xr[a], yi[c], acci[a][c]);
        acci[a][c] = fmaf(xi[a], yr[c], acci[a][c]);
      }
  }
}

#define PHL_UPDATE_LDS (4 * 6 * PHL_PLANE)

// blockIdx.y < n_at: tile k < l of A;  else (modes): rows of pair k x 64-column chunk of W.  n_at / p_max: grid decoding (batch-wide,
// no arithmetic depends on them)
__global__ void __launch_bounds__(PH_THREADS)
phl_update_kernel(LArgs L, int s, int n_at, int p_max) {
  extern __shared__ __align__(16) char phl_smem[];
  if (L.done[blockIdx.x]) return;   // (uniform)
  const LProb m = L.tab[blockIdx.x];
  const int nblk = m.mp / PHL_B;
  const int P = nblk / 2;
  if (s >= nblk - 1) return;
  float* S0 = reinterpret_cast<float*>(phl_smem);
  float* S1 = S0 + PHL_PLANE;
  float* S2 = S1 + PHL_PLANE;
  float* S3 = S2 + PHL_PLANE;
  float* S4 = S3 + PHL_PLANE;
  float* S5 = S4 + PHL_PLANE;
  const int t = threadIdx.x;
  const int ti = t >> 4, tj = t & 15;
  const int ld = m.mp;
  const float* Qall = reinterpret_cast<const float*>(L.ws + m.base + off_q(m.mp, L.want_v));
  float accr[4][4], acci[4][4];
  if ((int)blockIdx.y < n_at) {
    int k, l;
    if (!upper_tile(blockIdx.y, P, true, k, l)) return;
    int pk, qk, pl, ql;
    rr_pair(k, s, nblk, pk, qk);
    rr_pair(l, s, nblk, pl, ql);
    float* Are = reinterpret_cast<float*>(L.ws + m.base);
    float* Aim = reinterpret_cast<float*>(L.ws + m.base + off_aim(m.mp));
    const float* Qk = Qall + (size_t)k * 2 * PHL_S * PHL_S;
    const float* Ql = Qall + (size_t)l * 2 * PHL_S * PHL_S;
    for (int e = t; e < PHL_S * PHL_S; e += PH_THREADS) {
      const int i = e / PHL_S, j = e - i * PHL_S;
      const int at = i * PHL_LD + j;
      S0[at] = Qk[e];
      S1[at] = Qk[PHL_S * PHL_S + e];
      S4[at] = Ql[e];
      S5[at] = Ql[PHL_S * PHL_S + e];
      const size_t ge = (size_t)sub_coord(i, pk, qk) * ld + sub_coord(j, pl, ql);
      S2[at] = Are[ge];
      S3[at] = Aim[ge];
    }
    __syncthreads();
    ctile_product<0>(S0, S1, S2, S3, ti, tj, accr, acci);   // R = Qt_k T
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        S2[(ti + 16 * a) * PHL_LD + tj + 16 * c] = accr[a][c];
        S3[(ti + 16 * a) * PHL_LD + tj + 16 * c] = acci[a][c];
      }
    __syncthreads();
    ctile_product<1>(S2, S3, S4, S5, ti, tj, accr, acci);   // N = R Qt_l^H
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const size_t gi = sub_coord(ti + 16 * a, pk, qk);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t gj = sub_coord(tj + 16 * c, pl, ql);
        Are[gi * ld + gj] = accr[a][c];
        Aim[gi * ld + gj] = acci[a][c];
        Are[gj * ld + gi] = accr[a][c];
        Aim[gj * ld + gi] = -acci[a][c];
      }
    }
  } else {
    const int v = blockIdx.y - n_at;
    const int k = v / p_max, ch = v - k * p_max;
    if (!L.want_v || k >= P || ch >= P) return;   // (mp / 64 = P column chunks)
    int pk, qk;
    rr_pair(k, s, nblk, pk, qk);
    float* Wre = reinterpret_cast<float*>(L.ws + m.base + off_w(m.mp));
    float* Wim = Wre + (size_t)m.mp * m.mp;
    const float* Qk = Qall + (size_t)k * 2 * PHL_S * PHL_S;
    for (int e = t; e < PHL_S * PHL_S; e += PH_THREADS) {
      const int i = e / PHL_S, j = e - i * PHL_S;
      const int at = i * PHL_LD + j;
      S0[at] = Qk[e];
      S1[at] = Qk[PHL_S * PHL_S + e];
      const size_t ge = (size_t)sub_coord(i, pk, qk) * ld + ch * PHL_S + j;
      S2[at] = Wre[ge];
      S3[at] = Wim[ge];
    }
    __syncthreads();
    ctile_product<2>(S0, S1, S2, S3, ti, tj, accr, acci);   // conj(Qt_k) x rows
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t ge = (size_t)sub_coord(ti + 16 * a, pk, qk) * ld + ch * PHL_S + tj + 16 * c;
        Wre[ge] = accr[a][c];
        Wim[ge] = acci[a][c];
      }
  }
}

__global__ void __launch_bounds__(PH_THREADS)
phl_finish_kernel(PhlArgs g, LArgs L) {
  __shared__ float dg[PHL_MAX_DIM];
  __shared__ int rank[PHL_MAX_DIM];
  __shared__ float2 phs[PHL_MAX_DIM];
  if (L.done[blockIdx.x] != 1) return;   // (uniform) 2: not computed, its outputs keep what the caller put there
  const LProb m = L.tab[blockIdx.x];
  const int t = threadIdx.x;
  const int a0 = g.cry_ptr[m.b];
  const int M = 3 * (g.cry_ptr[m.b + 1] - a0);   // (<= 3 m.n <= PHL_MAX_DIM: prepare checked it)
  const int ld = m.mp;
  const float* Are = reinterpret_cast<const float*>(L.ws + m.base);
  const float* Wre = reinterpret_cast<const float*>(L.ws + m.base + off_w(m.mp));
  const float* Wim = Wre + (size_t)m.mp * m.mp;
  const bool want_v = L.want_v != 0;
  for (int i = t; i < M; i += PH_THREADS) dg[i] = Are[(size_t)i * ld + i];
  __syncthreads();
  float* evals = g.evals + (size_t)g.n_q * 3 * a0 + (size_t)m.qi * M;
  for (int i = t; i < M; i += PH_THREADS) {
    const float di = dg[i];
    int r = 0;
    for (int j = 0; j < M; ++j) {
      const float dj = dg[j];
      r += dj < di || (dj == di && j < i) ? 1 : 0;
    }
    rank[i] = r;
    evals[r] = di;
    if (want_v) phs[i] = ph_phase(Wre + (size_t)i * ld, Wim + (size_t)i * ld, M);
  }
  if (want_v) {
    __syncthreads();
    float2* out = reinterpret_cast<float2*>(g.modes) + (size_t)g.n_q * g.out_ptr[m.b] + (size_t)m.qi * M * M;
    for (int e = t; e < M * M; e += PH_THREADS) {
      const int i = e / M, j = e - i * M;
      const float2 f = phs[i];
      const float vr = Wre[(size_t)i * ld + j], vi = Wim[(size_t)i * ld + j];
      out[(size_t)rank[i] * M + j] = make_float2(f.x * vr - f.y * vi, f.x * vi + f.y * vr);
    }
  }
}

// the problems of the selected crystals with atoms, crystal by crystal and q ascending, their regions laid out in order; returns 0 or
// the error code (message set)
int plan(const char* who, const int32_t* cry_ptr_host, int n_cry, int n_q, const uint8_t* select_host, int want_v, bool fill,
         std::vector<LProb>& probs, size_t& n_prob, size_t& total) {
  n_prob = 0;
  for (int b = 0; b < n_cry; ++b) {
    const int n = cry_ptr_host[b + 1] - cry_ptr_host[b];
    if (n < 0) {
      nnhip_set_error("%s: cry_ptr_host decreases at crystal %d", who, b);
      return NNHIP_E_INVALID;
    }
    if (select_host && !select_host[b]) continue;
    if (3 * (long)n > PHL_MAX_DIM) {
      nnhip_set_error("%s: crystal %d has dimension 3 x %d = %ld, above the supported %d (nnhip_phonon_large_max_dim)", who, b, n,
                      3 * (long)n, PHL_MAX_DIM);
      return NNHIP_E_UNSUPPORTED;
    }
    if (n > 0) n_prob += (size_t)n_q;
  }
  if (n_prob > 0x7fffffff) {
    nnhip_set_error("%s: %zu (crystal, wave vector) problems in one call, above the 2^31 - 1 a launch addresses", who, n_prob);
    return NNHIP_E_UNSUPPORTED;
  }
  total = header_bytes(n_prob);
  probs.clear();
  for (int b = 0; b < n_cry; ++b) {
    const int n = cry_ptr_host[b + 1] - cry_ptr_host[b];
    if (n <= 0 || (select_host && !select_host[b])) continue;
    LProb m;
    m.b = b;
    m.mp = pad_order(3 * n);
    m.n = n;
    const size_t rb = region_bytes(m.mp, want_v);
    if (fill) {
      for (int qi = 0; qi < n_q; ++qi) {
        m.base = total + (size_t)qi * rb;
        m.qi = qi;
        probs.push_back(m);
      }
    }
    total += (size_t)n_q * rb;
  }
  return NNHIP_OK;
}

}  // namespace

extern "C" int nnhip_phonon_large_max_dim(void) { return PHL_MAX_DIM; }

extern "C" size_t nnhip_phonon_large_ws_bytes(const int32_t* cry_ptr_host, int32_t n_cry, int32_t n_q, int32_t want_modes,
                                              const uint8_t* select_host) {
  if (!cry_ptr_host || n_cry <= 0 || n_q <= 0) return 0;
  std::vector<LProb> probs;
  size_t n_prob = 0, total = 0;
  if (plan("nnhip_phonon_large_ws_bytes", cry_ptr_host, n_cry, n_q, select_host, want_modes ? 1 : 0, false, probs, n_prob, total) !=
      NNHIP_OK)
    return 0;
  return n_prob ? total : 0;
}

extern "C" int nnhip_phonon_bands_large(const float* fc, const int64_t* fc_ptr, const int32_t* cry_ptr, const int32_t* cry_ptr_host,
                                        const int32_t* sc_atoms, const int64_t* img_ptr, const int32_t* img_start,
                                        const double* img_off, const float* masses, const int64_t* out_ptr, int32_t n_cry,
                                        const double* q, int32_t n_q, float* evals, float* modes, float* dmat, int32_t* sweeps,
                                        int32_t* status, const uint8_t* select_host, void* ws, size_t ws_bytes, void* stream) {
  if (n_cry < 0 || n_q < 0 ||
      (n_cry > 0 && n_q > 0 && (!fc || !fc_ptr || !cry_ptr || !cry_ptr_host || !sc_atoms || !img_ptr || !img_start || !img_off ||
                                !out_ptr || !q || !evals || !sweeps || !status))) {
    nnhip_set_error("nnhip_phonon_bands_large: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_cry == 0 || n_q == 0) return NNHIP_OK;
  const int want_v = modes != nullptr;
  std::vector<LProb> probs;
  size_t n_prob_sz = 0, total = 0;
  const int rc = plan("nnhip_phonon_bands_large", cry_ptr_host, n_cry, n_q, select_host, want_v, true, probs, n_prob_sz, total);
  if (rc != NNHIP_OK) return rc;
  const int n_prob = (int)n_prob_sz;
  if (n_prob == 0) return NNHIP_OK;
  if (!ws || ws_bytes < total || (reinterpret_cast<uintptr_t>(ws) & 255)) {
    nnhip_set_error("nnhip_phonon_bands_large: workspace of %zu bytes, 256-byte aligned, needed (got %zu)", total, ws_bytes);
    return NNHIP_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  PhlArgs g;
  g.fc = fc;
  g.fc_ptr = fc_ptr;
  g.cry_ptr = cry_ptr;
  g.sc_atoms = sc_atoms;
  g.img_ptr = img_ptr;
  g.img_start = img_start;
  g.img_off = img_off;
  g.masses = masses;
  g.q = q;
  g.out_ptr = out_ptr;
  g.evals = evals;
  g.modes = modes;
  g.dmat = dmat;
  g.sweeps = sweeps;
  g.status = status;
  g.n_q = n_q;
  LArgs L;
  L.ws = static_cast<char*>(ws);
  L.tab = reinterpret_cast<const LProb*>(ws);
  L.done = reinterpret_cast<int*>(L.ws + round256((size_t)n_prob * sizeof(LProb)));
  L.want_v = want_v;
  int p_all = 0;
  for (int i = 0; i < n_prob; ++i) p_all = probs[i].mp / PHL_S > p_all ? probs[i].mp / PHL_S : p_all;
  // above the default limit a kernel has to ask for its dynamic LDS
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(phl_pair_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, PHL_PAIR_LDS));
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(phl_update_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              PHL_UPDATE_LDS));
  // the table goes to the device from pageable memory; `probs` outlives the copy (the loop below waits for the stream)
  HIP_TRY(hipMemcpyAsync(ws, probs.data(), (size_t)n_prob * sizeof(LProb), hipMemcpyHostToDevice, st));
  phl_prepare_kernel<<<n_prob, PH_THREADS, 0, st>>>(g, L);
  LAUNCH_CHECK();
  phl_assemble_kernel<<<dim3(n_prob, p_all * (p_all + 1) / 2), PH_THREADS, 0, st>>>(g, L);
  LAUNCH_CHECK();
  std::vector<int> done((size_t)n_prob, 0);
  for (int it = 0; it <= EIG_MAX_SWEEPS; ++it) {
    phl_converge_kernel<<<n_prob, PH_THREADS, 0, st>>>(g, L, it);
    LAUNCH_CHECK();
    // the one read-back per sweep: this path is not the steady-state inference step
    HIP_TRY(hipMemcpyAsync(done.data(), L.done, (size_t)n_prob * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int p_max = 0;   // over the problems still iterating: sizes the grids only
    for (int i = 0; i < n_prob; ++i)
      if (!done[i]) p_max = probs[i].mp / PHL_S > p_max ? probs[i].mp / PHL_S : p_max;
    if (p_max == 0) break;   // (it == EIG_MAX_SWEEPS sets every flag)
    const int n_at = p_max * (p_max - 1) / 2;
    const int n_up = n_at + (want_v ? p_max * p_max : 0);
    for (int s = 0; s < 2 * p_max - 1; ++s) {
      phl_pair_kernel<<<dim3(n_prob, p_max), PH_THREADS, PHL_PAIR_LDS, st>>>(L, s);
      LAUNCH_CHECK();
      if (n_up > 0) {
        phl_update_kernel<<<dim3(n_prob, n_up), PH_THREADS, PHL_UPDATE_LDS, st>>>(L, s, n_at, p_max);
        LAUNCH_CHECK();
      }
    }
  }
  phl_finish_kernel<<<n_prob, PH_THREADS, 0, st>>>(g, L);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
