// Batched phonon dispersion (gfx950, fp32): every (crystal, wave vector) problem of a batch in ONE launch.
//
// newtonnet_amd/phonons.py leaves per crystal the force constants Phi(i, J) of its n_b home atoms against the N_b atoms of a
// supercell, packed [n_b][3][N_b][3] (supercell atom J = R n_b + j: copy R of home atom j, the home cell R = 0 first), and an
// image table: for every (i, J) the m_iJ equally near supercell-lattice images of J as seen from i, each as its offset
// x = frac(r_J + T - r_i) in units of the PRIMITIVE lattice vectors (fp64).  A problem (b, q), d = 3 n_b, does:
//   1. D(q) in LDS.  w(i, J) = (1 / m_iJ) sum_T exp(2 pi i q_frac . x) with the product q_frac . x formed in fp64, reduced to
//      [-1/2, 1/2) and handed to sincospi (the phase never leaves fp64 before the sine and cosine), for a chunk of 8 copies R at a
//      time (the chunk shares its LDS with the eigenvectors, which are not needed yet); then the thread of element (i a, j b) adds
//      Phi(i a, (R, j) b) w(i, (R, j)) for R ascending (fmaf, fp32) -- the order of every sum is fixed by the element alone.
//      D_ij <- (D_ij + conj(D_ji)) / 2 / sqrt(m_i m_j), tile and mirror written by one thread: exactly Hermitian.  dmat != null
//      receives it as complex64 [d][d].
//   2. cyclic Jacobi for a complex Hermitian matrix with the round-robin ordering, the rotation formulas and the stopping rule of
//      csrc/eig_common.h (off^2 <= EIG_EPS2 ||A||_F^2 summed in fp64, EIG_MAX_SWEEPS, status bit 0).  The rotation of pair (p, q)
//      is U = P R: P = diag(1, conj(u)) with u = a_pq / |a_pq| makes a_pq real, R is the real rotation of eig.hip for
//      (a_pp, a_qq, |a_pq|).  A <- U^H A U in 2 x 2 tiles k <= l, each written with its conjugate mirror image by one thread;
//      W = U^T (row k = mode k) takes the same row operations with conj(u).  Real and imaginary parts live in separate planes
//      with the odd row stride Mp + 1, so the column walks of the tiles hit distinct banks as in eig.hip.  off^2 and ||A||_F^2
//      are summed row by row and then over the rows, each serially: the sums -- and so the sweep count -- do not depend on how
//      many threads serve the problem.
//   3. rank the eigenvalues by counting (index as tie-break), fix each mode's phase (the component of largest magnitude real and
//      positive, lowest index on a tie), write.
// Packing: a crystal with Mp <= 32 gives every problem ONE wave, four problems per workgroup, synchronised by wave barriers
// only (the waves of a workgroup never meet); a larger one takes the whole workgroup of 256 threads (a crystal that the host
// offsets left without LDS in either form is flagged for every wave vector and not computed).  The choice is a function
// of the crystal's own size, and no sum depends on the thread count, so the result of a (b, q) depends neither on the packing
// nor on what else is in the launch.  No float atomics: two calls are bitwise equal.  modes == null skips W; A's arithmetic does
// not read W, so the eigenvalues keep every bit.
// LDS of a problem with modes: 4 planes of Mp (Mp + 1) floats + 48 Mp bytes of vectors + the tile table: 155 952 bytes at
// d = 96 (32 atoms), the largest multiple of 3 that fits the 160 KiB of a CU (d = 99 needs 168 950).
#include "eig_common.h"   // rr_pair, EIG_EPS2, EIG_MAX_SWEEPS: one statement of the ordering and of the stopping rule

#define PH_THREADS 256
#define PH_MAX_DIM 96
#define PH_WAVE_DIM 32     // Mp up to which a problem is served by one wave
#define PH_RCHUNK 8        // supercell copies whose phase factors are staged at a time

namespace {

struct PhArgs {
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
  int n_q, cap_big, cap_wave;
  unsigned slot_wave;
};

__host__ __device__ inline size_t ph_x_bytes(int cap, bool want_v) {
  const size_t nc = (size_t)cap / 3 + 1;
  const size_t v = want_v ? 8 * (size_t)cap * (cap + 1) : 0, w = 8 * (size_t)PH_RCHUNK * nc * nc;
  return v > w ? v : w;
}

// bytes of one problem's LDS for matrices of up to cap (even) coordinates, a multiple of 16
__host__ __device__ inline size_t ph_slot_bytes(int cap, bool want_v) {
  const int p = cap / 2;
  const size_t b = 16 * (size_t)cap      // rowo, rowd (fp64)
                   + 8 * (size_t)cap     // cst  [cap / 2] float4
                   + 16 * (size_t)cap    // dlt, dg, rank, (spare)
                   + 8 * (size_t)cap     // phs  [cap] float2
                   + 8 * (size_t)cap * (cap + 1)   // Are, Aim
                   + ph_x_bytes(cap, want_v) + 2 * (size_t)(p * (p + 1) / 2);
  return (b + 15) & ~(size_t)15;
}

template <bool ONE_WAVE>
__device__ __forceinline__ void ph_sync() {
  if (ONE_WAVE) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the wave's LDS writes are done and not moved across
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// one problem (crystal b, wave vector qi) on T = 64 (ONE_WAVE) or PH_THREADS threads, thread index t, in the LDS slot `smem` sized for cap
template <bool ONE_WAVE>
__device__ __forceinline__ void ph_problem(const PhArgs& g, int b, int qi, char* smem, int cap, int t) {
  constexpr int T = ONE_WAVE ? 64 : PH_THREADS;
  const int a0 = g.cry_ptr[b];
  const int n = g.cry_ptr[b + 1] - a0;
  const int M = 3 * n;
  const int Mp = (M + 1) & ~1;
  const int P = Mp >> 1;
  const int ld = Mp + 1;
  const size_t prob = (size_t)b * g.n_q + qi;
  if (Mp > cap) {   // cry_ptr and cry_ptr_host disagree: this launch's LDS is too small for the crystal (uniform)
    if (t == 0) {
      g.sweeps[prob] = 0;
      g.status[prob] = NNHIP_EIG_STATUS_SIZE;
    }
    return;
  }
  int bad_mass = 0;
  for (int i = 0; i < n; ++i) {
    const float m = g.masses ? g.masses[a0 + i] : 1.f;
    bad_mass |= !(m > 0.f && m <= 3.4e38f);
  }
  if (bad_mass) {   // (uniform: every thread looked at every mass)
    if (t == 0) {
      g.sweeps[prob] = 0;
      g.status[prob] = NNHIP_EIG_STATUS_MASS;
    }
    return;
  }
  const bool want_v = g.modes != nullptr;
  double* rowo = reinterpret_cast<double*>(smem);          // [cap] off^2 per row; 1 / sqrt(m_i) during the assembly
  double* rowd = rowo + cap;                               // [cap] diagonal^2 per row
  float4* cst = reinterpret_cast<float4*>(rowd + cap);     // [cap / 2] (c, s, Re u, Im u) of the step's pairs
  float* dlt = reinterpret_cast<float*>(cst + cap / 2);    // [cap] t |a_pq| of the step's pairs
  float* dg = dlt + cap;                                   // [cap] eigenvalues before sorting
  int* rank = reinterpret_cast<int*>(dg + cap);            // [cap]
  float2* phs = reinterpret_cast<float2*>(rank + 2 * cap); // [cap] phase factor of each mode
  float* Are = reinterpret_cast<float*>(phs + cap);        // [cap][cap + 1] (this problem uses [Mp][ld])
  float* Aim = Are + (size_t)cap * (cap + 1);
  float* Wre = Aim + (size_t)cap * (cap + 1);              // W = U^T when modes are wanted ...
  float* Wim = Wre + (size_t)Mp * ld;
  float2* wch = reinterpret_cast<float2*>(Wre);            // ... and before that the phase factors of a chunk [r][i][j]
  unsigned short* tab = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(Wre) + ph_x_bytes(cap, want_v));
  for (int e = t; e < P * P; e += T) {
    const int k = e / P, l = e - k * P;
    if (k <= l) tab[k * P - k * (k - 1) / 2 + (l - k)] = (unsigned short)(k | l << 8);
  }

  // ---- 1. D(q) ------------------------------------------------------------------------------------------------------------
  for (int e = t; e < Mp * Mp; e += T) {
    const int i = e / Mp, j = e - i * Mp;
    Are[i * ld + j] = 0.f;
    Aim[i * ld + j] = 0.f;
  }
  for (int i = t; i < n; i += T) rowo[i] = 1.0 / sqrt((double)(g.masses ? g.masses[a0 + i] : 1.f));
  ph_sync<ONE_WAVE>();
  const int N = g.sc_atoms[b];
  const int nR = N / n;
  const float* fc = g.fc + g.fc_ptr[b];
  const int* ist = g.img_start + g.img_ptr[b];
  const double q0 = g.q[3 * (size_t)qi], q1 = g.q[3 * (size_t)qi + 1], q2 = g.q[3 * (size_t)qi + 2];
  for (int R0 = 0; R0 < nR; R0 += PH_RCHUNK) {
    const int rc = nR - R0 < PH_RCHUNK ? nR - R0 : PH_RCHUNK;
    for (int x = t; x < rc * n * n; x += T) {
      const int r = x / (n * n), rem = x - r * n * n;
      const int i = rem / n, j = rem - i * n;
      const size_t ij = (size_t)i * N + (size_t)(R0 + r) * n + j;
      const int k0 = ist[ij], k1 = ist[ij + 1];
      double sr = 0.0, si = 0.0;
      for (int k = k0; k < k1; ++k) {
        double ph = q0 * g.img_off[3 * (size_t)k] + q1 * g.img_off[3 * (size_t)k + 1] + q2 * g.img_off[3 * (size_t)k + 2];
        ph -= rint(ph);   // [-1/2, 1/2]
        double s, c;
        sincospi(2.0 * ph, &s, &c);
        sr += c;
        si += s;
      }
      const double inv = k1 > k0 ? 1.0 / (double)(k1 - k0) : 0.0;
      wch[x] = make_float2((float)(sr * inv), (float)(si * inv));
    }
    ph_sync<ONE_WAVE>();
    for (int e = t; e < M * M; e += T) {
      const int a = e / M, c = e - a * M;
      const int i = a / 3, j = c / 3, beta = c - 3 * j;
      float are = Are[a * ld + c], aim = Aim[a * ld + c];
      const float* f = fc + ((size_t)a * N + (size_t)R0 * n + j) * 3 + beta;
      for (int r = 0; r < rc; ++r) {
        const float phi = f[(size_t)r * n * 3];
        const float2 w = wch[(r * n + i) * n + j];
        are = fmaf(phi, w.x, are);
        aim = fmaf(phi, w.y, aim);
      }
      Are[a * ld + c] = are;
      Aim[a * ld + c] = aim;
    }
    ph_sync<ONE_WAVE>();
  }
  for (int e = t; e < M * M; e += T) {
    const int a = e / M, c = e - a * M;
    if (a > c) continue;   // the thread of (a, c), a <= c, writes both halves: D is exactly Hermitian from here on
    const float f = (float)(rowo[a / 3] * rowo[c / 3]);
    const float re = 0.5f * (Are[a * ld + c] + Are[c * ld + a]) * f;
    const float im = a == c ? 0.f : 0.5f * (Aim[a * ld + c] - Aim[c * ld + a]) * f;
    Are[a * ld + c] = re;
    Are[c * ld + a] = re;
    Aim[a * ld + c] = im;
    Aim[c * ld + a] = -im;
  }
  ph_sync<ONE_WAVE>();
  if (g.dmat) {
    float2* out = reinterpret_cast<float2*>(g.dmat) + (size_t)g.n_q * g.out_ptr[b] + (size_t)qi * M * M;
    for (int e = t; e < M * M; e += T) {
      const int a = e / M, c = e - a * M;
      out[e] = make_float2(Are[a * ld + c], Aim[a * ld + c]);
    }
  }

  // ---- 2. Jacobi ------------------------------------------------------------------------------------------------------------
  if (want_v) {
    for (int e = t; e < Mp * Mp; e += T) {
      const int i = e / Mp, j = e - i * Mp;
      Wre[i * ld + j] = i == j ? 1.f : 0.f;
      Wim[i * ld + j] = 0.f;
    }
  }
  const int n_tiles = P * (P + 1) / 2;
  int n_sweeps = 0;
  bool converged = false;
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
    converged = off <= EIG_EPS2 * (off + diag) && off + diag <= 1.7976931348623157e308;
    if (converged || n_sweeps == EIG_MAX_SWEEPS) break;   // (uniform: every thread holds the same sums)
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
  if (t == 0) {
    g.sweeps[prob] = n_sweeps;
    g.status[prob] = converged ? 0 : NNHIP_EIG_STATUS_SWEEPS;
  }

  // ---- 3. sort, fix phases, write ---------------------------------------------------------------------------------------
  for (int i = t; i < M; i += T) dg[i] = Are[i * ld + i];
  ph_sync<ONE_WAVE>();
  float* evals = g.evals + (size_t)g.n_q * 3 * a0 + (size_t)qi * M;
  for (int i = t; i < M; i += T) {
    const float di = dg[i];
    int r = 0;
    for (int j = 0; j < M; ++j) {
      const float dj = dg[j];
      r += dj < di || (dj == di && j < i) ? 1 : 0;
    }
    rank[i] = r;
    evals[r] = di;
    if (want_v) {
      float best = -1.f, fr = 1.f, fi = 0.f;
      for (int j = 0; j < M; ++j) {
        const float vr = Wre[i * ld + j], vi = Wim[i * ld + j];
        const float a2 = vr * vr + vi * vi;
        if (a2 > best) {
          best = a2;
          fr = vr;
          fi = vi;
        }
      }
      const float ab = hypotf(fr, fi);
      phs[i] = ab > 0.f ? make_float2(fr / ab, -fi / ab) : make_float2(1.f, 0.f);
    }
  }
  if (want_v) {
    ph_sync<ONE_WAVE>();
    float2* out = reinterpret_cast<float2*>(g.modes) + (size_t)g.n_q * g.out_ptr[b] + (size_t)qi * M * M;
    for (int e = t; e < M * M; e += T) {
      const int i = e / M, j = e - i * M;
      const float2 f = phs[i];
      const float vr = Wre[i * ld + j], vi = Wim[i * ld + j];
      out[(size_t)rank[i] * M + j] = make_float2(f.x * vr - f.y * vi, f.x * vi + f.y * vr);
    }
  }
}

__global__ void __launch_bounds__(PH_THREADS)
phonon_kernel(PhArgs g) {
  extern __shared__ __align__(16) char ph_smem[];
  const int b = blockIdx.y;
  const int n = g.cry_ptr[b + 1] - g.cry_ptr[b];
  if (n <= 0) return;   // (uniform)
  const int Mp = (3 * n + 1) & ~1;
  if (Mp <= PH_WAVE_DIM && Mp <= g.cap_wave) {   // one wave per problem: the four waves never synchronise with each other
    const int wave = threadIdx.x >> 6;
    const int qi = blockIdx.x * (PH_THREADS / 64) + wave;
    if (qi >= g.n_q) return;
    ph_problem<true>(g, b, qi, ph_smem + (size_t)wave * g.slot_wave, g.cap_wave, threadIdx.x & 63);
  } else if (Mp <= g.cap_big) {   // (cap_big > 0: the grid has a workgroup per wave vector)
    const int qi = blockIdx.x;
    if (qi >= g.n_q) return;
    ph_problem<false>(g, b, qi, ph_smem, g.cap_big, threadIdx.x);
  } else {
    // cry_ptr gives the crystal more atoms than cry_ptr_host did and neither form of this launch has the LDS for it.  The grid
    // may be that of the wave form alone (a workgroup per FOUR wave vectors), so the flags are not left to a workgroup per
    // problem: whatever the grid, every problem of the crystal is flagged, and nothing else of it is written.
    for (int qi = blockIdx.x * PH_THREADS + threadIdx.x; qi < g.n_q; qi += gridDim.x * PH_THREADS) {
      g.sweeps[(size_t)b * g.n_q + qi] = 0;
      g.status[(size_t)b * g.n_q + qi] = NNHIP_EIG_STATUS_SIZE;
    }
  }
}

// one thread per bin; the values of crystal b are x[val_ptr[b] .. val_ptr[b + 1]) and every thread walks them in that order
__global__ void __launch_bounds__(256)
phonon_dos_kernel(const float* __restrict__ x, const int64_t* __restrict__ val_ptr, float lo, float hi, int n_bins, float width,
                  int* __restrict__ counts, float* __restrict__ dens) {
  const int bin = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (bin >= n_bins) return;
  const int64_t v0 = val_ptr[b], v1 = val_ptr[b + 1];
  const float wbin = (hi - lo) / (float)n_bins;
  if (counts) {
    int c = 0;
    for (int64_t v = v0; v < v1; ++v) {
      const float f = x[v];
      if (!(f >= lo && f <= hi)) continue;   // outside the range, or NaN
      int k = (int)floorf((f - lo) / wbin);
      k = k > n_bins - 1 ? n_bins - 1 : k;   // f == hi, or the quotient rounded up to n_bins
      c += k == bin ? 1 : 0;
    }
    counts[(size_t)b * n_bins + bin] = c;
  }
  if (dens) {
    const float centre = lo + ((float)bin + 0.5f) * wbin;
    const float inv = 1.f / width;
    double s = 0.0;
    for (int64_t v = v0; v < v1; ++v) {
      const float u = (centre - x[v]) * inv;
      s += (double)expf(-0.5f * u * u);
    }
    dens[(size_t)b * n_bins + bin] = (float)(s * 0.3989422804014327 / (double)width);
  }
}

}  // namespace

extern "C" int nnhip_phonon_max_dim(void) { return PH_MAX_DIM; }

extern "C" int nnhip_phonon_bands(const float* fc, const int64_t* fc_ptr, const int32_t* cry_ptr, const int32_t* cry_ptr_host,
                                  const int32_t* sc_atoms, const int64_t* img_ptr, const int32_t* img_start, const double* img_off,
                                  const float* masses, const int64_t* out_ptr, int32_t n_cry, const double* q, int32_t n_q,
                                  float* evals, float* modes, float* dmat, int32_t* sweeps, int32_t* status, void* stream) {
  if (n_cry < 0 || n_q < 0 ||
      (n_cry > 0 && n_q > 0 && (!fc || !fc_ptr || !cry_ptr || !cry_ptr_host || !sc_atoms || !img_ptr || !img_start || !img_off ||
                                !out_ptr || !q || !evals || !sweeps || !status))) {
    nnhip_set_error("nnhip_phonon_bands: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_cry > 65535) {
    nnhip_set_error("nnhip_phonon_bands: %d crystals in one call, above the 65535 a launch addresses", n_cry);
    return NNHIP_E_UNSUPPORTED;
  }
  int cap_big = 0, cap_wave = 0;
  for (int b = 0; b < n_cry; ++b) {
    const int m = 3 * (cry_ptr_host[b + 1] - cry_ptr_host[b]);
    if (m < 0) {
      nnhip_set_error("nnhip_phonon_bands: cry_ptr_host decreases at crystal %d", b);
      return NNHIP_E_INVALID;
    }
    if (m > PH_MAX_DIM) {
      nnhip_set_error("nnhip_phonon_bands: crystal %d has dimension 3 x %d = %d, above the supported %d (one workgroup holds the "
                      "dynamical matrix and its eigenvectors in LDS)", b, m / 3, m, PH_MAX_DIM);
      return NNHIP_E_UNSUPPORTED;
    }
    const int mp = (m + 1) & ~1;
    if (mp <= PH_WAVE_DIM) cap_wave = mp > cap_wave ? mp : cap_wave;
    else cap_big = mp > cap_big ? mp : cap_big;
  }
  if ((cap_big == 0 && cap_wave == 0) || n_q == 0) return NNHIP_OK;
  const bool want_v = modes != nullptr;
  PhArgs g;
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
  g.cap_big = cap_big;
  g.cap_wave = cap_wave;
  g.slot_wave = cap_wave ? (unsigned)ph_slot_bytes(cap_wave, want_v) : 0;
  const int per_wg = PH_THREADS / 64;
  const size_t lds_big = cap_big ? ph_slot_bytes(cap_big, want_v) : 0, lds_wave = (size_t)per_wg * g.slot_wave;
  const size_t lds = lds_big > lds_wave ? lds_big : lds_wave;
  const int gx_big = cap_big ? n_q : 0, gx_wave = cap_wave ? cdiv(n_q, per_wg) : 0;
  if (lds > 64 * 1024)   // above the default limit a kernel has to ask for its dynamic LDS
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(phonon_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)ph_slot_bytes(PH_MAX_DIM, true)));
  phonon_kernel<<<dim3(gx_big > gx_wave ? gx_big : gx_wave, n_cry), PH_THREADS, lds, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

extern "C" int nnhip_phonon_dos(const float* values, const int64_t* val_ptr, int32_t n_cry, float lo, float hi, int32_t n_bins,
                                float width, int32_t* counts, float* density, void* stream) {
  if (n_cry < 0 || n_bins < 1 || !(hi > lo) || !(hi - lo <= 3.4e38f) || (n_cry > 0 && (!values || !val_ptr)) ||
      (!counts && !density) || (density && !(width > 0.f && width <= 3.4e38f))) {
    nnhip_set_error("nnhip_phonon_dos: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_cry > 65535) {
    nnhip_set_error("nnhip_phonon_dos: %d crystals in one call, above the 65535 a launch addresses", n_cry);
    return NNHIP_E_UNSUPPORTED;
  }
  if (n_cry == 0) return NNHIP_OK;
  phonon_dos_kernel<<<dim3(cdiv(n_bins, 256), n_cry), 256, 0, (hipStream_t)stream>>>(values, val_ptr, lo, hi, n_bins, width, counts,
                                                                                   density);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
