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
// The weight, the element and the Jacobi are device functions of csrc/phonon_common.h, which csrc/phonon_large.hip (primitive cells
// above this file's bound) calls too.
// LDS of a problem with modes: 4 planes of Mp (Mp + 1) floats + 48 Mp bytes of vectors + the tile table: 155 952 bytes at
// d = 96 (32 atoms), the largest multiple of 3 that fits the 160 KiB of a CU (d = 99 needs 168 950).
#include "phonon_common.h"   // the weight, the element and the complex Jacobi, shared with csrc/phonon_large.hip

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
  for (int i = t; i < n; i += T) rowo[i] = ph_rsm(g.masses, a0 + i);
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
      wch[x] = ph_weight(ist, g.img_off, ij, q0, q1, q2);
    }
    ph_sync<ONE_WAVE>();
    for (int e = t; e < M * M; e += T) {
      const int a = e / M, c = e - a * M;
      const int i = a / 3, j = c / 3, beta = c - 3 * j;
      float are = Are[a * ld + c], aim = Aim[a * ld + c];
      const float* f = fc + ((size_t)a * N + (size_t)R0 * n + j) * 3 + beta;
      ph_accumulate(f, n, wch + i * n + j, n * n, rc, are, aim);
      Are[a * ld + c] = are;
      Aim[a * ld + c] = aim;
    }
    ph_sync<ONE_WAVE>();
  }
  for (int e = t; e < M * M; e += T) {
    const int a = e / M, c = e - a * M;
    if (a > c) continue;   // the thread of (a, c), a <= c, writes both halves: D is exactly Hermitian from here on
    const float f = (float)(rowo[a / 3] * rowo[c / 3]);
    float re, im;
    ph_hermitian(Are[a * ld + c], Aim[a * ld + c], Are[c * ld + a], Aim[c * ld + a], f, a == c, re, im);
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
  bool converged;
  const int n_sweeps = ph_jacobi<ONE_WAVE>(Are, Aim, Wre, Wim, Mp, ld, rowo, rowd, cst, dlt, tab, want_v, EIG_EPS2, EIG_MAX_SWEEPS, t,
                                           converged);
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
      phs[i] = ph_phase(Wre + i * ld, Wim + i * ld, M);
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
