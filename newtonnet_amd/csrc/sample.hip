// Normal-mode sampling (gfx950, fp32): displaced geometries of every molecule of a batch drawn from its harmonic distribution.
//
// nnhip_eig_blocks (csrc/eig.hip) leaves the spectrum of every molecule packed on the device: eigenvalues lambda_k in
// eV / (A^2 amu) at 3 mol_ptr[b] and the modes, ROW k = mode k in mass-weighted coordinates, at blk_ptr[b].  One workgroup serves
// one (molecule, tile of SMP_TILE samples):
//   1. the mode matrix L [M][M], M = 3 n_b, is staged in LDS once (126 x 126 fp32 = 63 504 bytes at the bound), with
//      1 / sqrt(m_i) per atom and, per mode, its standard deviation sigma_k:
//        live iff lambda_k > thr[b]                    (projected, zero and imaginary modes: sigma_k = 0, by rule)
//        classical  sigma^2 = kT / lambda
//        quantum    sigma^2 = (eps / 2 lambda) coth(eps / 2 kT),  eps = hbar omega = hbar_unit sqrt(lambda),
//                   coth(x / 2) = 1 + 2 / expm1(x), x = eps / kT: no overflow (expm1 -> inf gives coth = 1, the ground state, as
//                   does T = 0) and x -> 0 gives eps / 2 lambda + kT / lambda, the classical value, to fp32
//      n_skipped[b] = modes with lambda_k < -thr[b] (written by the molecule's first tile)
//   2. q[s][k] = sigma_k xi[s][k] for the samples of the tile, into LDS (and to `amplitudes` when asked); a mode that is not live
//      gets q = +0 whatever its xi holds
//   3. thread (s, j):  dx_j = (sum_k q[s][k] L[k][j]) / sqrt(m_{j / 3}),  k = 0 .. M - 1 in that order in fp32 FMAs; lanes walk j, so
//      the reads of row k of L are consecutive words (no bank conflicts at any row stride) and q[s][k] is a broadcast;
//      pos_out = pos + dx.  Thread s < tile also sums the harmonic energy 1/2 sum_k lambda_k q_k^2 over the same k order in fp64.
// Every output element is the work of one thread with a fixed summation order and no atomics: repeats are bitwise identical, and
// a sample's result depends neither on the number of samples nor on the tile it falls into.
//
// Layout of the sample batch: the samples of molecule b are the molecules b S .. b S + S - 1, so xi, amplitudes and pos_out hold
// S x [3 n_b] values per molecule at 3 S mol_ptr[b], sample-major.
// The tile sizes, the constants and the per-mode rule of step 1 live in sample_common.h, shared with sample_large.hip.
#include "sample_common.h"   // SMP_TILE = 32 samples per workgroup: q of the tile takes 32 x 126 x 4 = 16 128 bytes at the bound

namespace {

struct SampleArgs {
  const float* modes;
  const float* evals;
  const int64_t* blk_ptr;
  const int* mol_ptr;
  const float* masses;
  const float* pos;
  const float* thr;
  const float* xi;
  float* pos_out;
  float* energy;
  float* amplitudes;
  int* n_skipped;
  float kT, hbar_unit;   // eV;  eps = hbar_unit sqrt(lambda) in eV
  int quantum, n_samples, m_max;
};

__host__ __device__ inline int smp_atoms_max(int m_max) { return (m_max + 2) / 3; }

__global__ void __launch_bounds__(SMP_THREADS)
sample_kernel(SampleArgs g) {
  extern __shared__ __align__(16) float smem_f[];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const int a0 = g.mol_ptr[b];
  const int nb = g.mol_ptr[b + 1] - a0;
  if (nb <= 0) return;   // (uniform over the workgroup)
  const int M = 3 * nb;
  if (M > g.m_max) {     // mol_ptr and mol_ptr_host disagree: the LDS of this launch is too small for the molecule (uniform)
    if (t == 0 && blockIdx.y == 0) g.n_skipped[b] = -1;
    return;
  }
  const int S = g.n_samples;
  const int s0 = blockIdx.y * SMP_TILE;
  const int ns = min(SMP_TILE, S - s0);
  // LDS carve-up, sized by the host for the largest molecule of the batch (g.m_max)
  const int mx = g.m_max;
  float* Ls = smem_f;                      // [M][M]
  float* sig = Ls + mx * mx;               // [mx]  standard deviation of the mode's amplitude; 0 = not live
  float* lam = sig + mx;                   // [mx]  eigenvalue of a live mode, else 0
  float* rsm = lam + mx;                   // [atoms] 1 / sqrt(m_i)
  float* qs = rsm + smp_atoms_max(mx);     // [SMP_TILE][M]

  const float* L = g.modes + g.blk_ptr[b];
  for (int e = t; e < M * M; e += SMP_THREADS) Ls[e] = L[e];
  for (int i = t; i < nb; i += SMP_THREADS) {
    const float m = g.masses ? g.masses[a0 + i] : 1.f;
    rsm[i] = m > 0.f && m <= 3.4e38f ? 1.f / sqrtf(m) : 0.f;   // (nnhip_eig_blocks does not compute such a molecule: its spectrum is zero)
  }
  int imag = 0;
  if (t < M) {           // M <= 126 < SMP_THREADS: one mode per thread
    imag = smp_mode_rule(g.evals[3 * (size_t)a0 + t], g.thr[b], g.kT, g.hbar_unit, g.quantum, &sig[t], &lam[t]);
  }
  const int n_imag = __syncthreads_count(imag);   // (also the barrier behind the staging)
  if (t == 0 && blockIdx.y == 0) g.n_skipped[b] = n_imag;

  const size_t base = 3 * (size_t)S * a0 + (size_t)s0 * M;   // of this tile in xi / amplitudes / pos_out
  for (int e = t; e < ns * M; e += SMP_THREADS) {
    const int k = e % M;
    const float sg = sig[k];
    const float q = sg > 0.f ? sg * g.xi[base + e] : 0.f;
    qs[e] = q;
    if (g.amplitudes) g.amplitudes[base + e] = q;
  }
  __syncthreads();
  for (int e = t; e < ns * M; e += SMP_THREADS) {
    const int s = e / M, j = e - s * M;
    const float* q = qs + s * M;
    float acc = 0.f;
    for (int k = 0; k < M; ++k) acc = fmaf(q[k], Ls[k * M + j], acc);
    g.pos_out[base + e] = g.pos[3 * (size_t)a0 + j] + acc * rsm[j / 3];
  }
  if (t < ns) {
    const float* q = qs + t * M;
    double en = 0.0;
    for (int k = 0; k < M; ++k) en += 0.5 * (double)lam[k] * (double)q[k] * (double)q[k];
    g.energy[(size_t)b * S + s0 + t] = (float)en;
  }
}

size_t smp_lds_bytes(int m_max) {
  return 4 * ((size_t)m_max * m_max + 2 * (size_t)m_max + smp_atoms_max(m_max) + (size_t)SMP_TILE * m_max);
}

}  // namespace

extern "C" int nnhip_mode_sample(const float* modes, const float* evals, const int64_t* blk_ptr, const int32_t* mol_ptr,
                                 const int32_t* mol_ptr_host, int32_t n_mol, const float* masses, const float* pos, const float* thr,
                                 double temperature, int32_t quantum, int32_t n_samples, const float* xi, float* pos_out,
                                 float* energy, float* amplitudes, int32_t* n_skipped, void* stream) {
  if (n_mol < 0 || n_samples < 0 || !(temperature >= 0.0) || !std::isfinite(temperature) ||
      (n_mol > 0 && (!mol_ptr || !mol_ptr_host || !n_skipped))) {
    nnhip_set_error("nnhip_mode_sample: bad arguments");
    return NNHIP_E_INVALID;
  }
  const int bound = nnhip_eig_max_dim();
  int m_max = 0;
  for (int b = 0; b < n_mol; ++b) {
    const int m = 3 * (mol_ptr_host[b + 1] - mol_ptr_host[b]);
    if (m < 0) {
      nnhip_set_error("nnhip_mode_sample: mol_ptr_host decreases at molecule %d", b);
      return NNHIP_E_INVALID;
    }
    if (m > bound) {
      nnhip_set_error("nnhip_mode_sample: molecule %d has dimension 3 x %d = %d, above the supported %d (one workgroup holds the "
                      "mode matrix in LDS)", b, m / 3, m, bound);
      return NNHIP_E_UNSUPPORTED;
    }
    m_max = m > m_max ? m : m_max;
  }
  if (m_max == 0 || n_samples == 0) return NNHIP_OK;
  if (!modes || !evals || !blk_ptr || !pos || !thr || !xi || !pos_out || !energy) {
    nnhip_set_error("nnhip_mode_sample: bad arguments");
    return NNHIP_E_INVALID;
  }
  const int n_tiles = (n_samples + SMP_TILE - 1) / SMP_TILE;
  if (n_tiles > SMP_MAX_TILES) {
    nnhip_set_error("nnhip_mode_sample: %d samples per molecule, above the supported %d", n_samples, SMP_MAX_TILES * SMP_TILE);
    return NNHIP_E_UNSUPPORTED;
  }
  SampleArgs g;
  g.modes = modes;
  g.evals = evals;
  g.blk_ptr = blk_ptr;
  g.mol_ptr = mol_ptr;
  g.masses = masses;
  g.pos = pos;
  g.thr = thr;
  g.xi = xi;
  g.pos_out = pos_out;
  g.energy = energy;
  g.amplitudes = amplitudes;
  g.n_skipped = n_skipped;
  g.kT = smp_kT(temperature);
  g.hbar_unit = smp_hbar_unit();
  g.quantum = quantum ? 1 : 0;
  g.n_samples = n_samples;
  g.m_max = m_max;
  const size_t lds = smp_lds_bytes(m_max);
  if (lds > 64 * 1024)   // above the default limit a kernel has to ask for its dynamic LDS
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(sample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)smp_lds_bytes(bound)));
  sample_kernel<<<dim3(n_mol, n_tiles), SMP_THREADS, lds, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
