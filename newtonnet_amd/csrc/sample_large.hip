// Normal-mode sampling above the LDS bound (gfx950, fp32): the mathematics of sample.hip for molecules whose mode matrix does not
// fit in LDS (M = 3 n_b up to 1536: 9.4 MB of fp32), streamed from HBM instead.  Two ordinary launches on the caller's stream, no
// float atomics, no workspace:
//
//   amplitude kernel     one workgroup per (molecule, tile of SMP_TILE samples).  Per chunk of SMPL_KA modes: sigma_k by the rule
//                        of sample_common.h, q[s][k] = sigma_k xi[s][k] (+0 for a mode that is not live) to `amplitudes` and to an
//                        LDS chunk, and thread s adds 1/2 lambda_k q_k^2 of its sample in fp64, k ascending: the order (and the
//                        expression) of sample.hip.  The molecule's first tile writes n_skipped[b].
//   displacement kernel  one workgroup per (molecule, tile of SMP_TILE samples, tile of SMP_THREADS columns j).  Thread t owns
//                        column j0 + t and keeps one fp32 accumulator per sample of the tile in registers; it walks k = 0 .. M - 1
//                        with acc[s] = fmaf(q[s][k], L[k][j], acc[s]): L[k M + j] from global memory (lanes walk j, so a row is
//                        read as consecutive words, once per workgroup), q[s][k] from an LDS chunk of the tile's amplitudes laid
//                        out [k][SMP_TILE] (the 32 amplitudes of a mode are one broadcast read of 128 bytes).  Then
//                        pos_out = pos + acc / sqrt(m_{j / 3}).
// Every output element is the work of one thread that sums over k in the order of sample.hip's kernel with the same operations, so
// a molecule both kernels can serve gets the same bits from either, repeats are bitwise identical, and a sample depends neither on
// the number of samples nor on its tile nor on the rest of the batch.
//
// Which molecules a launch serves is decided on the device from mol_ptr: 3 n_b >= min_dim (and n_b > 0).  Nothing of any other
// molecule is touched, so nnhip_mode_sample on the small molecules and this call on the others fill one set of arrays.
//
// Traffic per molecule: L is read once per sample tile and column tile row by row, ceil(S / 32) x 4 M^2 bytes in all, for 2 S M^2
// flops; the amplitudes of a tile are read once per column tile (ceil(M / 256) x 4 x 32 M bytes, 1 / M of the former).
#include "sample_common.h"

#define SMPL_KA 256   // modes per chunk of the amplitude kernel: one mode per thread in the sigma step
#define SMPL_KC 128   // modes per LDS chunk of the displacement kernel: [128][32] fp32 = 16 KiB, so several workgroups share a CU

namespace {

struct SampleLargeArgs {
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
  float kT, hbar_unit;
  int quantum, n_samples;
  int min_dim;   // molecules with 3 n_b < min_dim are not this launch's
  int m_max;     // largest selected 3 n_b by the host's offsets: the column tiles of the grid cover it
};

// 3 n_b of molecule b if the launch serves it, else 0 (uniform over the workgroup)
__device__ __forceinline__ int smpl_dim(const SampleLargeArgs& g, int b, int* a0) {
  *a0 = g.mol_ptr[b];
  const int nb = g.mol_ptr[b + 1] - *a0;
  if (nb <= 0 || 3 * (long)nb < g.min_dim) return 0;
  return 3 * (long)nb > g.m_max ? -1 : 3 * nb;   // -1: mol_ptr gives the molecule more than mol_ptr_host did (or than the bound)
}

__global__ void __launch_bounds__(SMP_THREADS)
sample_large_amp_kernel(SampleLargeArgs g) {
  __shared__ float sig[SMPL_KA];                    // standard deviation of the mode's amplitude; 0 = not live
  __shared__ float lam[SMPL_KA];                    // eigenvalue of a live mode, else 0
  __shared__ float qs[SMP_TILE][SMPL_KA + 1];       // (+ 1: thread s walks row s, the 32 rows on 32 banks)
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  int a0;
  const int M = smpl_dim(g, b, &a0);
  if (M == 0) return;
  if (M < 0) {
    if (t == 0 && blockIdx.y == 0) g.n_skipped[b] = -1;
    return;
  }
  const int S = g.n_samples;
  const int s0 = blockIdx.y * SMP_TILE;
  const int ns = min(SMP_TILE, S - s0);
  const float thr = g.thr[b];
  const size_t base = 3 * (size_t)S * a0 + (size_t)s0 * M;   // of this tile in xi / amplitudes
  int n_imag = 0;
  double en = 0.0;
  for (int k0 = 0; k0 < M; k0 += SMPL_KA) {                  // (uniform)
    const int kc = min(SMPL_KA, M - k0);
    int imag = 0;
    if (t < kc) imag = smp_mode_rule(g.evals[3 * (size_t)a0 + k0 + t], thr, g.kT, g.hbar_unit, g.quantum, &sig[t], &lam[t]);
    n_imag += __syncthreads_count(imag);
    for (int e = t; e < ns * kc; e += SMP_THREADS) {
      const int s = e / kc, kk = e - s * kc;
      const size_t at = base + (size_t)s * M + k0 + kk;
      const float sg = sig[kk];
      const float q = sg > 0.f ? sg * g.xi[at] : 0.f;
      qs[s][kk] = q;
      g.amplitudes[at] = q;
    }
    __syncthreads();
    if (t < ns) {
      const float* q = qs[t];
      for (int k = 0; k < kc; ++k) en += 0.5 * (double)lam[k] * (double)q[k] * (double)q[k];
    }
    __syncthreads();   // sig / lam / qs are rewritten by the next chunk
  }
  if (t < ns) g.energy[(size_t)b * S + s0 + t] = (float)en;
  if (t == 0 && blockIdx.y == 0) g.n_skipped[b] = n_imag;
}

__global__ void __launch_bounds__(SMP_THREADS)
sample_large_disp_kernel(SampleLargeArgs g) {
  __shared__ __align__(16) float qc[SMPL_KC * SMP_TILE];     // [k][s]
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  int a0;
  const int M = smpl_dim(g, b, &a0);
  const int j0 = blockIdx.z * SMP_THREADS;
  if (M <= 0 || j0 >= M) return;                             // (uniform; the amplitude kernel flags M < 0)
  const int S = g.n_samples;
  const int s0 = blockIdx.y * SMP_TILE;
  const int ns = min(SMP_TILE, S - s0);
  const size_t base = 3 * (size_t)S * a0 + (size_t)s0 * M;   // of this tile in amplitudes / pos_out
  const float* L = g.modes + g.blk_ptr[b];
  const float* amp = g.amplitudes + base;
  const int j = j0 + t;
  const bool mine = j < M;
  float acc[SMP_TILE];
#pragma unroll
  for (int s = 0; s < SMP_TILE; ++s) acc[s] = 0.f;
  for (int k0 = 0; k0 < M; k0 += SMPL_KC) {                  // (uniform)
    const int kc = min(SMPL_KC, M - k0);
    // stage q[s][k0 .. k0 + kc) as [k][s]: e = (k / 4, s, k % 4), so a lane group of 32 reads 16-byte pieces of 8 samples' rows
    // and writes 8 banks 4 deep (twice the cycles of a conflict-free ds_write_b32: a sixteenth of the chunk's LDS reads)
    for (int e = t; e < SMP_TILE * ((kc + 3) & ~3); e += SMP_THREADS) {
      const int kk = ((e >> 7) << 2) | (e & 3), s = (e >> 2) & (SMP_TILE - 1);
      if (kk < kc) qc[kk * SMP_TILE + s] = s < ns ? amp[(size_t)s * M + k0 + kk] : 0.f;
    }
    __syncthreads();
    if (mine) {
      const float* Lk = L + (size_t)k0 * M + j;
#pragma unroll 4
      for (int kk = 0; kk < kc; ++kk) {
        const float l = Lk[(size_t)kk * M];
        const float4* q4 = reinterpret_cast<const float4*>(qc + kk * SMP_TILE);
#pragma unroll
        for (int u = 0; u < SMP_TILE / 4; ++u) {
          const float4 q = q4[u];
          acc[4 * u + 0] = fmaf(q.x, l, acc[4 * u + 0]);
          acc[4 * u + 1] = fmaf(q.y, l, acc[4 * u + 1]);
          acc[4 * u + 2] = fmaf(q.z, l, acc[4 * u + 2]);
          acc[4 * u + 3] = fmaf(q.w, l, acc[4 * u + 3]);
        }
      }
    }
    __syncthreads();   // qc is rewritten by the next chunk
  }
  if (!mine) return;
  const float m = g.masses ? g.masses[a0 + j / 3] : 1.f;
  const float rsm = m > 0.f && m <= 3.4e38f ? 1.f / sqrtf(m) : 0.f;   // as sample.hip
  const float p = g.pos[3 * (size_t)a0 + j];
#pragma unroll
  for (int s = 0; s < SMP_TILE; ++s)
    if (s < ns) g.pos_out[base + (size_t)s * M + j] = p + acc[s] * rsm;
}

}  // namespace

extern "C" int nnhip_mode_sample_large_max_dim(void) { return nnhip_eig_large_max_dim(); }

extern "C" int nnhip_mode_sample_large(const float* modes, const float* evals, const int64_t* blk_ptr, const int32_t* mol_ptr,
                                       const int32_t* mol_ptr_host, int32_t n_mol, const float* masses, const float* pos,
                                       const float* thr, double temperature, int32_t quantum, int32_t n_samples, const float* xi,
                                       float* pos_out, float* energy, float* amplitudes, int32_t* n_skipped, int32_t min_dim,
                                       void* stream) {
  if (n_mol < 0 || n_samples < 0 || !(temperature >= 0.0) || !std::isfinite(temperature) ||
      (n_mol > 0 && (!mol_ptr || !mol_ptr_host || !n_skipped))) {
    nnhip_set_error("nnhip_mode_sample_large: bad arguments");
    return NNHIP_E_INVALID;
  }
  const int bound = nnhip_mode_sample_large_max_dim();
  int m_max = 0;
  for (int b = 0; b < n_mol; ++b) {
    const long m = 3 * ((long)mol_ptr_host[b + 1] - mol_ptr_host[b]);
    if (m < 0) {
      nnhip_set_error("nnhip_mode_sample_large: mol_ptr_host decreases at molecule %d", b);
      return NNHIP_E_INVALID;
    }
    if (m == 0 || m < min_dim) continue;   // not this call's
    if (m > bound) {
      nnhip_set_error("nnhip_mode_sample_large: molecule %d has dimension 3 x %ld = %ld, above the supported %d "
                      "(nnhip_mode_sample_large_max_dim)", b, m / 3, m, bound);
      return NNHIP_E_UNSUPPORTED;
    }
    m_max = m > m_max ? (int)m : m_max;
  }
  if (m_max == 0 || n_samples == 0) return NNHIP_OK;
  if (!modes || !evals || !blk_ptr || !pos || !thr || !xi || !pos_out || !energy || !amplitudes) {
    nnhip_set_error(amplitudes ? "nnhip_mode_sample_large: bad arguments"
                               : "nnhip_mode_sample_large: amplitudes is required (the displacement kernel reads it)");
    return NNHIP_E_INVALID;
  }
  const int n_tiles = (n_samples + SMP_TILE - 1) / SMP_TILE;
  if (n_tiles > SMP_MAX_TILES) {
    nnhip_set_error("nnhip_mode_sample_large: %d samples per molecule, above the supported %d", n_samples, SMP_MAX_TILES * SMP_TILE);
    return NNHIP_E_UNSUPPORTED;
  }
  SampleLargeArgs g;
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
  g.min_dim = min_dim;
  g.m_max = m_max;
  sample_large_amp_kernel<<<dim3(n_mol, n_tiles), SMP_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  sample_large_disp_kernel<<<dim3(n_mol, n_tiles, cdiv(m_max, SMP_THREADS)), SMP_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
