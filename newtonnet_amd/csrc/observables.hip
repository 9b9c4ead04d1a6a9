// Observables of molecular-dynamics trajectories on the device (gfx950): the pair-distance histogram behind the radial distribution
// function, and lagged time correlations (mean squared displacement, velocity autocorrelation).  The arithmetic of both entry points
// is written out in include/newtonnet_hip.h; tests/observables_ref.py restates it.
//
// Both results are independent of scheduling and of the grid: the histogram counts integers (LDS uint32 counters flushed with 64-bit
// integer atomics), the correlation has one writer per element and adds in fp64 in an order fixed by the constants below.
#include "common.h"
#include "pair_disp.h"

// ---------------------------------------------------------------------------------------------
// pair-distance histogram
// ---------------------------------------------------------------------------------------------
#define RDF_THREADS 256
#define RDF_WAVES (RDF_THREADS / WAVE)
#define RDF_TILE 64                    // atoms of an i tile and of a j tile: one j per lane
#define RDF_MAX_KINDS NNHIP_RDF_MAX_KINDS
#define RDF_MAX_BINS NNHIP_RDF_MAX_BINS
#define RDF_MAX_COUNTERS NNHIP_RDF_MAX_COUNTERS   // S (S + 1) / 2 * n_bins: 64 KiB of LDS counters
// A workgroup counts at most (frames of a flush) x RDF_TILE x (atoms of the system) pairs between two flushes: the frames of a flush
// are cut so that this stays below 2^32, which needs a system of at most 2^26 atoms.
#define RDF_MAX_ATOMS (1 << 26)
#define RDF_TARGET_BLOCKS 2048         // frames are cut into chunks until the grid has about this many workgroups

// One workgroup = (system b, i tiles blockIdx.x, blockIdx.x + gridDim.x, ..., a chunk of frames).  A wave takes one (frame, j tile)
// at a time: every lane keeps its j in registers (a j is read once per i tile, and nothing is reread from LDS), the i of the tile
// come through uniform loads, and the four waves work on different frames.  LDS holds the bin table and the counters of the workgroup.
__global__ void __launch_bounds__(RDF_THREADS)
rdf_kernel(const float* __restrict__ pos, long pos_stride, int n_frames, const float* __restrict__ cell, long cell_stride,
           const int* __restrict__ mol_ptr, const int* __restrict__ kind, int S, const float* __restrict__ edge2, int n_bins,
           int frames_per_chunk, unsigned long long* __restrict__ counts) {
  extern __shared__ __align__(16) char rdf_smem[];
  float* s_edge = reinterpret_cast<float*>(rdf_smem);                 // [n_bins + 1]
  unsigned* s_hist = reinterpret_cast<unsigned*>(s_edge + n_bins + 1);   // [P][n_bins]
  const int b = blockIdx.z;
  const int s = mol_ptr[b], e = mol_ptr[b + 1], n = e - s;
  const int n_tiles = (n + RDF_TILE - 1) / RDF_TILE;
  if ((int)blockIdx.x >= n_tiles) return;       // (uniform: the whole workgroup leaves before any barrier)
  const int n_counters = (S * (S + 1) / 2) * n_bins;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int k = tid; k <= n_bins; k += RDF_THREADS) s_edge[k] = edge2[k];
  for (int k = tid; k < n_counters; k += RDF_THREADS) s_hist[k] = 0u;
  __syncthreads();
  const float r2_max = s_edge[n_bins];
  const float inv_dr = (float)n_bins / sqrtf(r2_max);     // for the first guess of a bin only: the table decides
  const int f_begin = blockIdx.y * frames_per_chunk;
  const int f_end = min(n_frames, f_begin + frames_per_chunk);
  // frames between two flushes of one i tile: frames x RDF_TILE x n < 2^32 (n <= 2^26 is checked by the host)
  const int f_flush = max(1, (int)min((long)frames_per_chunk, 0xFFFFFFFFl / ((long)RDF_TILE * max(n, 1))));
  unsigned long long* out = counts + (size_t)b * n_counters;
  // (max_atoms, which sizes the grid, is at least the largest system: one workgroup per i tile; the stride only keeps a call with a
  // smaller one in bounds and right)
  for (int it = blockIdx.x; it < n_tiles; it += gridDim.x) {
    const int i0 = s + it * RDF_TILE, i1 = min(e, i0 + RDF_TILE);
    const int njt = n_tiles - it;                 // j tiles it .. n_tiles - 1 hold every j > i
    for (int f0 = f_begin; f0 < f_end; f0 += f_flush) {
      const int nf = min(f_flush, f_end - f0);
      for (int u = w; u < nf * njt; u += RDF_WAVES) {
        const int f = f0 + u / njt, jt = it + u % njt;
        const float* __restrict__ p = pos + (long)f * pos_stride;
        const CellInfo ci = load_cell(cell + (long)f * cell_stride, b);
        const int j = s + jt * RDF_TILE + lane;
        const bool have_j = j < e;
        const int kj = have_j ? kind[j] : -1;
        const float xj = have_j ? p[3 * (long)j] : 0.f, yj = have_j ? p[3 * (long)j + 1] : 0.f, zj = have_j ? p[3 * (long)j + 2] : 0.f;
        const bool use_j = kj >= 0 && kj < S;
        for (int i = i0; i < i1; ++i) {
          const int ki = kind[i];
          if (ki < 0 || ki >= S) continue;        // (uniform)
          const float xi = p[3 * (long)i], yi = p[3 * (long)i + 1], zi = p[3 * (long)i + 2];
          if (!(use_j && j > i)) continue;
          float dx, dy, dz;
          const float r2 = pair_disp(xi, yi, zi, xj, yj, zj, ci, dx, dy, dz);
          if (!(r2 < r2_max)) continue;           // (also a NaN)
          // bin k: edge2[k] <= r2 < edge2[k+1].  The square root only proposes k; the two loops move it to where the table puts r2.
          int k = min(n_bins - 1, max(0, (int)(sqrtf(r2) * inv_dr)));
          while (k > 0 && r2 < s_edge[k]) --k;
          while (k < n_bins - 1 && r2 >= s_edge[k + 1]) ++k;
          if (r2 < s_edge[k]) continue;           // (below edge2[0]: only with a table that does not start at 0)
          const int a = min(ki, kj), c = max(ki, kj);
          atomicAdd(&s_hist[(a * S - a * (a - 1) / 2 + (c - a)) * n_bins + k], 1u);
        }
      }
      __syncthreads();
      for (int k = tid; k < n_counters; k += RDF_THREADS) {
        const unsigned v = s_hist[k];
        if (v) {
          atomicAdd(&out[k], (unsigned long long)v);
          s_hist[k] = 0u;
        }
      }
      __syncthreads();
    }
  }
}

extern "C" int nnhip_rdf_accumulate(const float* pos, int64_t pos_frame_stride, int32_t n_frames, const float* cell,
                                    int64_t cell_frame_stride, const int32_t* mol_ptr, int32_t n_mol, int32_t n_atoms,
                                    int32_t max_atoms, const int32_t* kind, int32_t n_kinds, const float* edge2, int32_t n_bins,
                                    int64_t* counts, void* stream_) {
  const char* who = "nnhip_rdf_accumulate";
  if (n_kinds < 1 || n_kinds > RDF_MAX_KINDS || n_bins < 1 || n_bins > RDF_MAX_BINS ||
      (long)(n_kinds * (n_kinds + 1) / 2) * n_bins > RDF_MAX_COUNTERS) {
    nnhip_set_error("%s: %d kinds and %d bins are outside the kernel's LDS histogram: at most %d kinds, %d bins and "
                    "n_kinds (n_kinds + 1) / 2 * n_bins <= %d", who, n_kinds, n_bins, RDF_MAX_KINDS, RDF_MAX_BINS, RDF_MAX_COUNTERS);
    return NNHIP_E_INVALID;
  }
  ARG_CHECK(n_frames >= 0 && n_mol >= 0 && n_atoms >= 0 && max_atoms >= 0 && max_atoms <= n_atoms, who);
  ARG_CHECK(mol_ptr && edge2 && counts, who);
  ARG_CHECK(n_atoms == 0 || (pos && kind && cell), who);
  ARG_CHECK(pos_frame_stride >= 3 * (int64_t)n_atoms, who);
  ARG_CHECK(cell_frame_stride == 0 || cell_frame_stride >= 9 * (int64_t)n_mol, who);
  if (n_atoms > RDF_MAX_ATOMS) {
    nnhip_set_error("%s: more than %d atoms", who, RDF_MAX_ATOMS);
    return NNHIP_E_UNSUPPORTED;
  }
  if (n_mol > 65535) {
    nnhip_set_error("%s: more than 65535 systems in one call", who);
    return NNHIP_E_UNSUPPORTED;
  }
  if (n_frames == 0 || n_mol == 0 || max_atoms < 2) return NNHIP_OK;     // no pair anywhere
  const int tiles = cdiv(max_atoms, RDF_TILE);
  int chunks = cdiv(RDF_TARGET_BLOCKS, (long)tiles * n_mol);
  chunks = chunks < 1 ? 1 : (chunks > n_frames ? n_frames : chunks);
  const int per_chunk = cdiv(n_frames, chunks);
  chunks = cdiv(n_frames, per_chunk);
  const size_t lds = ((size_t)n_bins + 1 + (size_t)(n_kinds * (n_kinds + 1) / 2) * n_bins) * 4;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(rdf_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  rdf_kernel<<<dim3(tiles, chunks, n_mol), RDF_THREADS, lds, (hipStream_t)stream_>>>(
      pos, (long)pos_frame_stride, n_frames, cell, (long)cell_frame_stride, mol_ptr, kind, n_kinds, edge2, n_bins, per_chunk,
      reinterpret_cast<unsigned long long*>(counts));
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// lagged time correlation
// ---------------------------------------------------------------------------------------------
#define TC_THREADS 256
#define TC_LAGS 64                     // lags of a workgroup: one per lane
#define TC_PARTS (TC_THREADS / WAVE)   // partial sums of an element: wave p takes the atoms p, p + TC_PARTS, ... of an atom tile
#define TC_ATOMS 16                    // atoms of a staged tile
#define TC_BLOCK 64                    // frames of an origin block
#define TC_PITCH (3 * TC_ATOMS + 1)    // LDS row of one frame; odd, so that the lanes (consecutive frames, one atom) hit 64 banks
#define TC_MAX_KINDS NNHIP_RDF_MAX_KINDS

// One workgroup = (system b, TC_LAGS lags).  Per atom tile and origin block it stages the frames of the origins and the frames they
// are paired with (TC_BLOCK and TC_BLOCK + TC_LAGS - 1 rows) and every thread adds the terms of its lag, in fp64, to the accumulator
// of the atom's kind.  Order of the sum of one element: atom tiles ascending, origin blocks ascending, the atoms of the wave's share
// ascending, origins ascending -- per (atom, block) a subtotal, added to the kind's accumulator -- and at the end
// (part 0 + part 1) + (part 2 + part 3).  None of it depends on the grid.
template <int MODE>
__global__ void __launch_bounds__(TC_THREADS)
time_corr_kernel(const float* __restrict__ x, long stride, int n_frames, const int* __restrict__ mol_ptr,
                 const int* __restrict__ kind, int S, const float* __restrict__ weight, int max_lag, int every,
                 double* __restrict__ sums) {
  __shared__ __align__(16) float s_org[TC_BLOCK * TC_PITCH];
  __shared__ __align__(16) float s_lag[(TC_BLOCK + TC_LAGS - 1) * TC_PITCH];
  static_assert(sizeof(s_lag) >= sizeof(double) * TC_PARTS * TC_MAX_KINDS * TC_LAGS, "the partial sums reuse the staged frames");
  double (*s_red)[TC_MAX_KINDS][TC_LAGS] = reinterpret_cast<double (*)[TC_MAX_KINDS][TC_LAGS]>(s_lag);   // after the last tile
  const int b = blockIdx.y;
  const int s = mol_ptr[b], e = mol_ptr[b + 1];
  const int l0 = blockIdx.x * TC_LAGS;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int part = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lag = l0 + lane;
  double acc[TC_MAX_KINDS];
#pragma unroll
  for (int k = 0; k < TC_MAX_KINDS; ++k) acc[k] = 0.0;
  for (int a0 = s; a0 < e; a0 += TC_ATOMS) {
    const int ta = min(TC_ATOMS, e - a0);
    // origins t0 with t0 + l0 < n_frames can pair with a lag of this workgroup
    for (int o0 = 0; o0 + l0 < n_frames; o0 += TC_BLOCK) {
      const int n_org = min(TC_BLOCK, n_frames - o0);
      const int n_lag = min(TC_BLOCK + TC_LAGS - 1, n_frames - (o0 + l0));
      __syncthreads();                 // the tile before has been read
      for (int k = tid; k < n_org * 3 * ta; k += TC_THREADS) {
        const int fr = k / (3 * ta), c = k - fr * 3 * ta;
        s_org[fr * TC_PITCH + c] = x[(long)(o0 + fr) * stride + 3 * (long)a0 + c];
      }
      for (int k = tid; k < n_lag * 3 * ta; k += TC_THREADS) {
        const int fr = k / (3 * ta), c = k - fr * 3 * ta;
        s_lag[fr * TC_PITCH + c] = x[(long)(o0 + l0 + fr) * stride + 3 * (long)a0 + c];
      }
      __syncthreads();
      const int first = ((o0 + every - 1) / every) * every;       // first origin of the block
      for (int a = part; a < ta; a += TC_PARTS) {
        const int ka = kind[a0 + a];
        if (ka < 0 || ka >= S) continue;                            // (uniform)
        const float wa = weight ? weight[a0 + a] : 1.0f;
        double sub = 0.0;
        for (int t0 = first; t0 < o0 + n_org; t0 += every) {
          if (lag <= max_lag && t0 + lag < n_frames) {
#pragma clang fp contract(off)
            const float* p0 = s_org + (t0 - o0) * TC_PITCH + 3 * a;
            const float* p1 = s_lag + (t0 - o0 + lane) * TC_PITCH + 3 * a;
            float v;
            if (MODE == 0) {
              v = __fmaf_rn(p0[2], p1[2], __fmaf_rn(p0[1], p1[1], p0[0] * p1[0]));
            } else {
              const float dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
              v = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
            }
            if (weight) v = wa * v;
            sub += (double)v;
          }
        }
#pragma unroll
        for (int k = 0; k < TC_MAX_KINDS; ++k)
          if (k == ka) acc[k] += sub;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TC_MAX_KINDS; ++k) s_red[part][k][lane] = acc[k];
  __syncthreads();
  if (part == 0 && lag <= max_lag) {
    for (int k = 0; k < S; ++k) {
      const double total = (s_red[0][k][lane] + s_red[1][k][lane]) + (s_red[2][k][lane] + s_red[3][k][lane]);
      sums[((size_t)b * S + k) * (max_lag + 1) + lag] += total;
    }
  }
}

extern "C" int nnhip_time_correlation(const float* x, int64_t frame_stride, int32_t n_frames, const int32_t* mol_ptr, int32_t n_mol,
                                      int32_t n_atoms, const int32_t* kind, int32_t n_kinds, const float* weight, int32_t mode,
                                      int32_t max_lag, int32_t origin_every, double* sums, void* stream_) {
  const char* who = "nnhip_time_correlation";
  if (mode != 0 && mode != 1) {
    nnhip_set_error("%s: mode %d (0 = product, 1 = squared displacement expected)", who, mode);
    return NNHIP_E_INVALID;
  }
  if (max_lag < 0 || max_lag >= n_frames) {
    nnhip_set_error("%s: max_lag %d needs more than %d frames (max_lag < n_frames)", who, max_lag, n_frames);
    return NNHIP_E_INVALID;
  }
  if (origin_every < 1) {
    nnhip_set_error("%s: origin_every %d (>= 1 expected)", who, origin_every);
    return NNHIP_E_INVALID;
  }
  ARG_CHECK(n_kinds >= 1 && n_kinds <= TC_MAX_KINDS, who);
  ARG_CHECK(n_mol >= 0 && n_atoms >= 0 && mol_ptr && sums, who);
  ARG_CHECK(n_atoms == 0 || (x && kind), who);
  ARG_CHECK(frame_stride >= 3 * (int64_t)n_atoms, who);
  if (n_mol > 65535) {
    nnhip_set_error("%s: more than 65535 systems in one call", who);
    return NNHIP_E_UNSUPPORTED;
  }
  if (n_mol == 0 || n_atoms == 0) return NNHIP_OK;
  const dim3 grid(cdiv(max_lag + 1, TC_LAGS), n_mol);
  if (mode == 0)
    time_corr_kernel<0><<<grid, TC_THREADS, 0, (hipStream_t)stream_>>>(x, (long)frame_stride, n_frames, mol_ptr, kind, n_kinds, weight,
                                                                      max_lag, origin_every, sums);
  else
    time_corr_kernel<1><<<grid, TC_THREADS, 0, (hipStream_t)stream_>>>(x, (long)frame_stride, n_frames, mol_ptr, kind, n_kinds, weight,
                                                                      max_lag, origin_every, sums);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
