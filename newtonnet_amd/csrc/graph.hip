// Neighbor list + edge embedding kernels (gfx950).
//
// Replaces RadiusGraph.forward (newtonnet/layers/representations.py:57-100), ScaledNorm (:118-133),
// PolynomialCutoff p=9 (:155-171) and RadialBesselLayer (:223-235) of the reference.
//
// The edge list is produced directly in the reference's order -- (molecule, i, j) ascending -- which
// makes it a CSR over the receiver i; every later aggregation is a deterministic segmented sum
// (no float atomics).  HBM-bound integer/float32 work: one thread per receiver row, molecule-local
// position reads served by L1/L2.
#include <stdlib.h>

#include "common.h"
#include "pair_disp.h"
#include "switches.h"

// ---------------------------------------------------------------------------------------------
// molecule extents from the (sorted) batch vector
// ---------------------------------------------------------------------------------------------
__global__ void mol_ptr_kernel(const int64_t* __restrict__ batch, int n_atoms, int n_mol, int* __restrict__ mol_ptr,
                               int* __restrict__ status, const int64_t* __restrict__ z = nullptr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  if (z) {   // (the species check of check_species_kernel, in the same pass: the deferred step's one launch less)
    const long zi = z[i];
    if (zi < 0 || zi >= NNHIP_N_ELEMENTS) atomicOr(status, 2);
  }
  const long b = batch[i];
  const long bp = (i == 0) ? -1 : batch[i - 1];
  if (b < bp || b < 0 || b >= n_mol) {
    atomicOr(status, 1);
    return;
  }
  for (long k = bp + 1; k <= b; ++k) mol_ptr[k] = i;  // also covers empty molecule ids in between
  if (i == n_atoms - 1)
    for (long k = b + 1; k <= n_mol; ++k) mol_ptr[k] = n_atoms;
}

// One launch instead of three memsets (each memset of an odd length is two fill dispatches): status[0] = 0,
// mol_ptr[0..n_mol] = 0 (so that an invalid batch vector leaves empty, in-bounds molecule extents) and row_ptr = 0.
__global__ void graph_init_kernel(int* __restrict__ status, int* __restrict__ mol_ptr, int n_mol1,
                                  int* __restrict__ row_ptr, int n_atoms1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) status[0] = 0;
  if (i < n_mol1) mol_ptr[i] = 0;
  if (i < n_atoms1) row_ptr[i] = 0;
}

// z outside the embedding / scale / shift tables (the reference raises IndexError, newtonnet.py:142): flag, never index
__global__ void check_species_kernel(const int64_t* __restrict__ z, int n_atoms, int* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  const long zi = z[i];
  if (zi < 0 || zi >= NNHIP_N_ELEMENTS) atomicOr(status, 2);
}
extern "C" int nnhip_check_species(const int64_t* z, int32_t n_atoms, int32_t* status, void* stream_) {
  if (n_atoms < 0 || !status || (n_atoms && !z)) {
    nnhip_set_error("nnhip_check_species: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_atoms == 0) return NNHIP_OK;
  check_species_kernel<<<cdiv(n_atoms, 256), 256, 0, (hipStream_t)stream_>>>(z, n_atoms, status);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// pair predicate shared by the count and fill passes (must be bit-identical in both)
// ---------------------------------------------------------------------------------------------
// CellInfo, load_cell and pair_disp live in pair_disp.h (csrc/observables.hip bins the same r2).  The reference's predicate is
// sqrt_rn(r2) < cutoff; the host turns the cutoff into the equivalent threshold on r2 once (see the header for why):
static float cut2_of(float cutoff) {
  float t = cutoff * cutoff;
  if (!(t < INFINITY)) return INFINITY;
  while (t > 0.f && sqrtf(t) >= cutoff) t = nextafterf(t, 0.f);
  while (sqrtf(t) < cutoff) t = nextafterf(t, INFINITY);
  return t;
}

// One wavefront per receiver atom i; the lanes test 64 candidate senders j at a time and a ballot + prefix popcount
// keeps the edges in ascending j (the reference's order) without any serial loop over the molecule.
template <bool FILL>
__global__ void __launch_bounds__(256)
graph_rows_kernel(const float* __restrict__ pos, const float* __restrict__ cell, const int64_t* __restrict__ batch,
                  const int* __restrict__ mol_ptr, int n_atoms, int n_mol, float cut2, int* __restrict__ deg,
                  const int* __restrict__ row_ptr, int* __restrict__ col, int* __restrict__ erow,
                  float* __restrict__ disp, int64_t* __restrict__ edge_index, int n_edges, int* __restrict__ upper = nullptr,
                  const int* __restrict__ n_edges_dev = nullptr, int* __restrict__ status = nullptr) {
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= n_atoms) return;
  if (FILL && n_edges_dev) {   // early launch (nnhip_graph_finish_early): n_edges is the CAPACITY of the arrays, the count is on the device
    const int cap = n_edges;
    n_edges = *n_edges_dev;
    if (n_edges > cap) return;   // the arrays are too small: nothing is written, the host repeats the launch with the real count
  }
  const int lane = threadIdx.x & 63;
  const long b = batch[i];
  if (b < 0 || b >= n_mol) {   // flagged by mol_ptr_kernel; keep every access in bounds
    if (!FILL && lane == 0) {
      deg[i] = 0;
      if (upper) upper[i] = 0;
    }
    return;
  }
  const int s = mol_ptr[b], e = mol_ptr[b + 1];
  // status bit 8: a molecule too large for the molecule-resident kernels (edge.hip:force_fwd_mol_kernel stages a molecule's node
  // rows in LDS); one atomic per such molecule, none in a batch of small ones
  if (!FILL && status && lane == 0 && i == s && e - s > NNHIP_MOL_STAGE_MAX) atomicOr(status, 8);
  const CellInfo ci = load_cell(cell, b);
  const float xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
  int cnt = 0, cnt_up = 0;   // cnt_up: neighbors above i = the undirected pairs this row owns (section "Undirected pairs")
  int w = FILL ? row_ptr[i] : 0;
  for (int j0 = s; j0 < e; j0 += 64) {
    const int j = j0 + lane;
    bool hit = false;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (j < e && j != i) {
      const float r2 = pair_disp(xi, yi, zi, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ci, dx, dy, dz);
      hit = r2 < cut2;
    }
    const unsigned long long mask = __ballot(hit);
    if (FILL) {
      if (hit) {
        const int o = w + __popcll(mask & ((1ull << lane) - 1ull));
        col[o] = j;
        erow[o] = i;
        disp[3 * (long)o] = dx;
        disp[3 * (long)o + 1] = dy;
        disp[3 * (long)o + 2] = dz;
        if (edge_index) {
          edge_index[o] = i;
          edge_index[(long)n_edges + o] = j;
        }
      }
      w += __popcll(mask);
    } else {
      cnt += __popcll(mask);
      if (upper) cnt_up += __popcll(__ballot(hit && j > i));
    }
  }
  if (!FILL && lane == 0) {
    deg[i] = cnt;
    if (upper) upper[i] = cnt_up;
  }
}

// exclusive scan of deg[n] -> row_ptr[n+1] in two fully parallel launches (in place is fine: deg may alias row_ptr):
//   scan_partials_kernel: one 1024-element tile per block -> tile sum
//   scan_apply_kernel:    every block sums the tile sums before it (<= 1024 tiles, one coalesced pass), scans its own
//                         tile in LDS and writes the exclusive prefix; the last block also writes row_ptr[n]
#define SCAN_TILE 1024
__device__ __forceinline__ int block_reduce_sum_1024(int v, int* sh) {
  const int t = threadIdx.x;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  if ((t & 63) == 0) sh[t >> 6] = v;
  __syncthreads();
  int s = 0;
  if (t < 16) s = sh[t];
  if (t < 64) {
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
    if (t == 0) sh[16] = s;
  }
  __syncthreads();
  const int total = sh[16];
  __syncthreads();
  return total;
}
__global__ void __launch_bounds__(SCAN_TILE) scan_partials_kernel(const int* deg, int n, int* tile_sums, const int* deg2 = nullptr,
                                                                  int* tile_sums2 = nullptr) {
  __shared__ int sh[17];
  if (blockIdx.y) {   // (second array of a dual scan)
    deg = deg2;
    tile_sums = tile_sums2;
  }
  const int k = blockIdx.x * SCAN_TILE + threadIdx.x;
  const int total = block_reduce_sum_1024(k < n ? deg[k] : 0, sh);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}
__global__ void __launch_bounds__(SCAN_TILE) scan_apply_kernel(const int* deg, int n, const int* tile_sums, int* row_ptr,
                                                               const int* deg2 = nullptr, const int* tile_sums2 = nullptr,
                                                               int* row_ptr2 = nullptr) {
  __shared__ int sh[17];
  __shared__ int part[SCAN_TILE];
  if (blockIdx.y) {
    deg = deg2;
    tile_sums = tile_sums2;
    row_ptr = row_ptr2;
  }
  const int t = threadIdx.x;
  int before = 0;
  for (int b = t; b < (int)blockIdx.x; b += SCAN_TILE) before += tile_sums[b];
  const int offset = block_reduce_sum_1024(before, sh);
  const int k = blockIdx.x * SCAN_TILE + t;
  const int d = k < n ? deg[k] : 0;
  part[t] = d;
  __syncthreads();
  for (int off = 1; off < SCAN_TILE; off <<= 1) {
    const int v = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  if (k < n) row_ptr[k] = offset + part[t] - d;
  if (k == n - 1) row_ptr[n] = offset + part[t];
}
// tile_sums: scratch of ceil(n / 1024) ints.  Callers pass the tail of a buffer they own (see below).
static int launch_scan(const int* deg, int n, int* row_ptr, int* tile_sums, hipStream_t stream) {
  const int nb = cdiv(n, SCAN_TILE);
  if (nb > SCAN_TILE * SCAN_TILE) {
    nnhip_set_error("scan: n = %d too large", n);
    return NNHIP_E_UNSUPPORTED;
  }
  scan_partials_kernel<<<nb, SCAN_TILE, 0, stream>>>(deg, n, tile_sums);
  LAUNCH_CHECK();
  scan_apply_kernel<<<nb, SCAN_TILE, 0, stream>>>(deg, n, tile_sums, row_ptr);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// two independent scans of the same length in the same two launches (row_ptr and pair_ptr of the deferred step)
static int launch_scan2(const int* deg, int* row_ptr, int* tile_sums, const int* deg2, int* row_ptr2, int* tile_sums2, int n,
                        hipStream_t stream) {
  const int nb = cdiv(n, SCAN_TILE);
  if (nb > SCAN_TILE * SCAN_TILE) {
    nnhip_set_error("scan: n = %d too large", n);
    return NNHIP_E_UNSUPPORTED;
  }
  scan_partials_kernel<<<dim3(nb, 2), SCAN_TILE, 0, stream>>>(deg, n, tile_sums, deg2, tile_sums2);
  LAUNCH_CHECK();
  scan_apply_kernel<<<dim3(nb, 2), SCAN_TILE, 0, stream>>>(deg, n, tile_sums, row_ptr, deg2, tile_sums2, row_ptr2);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// reverse-edge index: for e = (i, j) find e' = (j, i) by binary search in row j (cols ascending)
// (erow may alias rev: a thread reads only its own erow slot, before writing it)
__global__ void edge_rev_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col, const int* erow,
                                int n_edges, int* rev) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const int i = erow[e], j = col[e];
  int lo = row_ptr[j], hi = row_ptr[j + 1] - 1, found = -1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const int c = col[mid];
    if (c == i) {
      found = mid;
      break;
    }
    if (c < i) lo = mid + 1; else hi = mid - 1;
  }
  rev[e] = found;
}

// Cutoff envelope and its derivative (fp64).  env > 0: PolynomialCutoff(p = env), representations.py:138-171 (the model uses
// p = 9, :17):  1 - (p+1)(p+2)/2 x^p + p(p+2) x^(p+1) - p(p+1)/2 x^(p+2),  derivative  -p(p+1)(p+2)/2 x^(p-1) (1-x)^2;
// env == NNHIP_ENVELOPE_COSINE: CosineCutoff, representations.py:177-203:  (1 + cos(pi x)) / 2.
__device__ __forceinline__ void envelope_eval(double x, int env, double& e, double& de) {
  if (env == NNHIP_ENVELOPE_COSINE) {
    double sn, cs;
    sincos(3.14159265358979323846 * x, &sn, &cs);
    e = 0.5 * (1.0 + cs);
    de = -0.5 * 3.14159265358979323846 * sn;
  } else if (env == 9) {
    const double x2 = x * x, x4 = x2 * x2, x8 = x4 * x4, x9 = x8 * x;
    e = 1.0 - x9 * (55.0 - 99.0 * x + 45.0 * x2);      // 1 - 55x^9 + 99x^10 - 45x^11
    de = -495.0 * x8 * (1.0 - x) * (1.0 - x);           // -495x^8 + 990x^9 - 495x^10
  } else {
    const double p = (double)env, xp = pow(x, p - 1.0);   // x^(p-1)
    e = 1.0 - 0.5 * (p + 1.0) * (p + 2.0) * xp * x + p * (p + 2.0) * xp * x * x - 0.5 * p * (p + 1.0) * xp * x * x * x;
    de = -0.5 * p * (p + 1.0) * (p + 2.0) * xp * (1.0 - x) * (1.0 - x);
  }
}

// ---------------------------------------------------------------------------------------------
// edge embedding: geo = (dir, r), rbf = env(x) sin(w x)/x, drbf = d rbf/dx.  Evaluated in fp64 and
// rounded once (E x nb values; the cost is negligible next to the [E,F] tensors and it removes the
// cancellation of the p=9 polynomial envelope near x -> 1 from the fp32 error budget).
// ---------------------------------------------------------------------------------------------
// geo / xg of one edge from its displacement (the part of the embedding every path needs); returns x = r / cutoff
__device__ __forceinline__ double edge_embed_geo(int e, float fx, float fy, float fz, float cutoff, float cut2,
                                                 float* __restrict__ geo, int2* __restrict__ xg, bool& inside) {
  const double dx = fx, dy = fy, dz = fz;
  const double r = sqrt(dx * dx + dy * dy + dz * dz);
  const double ir = 1.0 / r;
  float4 g;
  g.x = (float)(dx * ir);
  g.y = (float)(dy * ir);
  g.z = (float)(dz * ir);
  g.w = (float)r;
  reinterpret_cast<float4*>(geo)[e] = g;
  const double x = r / (double)cutoff;
  // Candidates of a reused list (Verlet skin, static training list) that are outside the cutoff right now point at the
  // all-zero filter rows, are masked out of the force kernels and get an all-zero radial basis.  "Outside" is the neighbor
  // list's own fp32 predicate (pair_disp: the reference's `norm < r`), so an edge of the exact list is never masked,
  // whatever the fp64 value of x.
  inside = __fmaf_rn(fz, fz, __fmaf_rn(fy, fy, fx * fx)) < cut2;
  if (xg) {  // position on the radial-filter table grid (edge.hip): interval index and fraction, fraction in fp64 accuracy
    const double t = x * (double)FT_G;
    int g0 = (int)floor(t);
    g0 = g0 < 0 ? 0 : (g0 > FT_G - 1 ? FT_G - 1 : g0);
    xg[e] = inside ? make_int2(g0, __float_as_int((float)(t - (double)g0))) : make_int2(FT_ZERO_ROW, 0);
  }
  return x;
}
__device__ __forceinline__ void edge_embed_one(int e, const float* __restrict__ disp, float cutoff, float cut2, int env_id,
                                               const float* __restrict__ freq, int nb, float* __restrict__ geo,
                                               float* __restrict__ rbf, float* __restrict__ drbf, int2* __restrict__ xg) {
  bool inside;
  const double x = edge_embed_geo(e, disp[3 * (long)e], disp[3 * (long)e + 1], disp[3 * (long)e + 2], cutoff, cut2, geo, xg, inside);
  if (!rbf) return;
  if (!inside) {
    for (int n = 0; n < nb; ++n) {
      rbf[(long)e * nb + n] = 0.f;
      if (drbf) drbf[(long)e * nb + n] = 0.f;
    }
    return;
  }
  double env, denv;
  envelope_eval(x, env_id, env, denv);
  const double ix = 1.0 / x;
  for (int n = 0; n < nb; ++n) {
    const double w = (double)freq[n];
    double s, c;
    sincos(w * x, &s, &c);
    const double bes = s * ix;
    const double dbes = (w * c - bes) * ix;
    rbf[(long)e * nb + n] = (float)(env * bes);
    if (drbf) drbf[(long)e * nb + n] = (float)(denv * bes + env * dbes);
  }
}

__global__ void __launch_bounds__(256)
edge_embed_kernel(const float* __restrict__ disp, int n_edges, float cutoff, float cut2, int env_id, const float* __restrict__ freq, int nb,
                  float* __restrict__ geo, float* __restrict__ rbf, float* __restrict__ drbf, int2* __restrict__ xg) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  edge_embed_one(e, disp, cutoff, cut2, env_id, freq, nb, geo, rbf, drbf, xg);
}

// Everything per-edge that follows the fill, in ONE thread-per-edge launch (the post-count part of the neighbor list sits on the
// critical path of a step behind the host's edge-count round trip: seven tiny launches there cost more than their work):
//   rev[e]  by binary search in row j (edge_rev_kernel);
//   pid[e]  in closed form from pair_ptr, the scan of the per-row counts of upper edges taken by the COUNT pass
//           (pairs_assign_kernel's formula);
//   geo / rbf / drbf / xg of the edge embedding (edge_embed_one).
__global__ void __launch_bounds__(256)
edge_finish_kernel(const int* __restrict__ row_ptr, const int* __restrict__ pair_ptr, const int* __restrict__ col, const int* erow,
                   int n_edges, int* rev, int* __restrict__ pid, const float* __restrict__ disp, float cutoff, float cut2,
                   int env_id, const float* __restrict__ freq, int nb, float* __restrict__ geo, float* __restrict__ rbf,
                   float* __restrict__ drbf, int2* __restrict__ xg, const int* __restrict__ n_edges_dev = nullptr) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (n_edges_dev) {   // early launch: the grid covers the capacity, the count is on the device
    const int cap = n_edges;
    n_edges = *n_edges_dev;
    if (n_edges > cap) return;
  }
  if (e >= n_edges) return;
  const int i = erow[e], j = col[e];
  int lo = row_ptr[j], hi = row_ptr[j + 1] - 1, found = -1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const int c = col[mid];
    if (c == i) {
      found = mid;
      break;
    }
    if (c < i) lo = mid + 1; else hi = mid - 1;
  }
  rev[e] = found;
  pid[e] = (j > i) ? pair_ptr[i + 1] - (row_ptr[i + 1] - e) : pair_ptr[j + 1] - (row_ptr[j + 1] - found);
  edge_embed_one(e, disp, cutoff, cut2, env_id, freq, nb, geo, rbf, drbf, xg);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static int graph_count_impl(const float* pos, const float* cell, const int64_t* batch, int32_t n_atoms, int32_t n_mol,
                            float cutoff, int32_t* mol_ptr, int32_t* row_ptr, int32_t* status, int32_t* pair_cnt, void* stream_,
                            const int64_t* z = nullptr, int32_t* pair_scan_scratch = nullptr);
extern "C" int nnhip_graph_count(const float* pos, const float* cell, const int64_t* batch, int32_t n_atoms,
                                 int32_t n_mol, float cutoff, int32_t* mol_ptr, int32_t* row_ptr, int32_t* status,
                                 void* stream_) {
  return graph_count_impl(pos, cell, batch, n_atoms, n_mol, cutoff, mol_ptr, row_ptr, status, nullptr, stream_);
}
extern "C" int nnhip_graph_count_pairs(const float* pos, const float* cell, const int64_t* batch, int32_t n_atoms,
                                       int32_t n_mol, float cutoff, int32_t* mol_ptr, int32_t* row_ptr, int32_t* status,
                                       int32_t* pair_cnt, void* stream_) {
  if (!pair_cnt) {
    nnhip_set_error("nnhip_graph_count_pairs: bad arguments");
    return NNHIP_E_INVALID;
  }
  return graph_count_impl(pos, cell, batch, n_atoms, n_mol, cutoff, mol_ptr, row_ptr, status, pair_cnt, stream_);
}
// pair_ptr[0 .. N] = exclusive scan of the per-row upper-edge counts nnhip_graph_count_pairs left in pair_ptr[0 .. N), in place
extern "C" int nnhip_graph_pair_scan(int32_t* pair_ptr, int32_t n_atoms, int32_t* scan_scratch, void* stream_) {
  if (n_atoms < 0 || !pair_ptr || !scan_scratch) {
    nnhip_set_error("nnhip_graph_pair_scan: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_atoms == 0) {
    HIP_TRY(hipMemsetAsync(pair_ptr, 0, sizeof(int32_t), (hipStream_t)stream_));
    return NNHIP_OK;
  }
  ScopedTimer tm(TC_GRAPH, (hipStream_t)stream_);
  return launch_scan(pair_ptr, n_atoms, pair_ptr, scan_scratch, (hipStream_t)stream_);
}
// z != NULL: the species check rides in mol_ptr_kernel; pair_scan_scratch != NULL (with pair_cnt): pair_cnt is scanned in place in
// the same two launches as row_ptr (what nnhip_graph_pair_scan would do in two more)
extern "C" int nnhip_graph_count_pairs_z(const float* pos, const float* cell, const int64_t* batch, const int64_t* z, int32_t n_atoms,
                                         int32_t n_mol, float cutoff, int32_t* mol_ptr, int32_t* row_ptr, int32_t* status,
                                         int32_t* pair_ptr, int32_t* pair_scan_scratch, void* stream_) {
  if (!pair_ptr || !pair_scan_scratch) {
    nnhip_set_error("nnhip_graph_count_pairs_z: bad arguments");
    return NNHIP_E_INVALID;
  }
  return graph_count_impl(pos, cell, batch, n_atoms, n_mol, cutoff, mol_ptr, row_ptr, status, pair_ptr, stream_, z, pair_scan_scratch);
}
static int graph_count_impl(const float* pos, const float* cell, const int64_t* batch, int32_t n_atoms, int32_t n_mol,
                            float cutoff, int32_t* mol_ptr, int32_t* row_ptr, int32_t* status, int32_t* pair_cnt, void* stream_,
                            const int64_t* z, int32_t* pair_scan_scratch) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_atoms < 0 || n_mol < 0 || !mol_ptr || !row_ptr || !status) {
    nnhip_set_error("nnhip_graph_count: bad arguments");
    return NNHIP_E_INVALID;
  }
  ScopedTimer tm(TC_GRAPH, stream);
  {  // status[0]; status[1..] is scan scratch
    const int n_init = (n_mol > n_atoms ? n_mol : n_atoms) + 1;
    graph_init_kernel<<<cdiv(n_init, 256), 256, 0, stream>>>(status, mol_ptr, n_mol + 1, row_ptr, n_atoms + 1);
    LAUNCH_CHECK();
  }
  if (n_atoms == 0) return NNHIP_OK;
  mol_ptr_kernel<<<cdiv(n_atoms, 256), 256, 0, stream>>>(batch, n_atoms, n_mol, mol_ptr, status, z);
  LAUNCH_CHECK();
  // in-degrees are counted into row_ptr[0..N) and scanned in place
  graph_rows_kernel<false><<<cdiv(n_atoms, 4), 256, 0, stream>>>(pos, cell, batch, mol_ptr, n_atoms, n_mol, cut2_of(cutoff), row_ptr,
                                                                   nullptr, nullptr, nullptr, nullptr, nullptr, 0, pair_cnt, nullptr, status);
  LAUNCH_CHECK();
  if (pair_cnt && pair_scan_scratch)
    return launch_scan2(row_ptr, row_ptr, status + 1, pair_cnt, pair_cnt, pair_scan_scratch, n_atoms, stream);
  {
    const int rc = launch_scan(row_ptr, n_atoms, row_ptr, status + 1, stream);   // status[1..] = scan scratch
    if (rc) return rc;
  }
  return NNHIP_OK;
}

extern "C" int nnhip_graph_fill(const float* pos, const float* cell, const int64_t* batch, const int32_t* mol_ptr,
                                const int32_t* row_ptr, int32_t n_atoms, int32_t n_mol, int32_t n_edges, float cutoff,
                                int32_t* col, int32_t* rev, float* disp, int64_t* edge_index, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_atoms < 0 || n_edges < 0) {
    nnhip_set_error("nnhip_graph_fill: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_atoms == 0 || n_edges == 0) return NNHIP_OK;
  ScopedTimer tm(TC_GRAPH, stream);
  // `rev` doubles as the receiver-of-edge scratch during the fill; edge_rev_kernel then replaces it in place
  graph_rows_kernel<true><<<cdiv(n_atoms, 4), 256, 0, stream>>>(pos, cell, batch, mol_ptr, n_atoms, n_mol, cut2_of(cutoff), nullptr,
                                                                  row_ptr, col, rev, disp, edge_index, n_edges);
  LAUNCH_CHECK();
  edge_rev_kernel<<<cdiv(n_edges, 256), 256, 0, stream>>>(row_ptr, col, rev, n_edges, rev);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// fill + everything per edge, two launches (all-pairs builder; pair_ptr scanned by nnhip_graph_pair_scan)
extern "C" int nnhip_graph_finish(const float* pos, const float* cell, const int64_t* batch, const int32_t* mol_ptr,
                                  const int32_t* row_ptr, const int32_t* pair_ptr, int32_t n_atoms, int32_t n_mol,
                                  int32_t n_edges, float cutoff, int32_t* col, int32_t* rev, int32_t* pid, float* disp,
                                  int64_t* edge_index, const float* frequencies, int32_t n_basis, float* geo, float* rbf,
                                  float* drbf, int32_t* xg, int32_t envelope, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_atoms < 0 || n_edges < 0 || !pair_ptr || n_basis < 1 || n_basis > NNHIP_MAX_NB ||
      (envelope < 0 && envelope != NNHIP_ENVELOPE_COSINE) || envelope > 64) {
    nnhip_set_error("nnhip_graph_finish: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_atoms == 0 || n_edges == 0) return NNHIP_OK;
  ScopedTimer tm(TC_GRAPH, stream);
  graph_rows_kernel<true><<<cdiv(n_atoms, 4), 256, 0, stream>>>(pos, cell, batch, mol_ptr, n_atoms, n_mol, cut2_of(cutoff), nullptr,
                                                                  row_ptr, col, rev, disp, edge_index, n_edges);
  LAUNCH_CHECK();
  edge_finish_kernel<<<cdiv(n_edges, 256), 256, 0, stream>>>(row_ptr, pair_ptr, col, rev, n_edges, rev, pid, disp, cutoff,
                                                             cut2_of(cutoff), envelope ? envelope : 9, frequencies, n_basis, geo,
                                                             rbf, drbf, reinterpret_cast<int2*>(xg));
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// nnhip_graph_finish BEFORE the host knows the edge count: the arrays hold `capacity` edges (edge_index: 2 x capacity int64, its
// two rows written at the TRUE stride, so the first 2 E entries are the contiguous [2][E] result), the kernels read the count
// from row_ptr[n_atoms] and write nothing at all when it exceeds the capacity (the caller then calls nnhip_graph_finish).
// NewtonNet.forward launches this while the host waits for the count: the ~24 us of GPU idle time behind that round trip.
extern "C" int nnhip_graph_finish_early(const float* pos, const float* cell, const int64_t* batch, const int32_t* mol_ptr,
                                        const int32_t* row_ptr, const int32_t* pair_ptr, int32_t n_atoms, int32_t n_mol,
                                        int32_t capacity, float cutoff, int32_t* col, int32_t* rev, int32_t* pid, float* disp,
                                        int64_t* edge_index, const float* frequencies, int32_t n_basis, float* geo, float* rbf,
                                        float* drbf, int32_t* xg, int32_t envelope, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_atoms < 0 || capacity < 0 || !pair_ptr || !row_ptr || n_basis < 1 || n_basis > NNHIP_MAX_NB ||
      (envelope < 0 && envelope != NNHIP_ENVELOPE_COSINE) || envelope > 64) {
    nnhip_set_error("nnhip_graph_finish_early: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_atoms == 0 || capacity == 0) return NNHIP_OK;
  ScopedTimer tm(TC_GRAPH, stream);
  graph_rows_kernel<true><<<cdiv(n_atoms, 4), 256, 0, stream>>>(pos, cell, batch, mol_ptr, n_atoms, n_mol, cut2_of(cutoff), nullptr,
                                                                  row_ptr, col, rev, disp, edge_index, capacity, nullptr,
                                                                  row_ptr + n_atoms);
  LAUNCH_CHECK();
  edge_finish_kernel<<<cdiv(capacity, 256), 256, 0, stream>>>(row_ptr, pair_ptr, col, rev, capacity, rev, pid, disp, cutoff,
                                                              cut2_of(cutoff), envelope ? envelope : 9, frequencies, n_basis, geo,
                                                              rbf, drbf, reinterpret_cast<int2*>(xg), row_ptr + n_atoms);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// A step that never waits for the host (nnhip_energy_forces_dev): nnhip_graph_finish_early + a guard.  When the edge count
// turned out larger than the capacity the fill wrote nothing; the guard then EMPTIES the graph on the device (row_ptr = pair_ptr =
// 0: every kernel of the step that follows sees zero edges and stays inside the arrays) -- the host finds count > capacity in the
// (count, status) words it copied out BEFORE this call and repeats the step with the real count.
// (an invalid batch vector or species -- status bits 1 / 2, which the synchronous path raises on BEFORE it runs the step -- empties
// the graph too: with a broken batch vector the edge set need not be symmetric and pid would index out of the pair arrays)
// "Empty" without touching row_ptr[n_atoms] (which other workgroups of this launch are reading): every row_ptr[k], k < n_atoms,
// is set to the count itself, so every row is [count, count); pair_ptr, whose last entry the pair-row kernels read, goes to zero.
// tail_host (optional): four int32 in pinned host memory (mapped into the device's address space) -- the count, the status bits
// and the prepared block's change counter go to the host by a plain store of this kernel: no copy dispatch, no bubble behind it.
__global__ void __launch_bounds__(256)
graph_guard_kernel(int* __restrict__ row_ptr, int* __restrict__ pair_ptr, int n_atoms, int capacity, const int* __restrict__ status,
                   int* __restrict__ tail_host, const int* __restrict__ changes, int seq) {
  const int count = row_ptr[n_atoms];
  if (tail_host && blockIdx.x == 0 && threadIdx.x == 0) {
    tail_host[0] = count;
    tail_host[1] = status[0];
    tail_host[2] = changes ? changes[0] : 0;
    __threadfence_system();
    // the caller's sequence number LAST: a host that sees it sees the three words (it polls this word instead of waiting on an
    // event -- an event record is a marker packet in the stream and cost a 5.8 us bubble per step)
    __hip_atomic_store(tail_host + 3, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (!(status[0] & (3 | 16 | 32)) && count <= capacity) return;     // (16 / 32: graph_mol_kernel could not build the list)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_atoms) row_ptr[i] = count;
  if (i <= n_atoms) pair_ptr[i] = 0;
}
extern "C" int nnhip_graph_finish_dev(const float* pos, const float* cell, const int64_t* batch, const int32_t* mol_ptr,
                                      int32_t* row_ptr, int32_t* pair_ptr, int32_t n_atoms, int32_t n_mol, int32_t capacity,
                                      float cutoff, int32_t* col, int32_t* rev, int32_t* pid, float* disp, int64_t* edge_index,
                                      const float* frequencies, int32_t n_basis, float* geo, float* rbf, float* drbf, int32_t* xg,
                                      int32_t envelope, const int32_t* status, int32_t* tail_host, const int32_t* changes,
                                      int32_t seq, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!status || capacity < 1) {
    nnhip_set_error("nnhip_graph_finish_dev: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_atoms == 0) return NNHIP_OK;
  ScopedTimer tm(TC_GRAPH, stream);
  const int rc = nnhip_graph_finish_early(pos, cell, batch, mol_ptr, row_ptr, pair_ptr, n_atoms, n_mol, capacity, cutoff, col, rev,
                                          pid, disp, edge_index, frequencies, n_basis, geo, rbf, drbf, xg, envelope, stream_);
  if (rc) return rc;
  graph_guard_kernel<<<cdiv(n_atoms + 1, 256), 256, 0, stream>>>(row_ptr, pair_ptr, n_atoms, capacity, status, tail_host, changes, seq);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// The whole neighbor list of a SMALL system in ONE launch (at most SG_MAX_ATOMS atoms; the deferred step of NewtonNet.forward):
// what nnhip_graph_count_pairs + nnhip_check_species + nnhip_graph_pair_scan + nnhip_graph_finish_dev do in fourteen launches of
// 3-4 us each, as the phases of one 1024-thread workgroup -- molecule extents and species check, per-row degree and upper-edge
// counts (one wave per row, the same ballot scan as graph_rows_kernel), both prefix scans in LDS, the capacity / status decision
// (an emptied graph when the count does not fit or the status word carries an error bit), fill, reverse edges, pair ids and edge
// embedding.  Same device functions, same order: the list is bit-identical to the multi-launch path (tested).
// tail[0] = the TRUE edge count, tail[1] = the status bits, tail[2] = the prepared block's change counter (`changes`, or 0),
// tail[3] = `seq`, stored last; `tail` may be pinned host memory: the words then reach the host by this kernel's own stores.
// ---------------------------------------------------------------------------------------------
#define SG_MAX_ATOMS 1024
#define SG_THREADS 1024
struct SmallGraphArgs {
  const float* pos; const float* cell; const int64_t* batch; const int64_t* z;
  int n_atoms, n_mol, capacity; float cutoff, cut2;
  int *mol_ptr, *row_ptr, *pair_ptr, *tail, *col, *rev, *pid;   // tail: 3 words, may be pinned HOST memory (count, status, changes)
  const int* changes;                                            // the prepared block's change counter (may be NULL)
  int seq;                                                       // stored into tail[3] after the three words (release, system scope)
  float* disp; int64_t* edge_index; const float* freq; int nb, env; float* geo; int2* xg;
};
__device__ __forceinline__ int sg_block_excl_scan(int v, int* wave_tot, int& total) {   // 1024 threads, one value each
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(inc, o, WAVE);
    if (lane >= o) inc += n;
  }
  if (lane == 63) wave_tot[w] = inc;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < SG_THREADS / 64; ++k) {
    const int t = wave_tot[k];
    before += k < w ? t : 0;
    tot += t;
  }
  __syncthreads();            // (wave_tot is reused by the next scan)
  total = tot;
  return before + inc - v;
}
__global__ void __launch_bounds__(SG_THREADS) graph_small_kernel(const SmallGraphArgs a) {
  __shared__ int s_status, s_ok, s_edges;
  __shared__ int rp[SG_MAX_ATOMS + 1], pp[SG_MAX_ATOMS + 1], wave_tot[SG_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int N = a.n_atoms, B = a.n_mol;
  if (t == 0) s_status = 0;
  for (int k = t; k <= B; k += SG_THREADS) a.mol_ptr[k] = 0;
  __syncthreads();
  // ---- molecule extents (mol_ptr_kernel) + species check (check_species_kernel)
  if (t < N) {
    const long b = a.batch[t];
    const long bp = (t == 0) ? -1 : a.batch[t - 1];
    if (b < bp || b < 0 || b >= B) {
      atomicOr(&s_status, 1);
    } else {
      for (long k = bp + 1; k <= b; ++k) a.mol_ptr[k] = t;
      if (t == N - 1)
        for (long k = b + 1; k <= B; ++k) a.mol_ptr[k] = N;
    }
    if (a.z) {
      const long zi = a.z[t];
      if (zi < 0 || zi >= NNHIP_N_ELEMENTS) atomicOr(&s_status, 2);
    }
  }
  __syncthreads();
  // ---- degrees and upper-edge counts, one wave per row (graph_rows_kernel<false>)
  for (int i = wave; i < N; i += SG_THREADS / 64) {
    const long b = a.batch[i];
    int cnt = 0, cnt_up = 0;
    if (b >= 0 && b < B) {
      const int s = a.mol_ptr[b], e = a.mol_ptr[b + 1];
      if (lane == 0 && i == s && e - s > NNHIP_MOL_STAGE_MAX) atomicOr(&s_status, 8);   // (as graph_rows_kernel<false>)
      const CellInfo ci = load_cell(a.cell, b);
      const float xi = a.pos[3 * i], yi = a.pos[3 * i + 1], zi = a.pos[3 * i + 2];
      for (int j0 = s; j0 < e; j0 += 64) {
        const int j = j0 + lane;
        bool hit = false;
        float dx = 0.f, dy = 0.f, dz = 0.f;
        if (j < e && j != i) hit = pair_disp(xi, yi, zi, a.pos[3 * j], a.pos[3 * j + 1], a.pos[3 * j + 2], ci, dx, dy, dz) < a.cut2;
        cnt += __popcll(__ballot(hit));
        cnt_up += __popcll(__ballot(hit && j > i));
      }
    }
    if (lane == 0) {
      rp[i] = cnt;
      pp[i] = cnt_up;
    }
  }
  __syncthreads();
  // ---- both exclusive scans
  {
    int total, total_up;
    const int d = t < N ? rp[t] : 0, u = t < N ? pp[t] : 0;
    const int ex = sg_block_excl_scan(d, wave_tot, total);
    const int exu = sg_block_excl_scan(u, wave_tot, total_up);
    if (t < N) {
      rp[t] = ex;
      pp[t] = exu;
    }
    if (t == 0) {
      rp[N] = total;
      pp[N] = total_up;
      const int st = s_status;
      s_edges = total;
      s_ok = (!(st & 3) && total <= a.capacity) ? 1 : 0;
      a.tail[0] = total;
      a.tail[1] = st;
      a.tail[2] = a.changes ? a.changes[0] : 0;
      __threadfence_system();
      __hip_atomic_store(a.tail + 3, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  __syncthreads();
  const int E = s_edges;
  const bool ok = s_ok != 0;
  for (int k = t; k <= N; k += SG_THREADS) {     // (an emptied graph when the step must not run on this list: graph_guard_kernel)
    a.row_ptr[k] = ok ? rp[k] : 0;
    a.pair_ptr[k] = ok ? pp[k] : 0;
  }
  if (!ok) return;
  // ---- fill (graph_rows_kernel<true>; `rev` doubles as the receiver-of-edge scratch)
  for (int i = wave; i < N; i += SG_THREADS / 64) {
    const long b = a.batch[i];
    const int s = a.mol_ptr[b], e = a.mol_ptr[b + 1];
    const CellInfo ci = load_cell(a.cell, b);
    const float xi = a.pos[3 * i], yi = a.pos[3 * i + 1], zi = a.pos[3 * i + 2];
    int w = rp[i];
    for (int j0 = s; j0 < e; j0 += 64) {
      const int j = j0 + lane;
      bool hit = false;
      float dx = 0.f, dy = 0.f, dz = 0.f;
      if (j < e && j != i) hit = pair_disp(xi, yi, zi, a.pos[3 * j], a.pos[3 * j + 1], a.pos[3 * j + 2], ci, dx, dy, dz) < a.cut2;
      const unsigned long long mask = __ballot(hit);
      if (hit) {
        const int o = w + __popcll(mask & ((1ull << lane) - 1ull));
        a.col[o] = j;
        a.rev[o] = i;
        a.disp[3 * (long)o] = dx;
        a.disp[3 * (long)o + 1] = dy;
        a.disp[3 * (long)o + 2] = dz;
        if (a.edge_index) {
          a.edge_index[o] = i;
          a.edge_index[(long)E + o] = j;
        }
      }
      w += __popcll(mask);
    }
  }
  __syncthreads();
  // ---- reverse edge, pair id, edge embedding (edge_finish_kernel)
  for (int e = t; e < E; e += SG_THREADS) {
    const int i = a.rev[e], j = a.col[e];
    int lo = rp[j], hi = rp[j + 1] - 1, found = -1;
    while (lo <= hi) {
      const int mid = (lo + hi) >> 1;
      const int c = a.col[mid];
      if (c == i) {
        found = mid;
        break;
      }
      if (c < i) lo = mid + 1; else hi = mid - 1;
    }
    a.rev[e] = found;
    a.pid[e] = (j > i) ? pp[i + 1] - (rp[i + 1] - e) : pp[j + 1] - (rp[j + 1] - found);
    edge_embed_one(e, a.disp, a.cutoff, a.cut2, a.env, a.freq, a.nb, a.geo, nullptr, nullptr, a.xg);
  }
}
extern "C" int nnhip_graph_small_dev(const float* pos, const float* cell, const int64_t* batch, const int64_t* z, int32_t n_atoms,
                                     int32_t n_mol, int32_t capacity, float cutoff, int32_t* mol_ptr, int32_t* row_ptr,
                                     int32_t* pair_ptr, int32_t* tail, const int32_t* changes, int32_t seq, int32_t* col, int32_t* rev,
                                     int32_t* pid, float* disp,
                                     int64_t* edge_index, const float* frequencies, int32_t n_basis, float* geo, int32_t* xg,
                                     int32_t envelope, void* stream_) {
  if (n_atoms < 1 || n_atoms > SG_MAX_ATOMS || n_mol < 0 || capacity < 2 || !tail || !mol_ptr || !row_ptr || !pair_ptr || n_basis < 1 ||
      n_basis > NNHIP_MAX_NB || (envelope < 0 && envelope != NNHIP_ENVELOPE_COSINE) || envelope > 64) {
    nnhip_set_error("nnhip_graph_small_dev: bad arguments (1..%d atoms)", SG_MAX_ATOMS);
    return NNHIP_E_INVALID;
  }
  ScopedTimer tm(TC_GRAPH, (hipStream_t)stream_);
  SmallGraphArgs a = {pos, cell, batch, z, n_atoms, n_mol, capacity, cutoff, cut2_of(cutoff), mol_ptr, row_ptr, pair_ptr, tail,
                      col, rev, pid, changes, seq, disp, edge_index, frequencies, n_basis, envelope ? envelope : 9, geo,
                      reinterpret_cast<int2*>(xg)};
  graph_small_kernel<<<1, SG_THREADS, 0, (hipStream_t)stream_>>>(a);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
// What the deferred step sends through the single launch: systems of at most this many atoms (the kernel itself serves up to
// SG_MAX_ATOMS = 1024).  One workgroup walks the rows 16 at a time, so the launch loses to the parallel kernels beyond ~100-150
// atoms (back-to-back aspirin batches, us per step, single launch vs fourteen: 21 atoms 182 vs 206, 84: 207 vs 216, 168: 218 vs 208,
// 336: 257 vs 231, 1008: 390 vs 255; profiles/r04_small_thresholds.txt).  NNHIP_GRAPH_SMALL_ATOMS overrides (0 = never).
extern "C" int nnhip_graph_small_max_atoms(void) {
  const int n = switches().graph_small_atoms;   // (default 128)
  return n < 0 ? 0 : (n > SG_MAX_ATOMS ? SG_MAX_ATOMS : n);
}

// ---------------------------------------------------------------------------------------------
// The neighbor list of a batch of SMALL molecules, a workgroup per molecule, in TWO launches (the deferred step of
// NewtonNet.forward when the previous batch of the shape had no molecule above NNHIP_MOL_STAGE_MAX atoms; the kernels themselves
// serve molecules of up to MG_MAX_ATOMS).  What graph_rows_kernel<count> + two dual-scan launches + graph_rows_kernel<fill> +
// edge_finish_kernel do in five launches of 5-11 us, the molecule's positions, row_ptr / pair_ptr and col staged in LDS:
//   graph_mol_count_kernel: per-row degree and upper-edge counts (a wave per row, the same ballot scan), both prefix scans of the
//     molecule in LDS -> row_ptr / pair_ptr of the molecule's rows RELATIVE to the molecule, and the molecule's edge total;
//   graph_mol_fill_kernel: the molecule's offset = the sum of the totals before it (one coalesced pass over <= MG_SUM_MAX totals
//     by the whole workgroup; above that a scan launch in between), row_ptr / pair_ptr made absolute, fill, edge embedding from the
//     registers that hold each displacement, reverse edges and pair ids by a search over the LDS col.
// A molecule's pairs = its edges / 2 (the edge set is symmetric), so one offset serves both arrays.  Same device functions, same
// order: the list is bit-identical to the multi-launch path (tested).  (A single launch with a look-back over published totals was
// built first: 24 us, of which 12 us waiting for words to cross between the XCDs' L2s -- and a workgroup counter for "who is
// last" cost 33 us more: 1024 atomics on one address.  Two launches without any waiting: profiles/r04_graph_mol_*.)
// status bits set here: 8 (a molecule above NNHIP_MOL_STAGE_MAX atoms), 16 (a molecule above MG_MAX_ATOMS: its rows are not
// built -- graph_guard_kernel empties the graph).
// ---------------------------------------------------------------------------------------------
#define MG_MAX_ATOMS 1024
#define MG_THREADS 512
#define MG_LDS_EDGES 4096
#define MG_SUM_MAX 8192
struct MolGraphArgs {
  const float* pos; const float* cell; const int* mol_ptr;
  int n_atoms, n_mol, capacity; float cutoff, cut2;
  int *row_ptr, *pair_ptr, *status; int* mol_edges; const int* mol_base;   // mol_base: the scanned totals (n_mol > MG_SUM_MAX) or NULL
  int *col, *rev, *pid; float* disp; float* geo; int2* xg;
};
__device__ __forceinline__ int mg_extent(const MolGraphArgs& a, int b, int& s) {
  s = a.mol_ptr[b];
  int n = a.mol_ptr[b + 1] - s;
  if (n > MG_MAX_ATOMS) n = -1;      // (rows not built: status bit 16)
  return n;
}
__global__ void __launch_bounds__(MG_THREADS) graph_mol_count_kernel(const MolGraphArgs a) {
  __shared__ int rp[MG_MAX_ATOMS + 1], pp[MG_MAX_ATOMS + 1];
  __shared__ float spos[3 * MG_MAX_ATOMS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x;
  int s;
  int n = mg_extent(a, b, s);
  if (n < 0) {
    if (t == 0) atomicOr(a.status, 8 | 16);
    n = 0;
  }
  if (t == 0 && n > NNHIP_MOL_STAGE_MAX) atomicOr(a.status, 8);
  for (int k = t; k < 3 * n; k += MG_THREADS) spos[k] = a.pos[3 * (long)s + k];
  const CellInfo ci = load_cell(a.cell, b);
  __syncthreads();
  // ---- degrees and upper-edge counts (graph_rows_kernel<false>)
  for (int k = wave; k < n; k += MG_THREADS / 64) {
    const float xi = spos[3 * k], yi = spos[3 * k + 1], zi = spos[3 * k + 2];
    int cnt = 0, cnt_up = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int j = j0 + lane;
      bool hit = false;
      float dx = 0.f, dy = 0.f, dz = 0.f;
      if (j < n && j != k) hit = pair_disp(xi, yi, zi, spos[3 * j], spos[3 * j + 1], spos[3 * j + 2], ci, dx, dy, dz) < a.cut2;
      cnt += __popcll(__ballot(hit));
      cnt_up += __popcll(__ballot(hit && j > k));
    }
    if (lane == 0) {
      rp[k] = cnt;
      pp[k] = cnt_up;
    }
  }
  __syncthreads();
  // ---- both exclusive scans of the molecule, by one wave, 64 rows at a time
  if (wave == 0) {
    int run = 0, run_up = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
      const int k = k0 + lane;
      const int v = k < n ? rp[k] : 0, u = k < n ? pp[k] : 0;
      int inc = v, inc_up = u;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(inc, o, WAVE), y = __shfl_up(inc_up, o, WAVE);
        if (lane >= o) inc += x, inc_up += y;
      }
      if (k < n) {      // (relative to the molecule; graph_mol_fill_kernel adds its offset)
        a.row_ptr[s + k] = run + inc - v;
        a.pair_ptr[s + k] = run_up + inc_up - u;
      }
      run += __shfl(inc, 63, WAVE);
      run_up += __shfl(inc_up, 63, WAVE);
    }
    if (lane == 0) a.mol_edges[b] = run;
  }
}
__global__ void __launch_bounds__(MG_THREADS) graph_mol_fill_kernel(const MolGraphArgs a) {
  __shared__ int rp[MG_MAX_ATOMS + 1], pp[MG_MAX_ATOMS + 1];
  __shared__ float spos[3 * MG_MAX_ATOMS];       // the molecule's positions: the row pass reads nothing else from global memory
  __shared__ int scol[MG_LDS_EDGES];             // the molecule's col (when it fits): the reverse-edge search stays in LDS
  __shared__ int s_base;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x, B = a.n_mol, N = a.n_atoms;
  // An invalid batch vector (bit 1: unsorted or out of range -- mol_ptr_kernel's racing writes can then leave molecule extents that
  // overlap, so that two workgroups would fill the same rows from different offsets), a species outside the tables (2) or a
  // molecule this kernel does not serve (16): the status word is final after the two launches before this one, the guard behind
  // it empties the graph, the host raises what the synchronous path raises -- nothing is filled.  
  if (a.status[0] & (1 | 2 | 16)) return;   // (uniform)
  int s;
  int n = mg_extent(a, b, s);
  if (n < 0) n = 0;
  if (t == 0) s_base = 0;
  for (int k = t; k < 3 * n; k += MG_THREADS) spos[k] = a.pos[3 * (long)s + k];
  for (int k = t; k < n; k += MG_THREADS) {
    rp[k] = a.row_ptr[s + k];
    pp[k] = a.pair_ptr[s + k];
  }
  const int total = a.mol_edges[b];
  const CellInfo ci = load_cell(a.cell, b);
  __syncthreads();
  // ---- the molecule's offset in the edge list
  int base;
  if (a.mol_base) {
    base = a.mol_base[b];
  } else {
    int part = 0;
    for (int q = t; q < b; q += MG_THREADS) part += a.mol_edges[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, WAVE);
    if (lane == 0 && part) atomicAdd(&s_base, part);
    __syncthreads();
    base = s_base;
  }
  const int pair_base = base >> 1;
  for (int k = t; k < n; k += MG_THREADS) {
    rp[k] += base;
    pp[k] += pair_base;
    a.row_ptr[s + k] = rp[k];
    a.pair_ptr[s + k] = pp[k];
  }
  if (t == 0) {
    rp[n] = base + total;
    pp[n] = pair_base + (total >> 1);
    if (b == B - 1) {
      a.row_ptr[N] = base + total;
      a.pair_ptr[N] = pair_base + (total >> 1);
    }
  }
  __syncthreads();
  const int e0 = rp[0], e1 = rp[n];
  if (e1 > a.capacity) return;             // (uniform; this molecule's edges would not lie inside the arrays: the guard empties the graph)
  const bool lds_col = e1 - e0 <= MG_LDS_EDGES;
  // ---- fill (graph_rows_kernel<true>) + the edge embedding of each edge from the registers that hold its displacement
  for (int k = wave; k < n; k += MG_THREADS / 64) {
    const float xi = spos[3 * k], yi = spos[3 * k + 1], zi = spos[3 * k + 2];
    int w = rp[k];
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int j = j0 + lane;
      bool hit = false;
      float dx = 0.f, dy = 0.f, dz = 0.f;
      if (j < n && j != k) hit = pair_disp(xi, yi, zi, spos[3 * j], spos[3 * j + 1], spos[3 * j + 2], ci, dx, dy, dz) < a.cut2;
      const unsigned long long mask = __ballot(hit);
      const int o = w + __popcll(mask & ((1ull << lane) - 1ull));
      if (hit && o < e1) {   // (o < e1 <= capacity always holds for consistent counts; the predicate keeps every store inside the arrays)
        a.col[o] = s + j;
        if (lds_col) scol[o - e0] = s + j;
        a.disp[3 * (long)o] = dx;
        a.disp[3 * (long)o + 1] = dy;
        a.disp[3 * (long)o + 2] = dz;
        bool inside;
        edge_embed_geo(o, dx, dy, dz, a.cutoff, a.cut2, a.geo, a.xg, inside);
      }
      w += __popcll(mask);
    }
  }
  __syncthreads();
  // ---- reverse edge and pair id (edge_finish_kernel), row by row: the receiver is the row, the search runs over the LDS col
  for (int k = wave; k < n; k += MG_THREADS / 64) {
    const int i = s + k;
    for (int e = rp[k] + lane; e < rp[k + 1]; e += 64) {
      const int j = lds_col ? scol[e - e0] : a.col[e];
      int lo = rp[j - s], hi = rp[j - s + 1] - 1, found = -1;
      while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int c = lds_col ? scol[mid - e0] : a.col[mid];
        if (c == i) {
          found = mid;
          break;
        }
        if (c < i) lo = mid + 1; else hi = mid - 1;
      }
      a.rev[e] = found;
      a.pid[e] = (j > i) ? pp[k + 1] - (rp[k + 1] - e) : pp[j - s + 1] - (rp[j - s + 1] - found);
    }
  }
}
// Launches: [graph_init_kernel (status, mol_ptr, row_ptr) unless `initialised`], mol_ptr_kernel (molecule extents + species check:
// status bits 1 / 2), graph_mol_count_kernel, [a scan of the molecule totals when n_mol > MG_SUM_MAX], graph_mol_fill_kernel,
// graph_guard_kernel.  scratch: 2 n_mol + n_mol / 1024 + 4 ints (any content).
extern "C" int nnhip_graph_mol_dev(const float* pos, const float* cell, const int64_t* batch, const int64_t* z, int32_t n_atoms,
                                   int32_t n_mol, int32_t capacity, float cutoff, int32_t* mol_ptr, int32_t* row_ptr,
                                   int32_t* pair_ptr, int32_t* status, int32_t* scratch, int32_t initialised,
                                   int32_t* tail_host, const int32_t* changes, int32_t seq, int32_t* col,
                                   int32_t* rev, int32_t* pid, float* disp, float* geo, int32_t* xg, void* stream_) {
  if (n_atoms < 1 || n_mol < 1 || capacity < 2 || !batch || !mol_ptr || !row_ptr || !pair_ptr || !status || !scratch || !col ||
      !rev || !pid || !disp || !geo || !xg) {
    nnhip_set_error("nnhip_graph_mol_dev: bad arguments");
    return NNHIP_E_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  ScopedTimer tm(TC_GRAPH, stream);
  if (!initialised) {
    const int n_init = (n_mol > n_atoms ? n_mol : n_atoms) + 1;
    graph_init_kernel<<<cdiv(n_init, 256), 256, 0, stream>>>(status, mol_ptr, n_mol + 1, row_ptr, n_atoms + 1);
    LAUNCH_CHECK();
  }
  mol_ptr_kernel<<<cdiv(n_atoms, 256), 256, 0, stream>>>(batch, n_atoms, n_mol, mol_ptr, status, z);
  LAUNCH_CHECK();
  int* mol_edges = scratch;
  int* mol_base = n_mol > MG_SUM_MAX ? scratch + n_mol + 1 : nullptr;
  MolGraphArgs a = {pos, cell, mol_ptr, n_atoms, n_mol, capacity, cutoff, cut2_of(cutoff), row_ptr, pair_ptr, status, mol_edges,
                    mol_base, col, rev, pid, disp, geo, reinterpret_cast<int2*>(xg)};
  graph_mol_count_kernel<<<n_mol, MG_THREADS, 0, stream>>>(a);
  LAUNCH_CHECK();
  if (mol_base) {
    const int rc = launch_scan(mol_edges, n_mol, mol_base, scratch + 2 * n_mol + 2, stream);
    if (rc) return rc;
  }
  graph_mol_fill_kernel<<<n_mol, MG_THREADS, 0, stream>>>(a);
  LAUNCH_CHECK();
  graph_guard_kernel<<<cdiv(n_atoms + 1, 256), 256, 0, stream>>>(row_ptr, pair_ptr, n_atoms, capacity, status, tail_host, changes, seq);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// edge_index [2][E] int64 (the reference's API array) from the CSR list, for callers that ask for it after the fact (the deferred
// step does not write it: most evaluation steps never look at it): row 0 = the receiver of edge e (binary search in row_ptr),
// row 1 = col[e].
__global__ void __launch_bounds__(256)
edge_index_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col, int n_atoms, int n_edges, int64_t* __restrict__ out,
                  const int* __restrict__ n_edges_dev) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (n_edges_dev) {   // the grid covers the capacity of `out`, the count is on the device (row 1 starts at the TRUE count)
    const int cap = n_edges;
    n_edges = *n_edges_dev;
    if (n_edges > cap) return;
  }
  if (e >= n_edges) return;
  int lo = 0, hi = n_atoms - 1;          // the last row with row_ptr[i] <= e
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (row_ptr[mid] <= e) lo = mid; else hi = mid - 1;
  }
  out[e] = lo;
  out[(long)n_edges + e] = col[e];
}
extern "C" int nnhip_edge_index_from_csr(const int32_t* row_ptr, const int32_t* col, int32_t n_atoms, int32_t n_edges,
                                         int64_t* edge_index, const int32_t* n_edges_dev, void* stream_) {
  if (n_atoms < 0 || n_edges < 0 || (n_edges && (!row_ptr || !col || !edge_index || n_atoms < 1))) {
    nnhip_set_error("nnhip_edge_index_from_csr: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_edges == 0) return NNHIP_OK;
  edge_index_kernel<<<cdiv(n_edges, 256), 256, 0, (hipStream_t)stream_>>>(row_ptr, col, n_atoms, n_edges, edge_index, n_edges_dev);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// Radial-filter tables of one layer, nodes x_g = g / FT_G (row = g + 1; fp64 evaluation, one rounding per entry):
//   T[g][f] = sum_n W_e[f][n] rbf_n(x_g)                         (values; node -1 = the analytic continuation to x < 0)
//   S[g][f] = (eps_f(x_g+1) - eps_f(x_g)) FT_G                   (secant slopes, differenced in fp64)
//   D[g][f] = sum_n W_e[f][n] d rbf_n/dx (x_g)                   (derivatives)
// three planes of FT_ROWS rows (edge_common.h says who reads what); every row read is one coalesced 16-byte-per-lane instruction.
struct FilterTableArgs {
  const float* edge_w[NNHIP_MAX_LAYERS];
  float* table[NNHIP_MAX_LAYERS];
  const float* freq;
  int nb;
  int env;
};
__device__ __forceinline__ void radial_basis_f64(double x, double w, int env_id, double& rb, double& drb) {
  if (x >= 1.0) {   // at and beyond the cutoff the filter is identically zero (the polynomial envelope itself is not)
    rb = drb = 0.0;
    return;
  }
  double env, denv;
  envelope_eval(x, env_id, env, denv);
  double bes, dbes;
  if (x == 0.0) {
    bes = w;       // sin(wx)/x -> w
    dbes = 0.0;    // even function of x
  } else {
    double sn, cs;
    sincos(w * x, &sn, &cs);
    bes = sn / x;
    dbes = (w * cs - bes) / x;
  }
  rb = env * bes;
  drb = denv * bes + env * dbes;
}
__global__ void __launch_bounds__(NF) filter_table_kernel(FilterTableArgs a) {
  __shared__ double rb[NNHIP_MAX_NB], drb[NNHIP_MAX_NB], rb1[NNHIP_MAX_NB];
  const int nb = a.nb;
  const int row = blockIdx.x, l = blockIdx.y, g = row - 1;
  float* __restrict__ out = a.table[l] + (size_t)row * NF + threadIdx.x;
  if (g > FT_G) {   // beyond the cutoff: all-zero rows
    out[0] = out[FT_PLANE] = out[2 * FT_PLANE] = 0.f;
    return;
  }
  if (threadIdx.x < nb) {
    const double w = (double)a.freq[threadIdx.x];
    double unused;
    radial_basis_f64((double)g / (double)FT_G, w, a.env, rb[threadIdx.x], drb[threadIdx.x]);
    radial_basis_f64((double)(g + 1) / (double)FT_G, w, a.env, rb1[threadIdx.x], unused);
  }
  __syncthreads();
  const float* __restrict__ we = a.edge_w[l] + (size_t)threadIdx.x * nb;
  double acc = 0.0, dacc = 0.0, sacc = 0.0;
  for (int n = 0; n < nb; ++n) {
    const double wn = (double)we[n];
    acc += wn * rb[n];
    dacc += wn * drb[n];
    sacc += wn * (rb1[n] - rb[n]);
  }
  out[0] = (float)acc;
  out[FT_PLANE] = (float)(sacc * (double)FT_G);
  out[2 * FT_PLANE] = (float)dacc;
}

int launch_filter_tables(const float* const* edge_w, float* const* tables, int n_layers, const float* freq, int nb,
                         int envelope, hipStream_t s) {
  ScopedTimer tm(TC_OTHER, s);
  FilterTableArgs a;
  for (int l = 0; l < n_layers; ++l) {
    a.edge_w[l] = edge_w[l];
    a.table[l] = tables[l];
  }
  a.freq = freq;
  a.nb = nb;
  a.env = envelope ? envelope : 9;
  filter_table_kernel<<<dim3(FT_ROWS, n_layers), NF, 0, s>>>(a);
  LAUNCH_CHECK();
  return 0;
}

// Displacements of a FIXED candidate list at new positions (Verlet-skin reuse in an MD loop: the list was built with
// cutoff + skin, nnhip_edge_embed then zeroes the candidates that are outside the cutoff at this step).  Same pair_disp as
// the list builders, so an edge that is in the exact list gets the identical displacement.
__global__ void __launch_bounds__(256)
edge_disp_kernel(const float* __restrict__ pos, const float* __restrict__ cell, const int64_t* __restrict__ batch,
                 const int64_t* __restrict__ edge_index, int n_edges, float* __restrict__ disp) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const long i = edge_index[e], j = edge_index[(long)n_edges + e];
  const CellInfo ci = load_cell(cell, batch[i]);
  float dx, dy, dz;
  pair_disp(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ci, dx, dy, dz);
  disp[3 * (long)e] = dx;
  disp[3 * (long)e + 1] = dy;
  disp[3 * (long)e + 2] = dz;
}

extern "C" int nnhip_edge_disp(const float* pos, const float* cell, const int64_t* batch, const int64_t* edge_index,
                               int32_t n_edges, float* disp, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_edges < 0 || (n_edges && (!pos || !cell || !batch || !edge_index || !disp))) {
    nnhip_set_error("nnhip_edge_disp: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_edges == 0) return NNHIP_OK;
  ScopedTimer tm(TC_GRAPH, stream);
  edge_disp_kernel<<<cdiv(n_edges, 256), 256, 0, stream>>>(pos, cell, batch, edge_index, n_edges, disp);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// nnhip_edge_disp + nnhip_edge_embed in one thread-per-edge launch (the per-step geometry refresh of a reused list: two
// dependent launches of a few microseconds of work each cost their latency twice in the 31-launch MD step)
__global__ void __launch_bounds__(256)
edge_refresh_kernel(const float* __restrict__ pos, const float* __restrict__ cell, const int64_t* __restrict__ batch,
                    const int64_t* __restrict__ edge_index, int n_edges, float* __restrict__ disp, float cutoff, float cut2, int env_id,
                    const float* __restrict__ freq, int nb, float* __restrict__ geo, float* __restrict__ rbf, float* __restrict__ drbf,
                    int2* __restrict__ xg) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const long i = edge_index[e], j = edge_index[(long)n_edges + e];
  const CellInfo ci = load_cell(cell, batch[i]);
  float dx, dy, dz;
  pair_disp(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ci, dx, dy, dz);
  disp[3 * (long)e] = dx;
  disp[3 * (long)e + 1] = dy;
  disp[3 * (long)e + 2] = dz;
  edge_embed_one(e, disp, cutoff, cut2, env_id, freq, nb, geo, rbf, drbf, xg);
}
extern "C" int nnhip_edge_refresh(const float* pos, const float* cell, const int64_t* batch, const int64_t* edge_index,
                                  int32_t n_edges, float cutoff, const float* frequencies, int32_t n_basis, float* disp, float* geo,
                                  float* rbf, float* drbf, int32_t* xg, int32_t envelope, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_edges < 0 || (n_edges && (!pos || !cell || !batch || !edge_index || !disp || !geo)) || n_basis < 1 ||
      n_basis > NNHIP_MAX_NB || (envelope < 0 && envelope != NNHIP_ENVELOPE_COSINE) || envelope > 64) {
    nnhip_set_error("nnhip_edge_refresh: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_edges == 0) return NNHIP_OK;
  ScopedTimer tm(TC_GRAPH, stream);
  edge_refresh_kernel<<<cdiv(n_edges, 256), 256, 0, stream>>>(pos, cell, batch, edge_index, n_edges, disp, cutoff, cut2_of(cutoff),
                                                              envelope ? envelope : 9, frequencies, n_basis, geo, rbf, drbf,
                                                              reinterpret_cast<int2*>(xg));
  LAUNCH_CHECK();
  return NNHIP_OK;
}

extern "C" int nnhip_edge_embed(const float* disp, int32_t n_edges, float cutoff, const float* frequencies,
                                int32_t n_basis, float* geo, float* rbf, float* drbf, int32_t* xg, int32_t envelope,
                                void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_basis < 1 || n_basis > NNHIP_MAX_NB || (envelope < 0 && envelope != NNHIP_ENVELOPE_COSINE) || envelope > 64) {
    nnhip_set_error("nnhip_edge_embed: n_basis=%d (1..%d) / envelope=%d unsupported", n_basis, NNHIP_MAX_NB, envelope);
    return NNHIP_E_UNSUPPORTED;
  }
  if (n_edges == 0) return NNHIP_OK;
  ScopedTimer tm(TC_GRAPH, stream);
  edge_embed_kernel<<<cdiv(n_edges, 256), 256, 0, stream>>>(disp, n_edges, cutoff, cut2_of(cutoff), envelope ? envelope : 9, frequencies, n_basis, geo, rbf, drbf,
                                                            reinterpret_cast<int2*>(xg));
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// =============================================================================================
// O(N) neighbor list for ONE large orthorhombic periodic box (BASELINE config 5: 100k atoms, which the
// reference's O(N^2) all-pairs build cannot hold in memory).
//
// Same predicate, same displacement arithmetic (pair_disp) and same (i, j)-ascending edge order as the
// all-pairs kernel above, so the two paths return bit-identical lists; only the candidate set is pruned:
// atoms are binned on a grid of cells >= cutoff wide, a row looks at the 27 surrounding cells, and each
// row is sorted by j.  Preconditions (checked by the caller, newtonnet_amd/hip.py): one molecule, diagonal
// cell, every box length >= 3 cells.  Integer atomics only (bin counters): the result is deterministic.
// =============================================================================================
struct CellGrid {
  int nb[3];
  float inv_len[3];  // 1 / L_k
};

__device__ __forceinline__ int bin_coord(float p, float inv_len, int nb) {
  float s = p * inv_len;
  s -= floorf(s);                      // wrapped fractional coordinate in [0, 1)
  int b = (int)(s * (float)nb);
  return b >= nb ? nb - 1 : (b < 0 ? 0 : b);
}

__global__ void __launch_bounds__(256)
cells_bin_count_kernel(const float* __restrict__ pos, int n_atoms, CellGrid g, int* __restrict__ bin_of,
                       int* __restrict__ bin_cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  const int bx = bin_coord(pos[3 * i], g.inv_len[0], g.nb[0]);
  const int by = bin_coord(pos[3 * i + 1], g.inv_len[1], g.nb[1]);
  const int bz = bin_coord(pos[3 * i + 2], g.inv_len[2], g.nb[2]);
  const int b = (bx * g.nb[1] + by) * g.nb[2] + bz;
  bin_of[i] = b;
  atomicAdd(&bin_cnt[b], 1);
}

__global__ void __launch_bounds__(256)
cells_bin_fill_kernel(const int* __restrict__ bin_of, const int* __restrict__ bin_ptr, int n_atoms,
                      int* __restrict__ cursor, int* __restrict__ bin_atoms) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  const int b = bin_of[i];
  bin_atoms[bin_ptr[b] + atomicAdd(&cursor[b], 1)] = i;
}

template <bool FILL>
__global__ void __launch_bounds__(256)
cells_rows_kernel(const float* __restrict__ pos, const float* __restrict__ cell, const int* __restrict__ bin_of,
                  const int* __restrict__ bin_ptr, const int* __restrict__ bin_atoms, CellGrid g, int n_atoms,
                  float cut2, int* __restrict__ deg, const int* __restrict__ row_ptr, int* col,
                  int* __restrict__ erow, float* __restrict__ disp, int64_t* __restrict__ edge_index, int n_edges) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  const CellInfo ci = load_cell(cell, 0);
  const float xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
  const int b = bin_of[i];
  const int bz = b % g.nb[2], by = (b / g.nb[2]) % g.nb[1], bx = b / (g.nb[2] * g.nb[1]);
  const int base = FILL ? row_ptr[i] : 0;
  int cnt = 0;
  for (int dx = -1; dx <= 1; ++dx) {
    const int cx = (bx + dx + g.nb[0]) % g.nb[0];
    for (int dy = -1; dy <= 1; ++dy) {
      const int cy = (by + dy + g.nb[1]) % g.nb[1];
      for (int dz = -1; dz <= 1; ++dz) {
        const int cz = (bz + dz + g.nb[2]) % g.nb[2];
        const int cb = (cx * g.nb[1] + cy) * g.nb[2] + cz;
        for (int k = bin_ptr[cb]; k < bin_ptr[cb + 1]; ++k) {
          const int j = bin_atoms[k];
          if (j == i) continue;
          float ddx, ddy, ddz;
          const float r2 = pair_disp(xi, yi, zi, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ci, ddx, ddy, ddz);
          if (r2 < cut2) {
            if (FILL) {  // insertion sort by j inside this row's slice of col[]
              int p = base + cnt;
              while (p > base && col[p - 1] > j) {
                col[p] = col[p - 1];
                --p;
              }
              col[p] = j;
            }
            ++cnt;
          }
        }
      }
    }
  }
  if (!FILL) {
    deg[i] = cnt;
    return;
  }
  for (int w = base; w < base + cnt; ++w) {
    const int j = col[w];
    float ddx, ddy, ddz;
    pair_disp(xi, yi, zi, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ci, ddx, ddy, ddz);
    erow[w] = i;
    disp[3 * (long)w] = ddx;
    disp[3 * (long)w + 1] = ddy;
    disp[3 * (long)w + 2] = ddz;
    if (edge_index) {
      edge_index[w] = i;
      edge_index[(long)n_edges + w] = j;
    }
  }
}

// Count pass, one wave per receiver atom: degree and the number of neighbors above the atom (the pairs the row owns)
__global__ void __launch_bounds__(256)
cells_count_wave_kernel(const float* __restrict__ pos, const float* __restrict__ cell, const int* __restrict__ bin_of,
                        const int* __restrict__ bin_ptr, const int* __restrict__ bin_atoms, CellGrid g, int n_atoms, float cut2,
                        int* __restrict__ deg, int* __restrict__ upper) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_atoms) return;
  const CellInfo ci = load_cell(cell, 0);
  const float xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
  const int b = bin_of[i];
  const int bz = b % g.nb[2], by = (b / g.nb[2]) % g.nb[1], bx = b / (g.nb[2] * g.nb[1]);
  int cnt = 0, cnt_up = 0;
  for (int dx = -1; dx <= 1; ++dx)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dz = -1; dz <= 1; ++dz) {
        const int cb = (((bx + dx + g.nb[0]) % g.nb[0]) * g.nb[1] + (by + dy + g.nb[1]) % g.nb[1]) * g.nb[2] + (bz + dz + g.nb[2]) % g.nb[2];
        const int kend = bin_ptr[cb + 1];
        for (int k0 = bin_ptr[cb]; k0 < kend; k0 += 64) {
          const int k = k0 + lane;
          const int j = k < kend ? bin_atoms[k] : -1;
          bool hit = false;
          if (j >= 0 && j != i) {
            float ddx, ddy, ddz;
            hit = pair_disp(xi, yi, zi, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ci, ddx, ddy, ddz) < cut2;
          }
          cnt += __popcll(__ballot(hit));
          cnt_up += __popcll(__ballot(hit && j > i));
        }
      }
  if (lane == 0) {
    deg[i] = cnt;
    if (upper) upper[i] = cnt_up;
  }
}

// Fill pass, one WAVE per receiver atom (the thread-per-atom insertion sort above is kept for the count pass and for rows of
// more than CW_CAP neighbors): the lanes test the atoms of the 27 surrounding cells 64 at a time, ballot-compact the hits into a
// per-wave LDS list, rank-sort it (keys are distinct: rank = number of smaller keys) and write the row in ascending j with its
// displacements -- the same set, the same pair_disp and the same order as cells_rows_kernel<true>, 1.5 ms -> ~0.2 ms on the
// 100k-atom box.
#define CW_CAP 256
__global__ void __launch_bounds__(256)
cells_fill_wave_kernel(const float* __restrict__ pos, const float* __restrict__ cell, const int* __restrict__ bin_of,
                       const int* __restrict__ bin_ptr, const int* __restrict__ bin_atoms, CellGrid g, int n_atoms, float cut2,
                       const int* __restrict__ row_ptr, int* col, int* __restrict__ erow, float* __restrict__ disp,
                       int64_t* __restrict__ edge_index, int n_edges) {
  __shared__ int list[4][CW_CAP];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n_atoms) return;
  const int base = row_ptr[i], deg = row_ptr[i + 1] - base;
  if (deg == 0) return;
  const CellInfo ci = load_cell(cell, 0);
  const float xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
  const int b = bin_of[i];
  const int bz = b % g.nb[2], by = (b / g.nb[2]) % g.nb[1], bx = b / (g.nb[2] * g.nb[1]);
  if (deg > CW_CAP) {   // a row too long for the list: the serial form, on one lane
    if (lane != 0) return;
    int cnt = 0;
    for (int dx = -1; dx <= 1; ++dx)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dz = -1; dz <= 1; ++dz) {
          const int cb = (((bx + dx + g.nb[0]) % g.nb[0]) * g.nb[1] + (by + dy + g.nb[1]) % g.nb[1]) * g.nb[2] + (bz + dz + g.nb[2]) % g.nb[2];
          for (int k = bin_ptr[cb]; k < bin_ptr[cb + 1]; ++k) {
            const int j = bin_atoms[k];
            if (j == i) continue;
            float ddx, ddy, ddz;
            if (pair_disp(xi, yi, zi, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ci, ddx, ddy, ddz) < cut2) {
              int p = base + cnt;
              while (p > base && col[p - 1] > j) {
                col[p] = col[p - 1];
                --p;
              }
              col[p] = j;
              ++cnt;
            }
          }
        }
    for (int w = base; w < base + cnt; ++w) {
      const int j = col[w];
      float ddx, ddy, ddz;
      pair_disp(xi, yi, zi, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ci, ddx, ddy, ddz);
      erow[w] = i;
      disp[3 * (long)w] = ddx;
      disp[3 * (long)w + 1] = ddy;
      disp[3 * (long)w + 2] = ddz;
      if (edge_index) {
        edge_index[w] = i;
        edge_index[(long)n_edges + w] = j;
      }
    }
    return;
  }
  int* L = list[wave];
  int cnt = 0;
  for (int dx = -1; dx <= 1; ++dx)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dz = -1; dz <= 1; ++dz) {
        const int cb = (((bx + dx + g.nb[0]) % g.nb[0]) * g.nb[1] + (by + dy + g.nb[1]) % g.nb[1]) * g.nb[2] + (bz + dz + g.nb[2]) % g.nb[2];
        const int kend = bin_ptr[cb + 1];
        for (int k0 = bin_ptr[cb]; k0 < kend; k0 += 64) {
          const int k = k0 + lane;
          const int j = k < kend ? bin_atoms[k] : -1;
          bool hit = false;
          if (j >= 0 && j != i) {
            float ddx, ddy, ddz;
            hit = pair_disp(xi, yi, zi, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ci, ddx, ddy, ddz) < cut2;
          }
          const unsigned long long mask = __ballot(hit);
          if (hit) L[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = j;
          cnt += __popcll(mask);
        }
      }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (one wave's LDS operations complete in issue order)
  __builtin_amdgcn_wave_barrier();
  for (int t = lane; t < deg; t += 64) {
    const int j = L[t];
    int rank = 0;
    for (int u = 0; u < deg; ++u) rank += (L[u] < j);
    const int w = base + rank;
    float ddx, ddy, ddz;
    pair_disp(xi, yi, zi, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], ci, ddx, ddy, ddz);
    col[w] = j;
    erow[w] = i;
    disp[3 * (long)w] = ddx;
    disp[3 * (long)w + 1] = ddy;
    disp[3 * (long)w + 2] = ddz;
    if (edge_index) {
      edge_index[w] = i;
      edge_index[(long)n_edges + w] = j;
    }
  }
}

static int make_grid(const float* box_len_host, float cutoff, CellGrid& g, int& n_bins) {
  n_bins = 1;
  for (int k = 0; k < 3; ++k) {
    if (!(box_len_host[k] > 0.f)) return NNHIP_E_INVALID;
    g.nb[k] = (int)floorf(box_len_host[k] / (cutoff * 1.0001f));  // cells strictly wider than the cutoff
    if (g.nb[k] < 3) return NNHIP_E_UNSUPPORTED;
    if (g.nb[k] > 1024) g.nb[k] = 1024;
    g.inv_len[k] = 1.0f / box_len_host[k];
    n_bins *= g.nb[k];
  }
  return NNHIP_OK;
}

// scratch: bin_of[N] | bin_cnt/bin_ptr[n_bins+1] | cursor[n_bins] | bin_atoms[N] | scan_tmp[max(N, n_bins)/1024 + 1]   (int32)
extern "C" size_t nnhip_graph_cells_scratch_bytes(int32_t n_atoms, const float* box_len_host, float cutoff) {
  CellGrid g;
  int n_bins;
  if (make_grid(box_len_host, cutoff, g, n_bins) != NNHIP_OK) return 0;
  return sizeof(int32_t) * ((size_t)2 * n_atoms + 2 * (size_t)n_bins + 2 + (size_t)(n_atoms > n_bins ? n_atoms : n_bins) / 1024 + 2);
}

static int* scan_tmp_of(void* scratch, int n_atoms, const float* box_len_host, float cutoff) {
  CellGrid g;
  int n_bins = 0;
  make_grid(box_len_host, cutoff, g, n_bins);
  return (int*)scratch + 2 * (size_t)n_atoms + 2 * (size_t)n_bins + 1;
}

static int cells_common(const float* pos, int n_atoms, const float* box_len_host, float cutoff, void* scratch,
                        CellGrid& g, int*& bin_of, int*& bin_ptr, int*& cursor, int*& bin_atoms, bool build,
                        hipStream_t stream) {
  int n_bins;
  const int rc = make_grid(box_len_host, cutoff, g, n_bins);
  if (rc != NNHIP_OK) {
    nnhip_set_error("nnhip_graph_*_cells: box must be orthorhombic with every length >= 3 x cutoff");
    return rc;
  }
  int* s = (int*)scratch;
  bin_of = s;
  bin_ptr = s + n_atoms;
  cursor = bin_ptr + n_bins + 1;
  bin_atoms = cursor + n_bins;
  int* scan_tmp = bin_atoms + n_atoms;
  if (build) {
    HIP_TRY(hipMemsetAsync(bin_ptr, 0, sizeof(int) * (2 * (size_t)n_bins + 1), stream));
    cells_bin_count_kernel<<<cdiv(n_atoms, 256), 256, 0, stream>>>(pos, n_atoms, g, bin_of, bin_ptr);
    LAUNCH_CHECK();
    {
      const int rc2 = launch_scan(bin_ptr, n_bins, bin_ptr, scan_tmp, stream);
      if (rc2) return rc2;
    }
    cells_bin_fill_kernel<<<cdiv(n_atoms, 256), 256, 0, stream>>>(bin_of, bin_ptr, n_atoms, cursor, bin_atoms);
    LAUNCH_CHECK();
  }
  return NNHIP_OK;
}

static int count_cells_impl(const float* pos, const float* cell, int32_t n_atoms, float cutoff, const float* box_len_host,
                            void* scratch, int32_t* mol_ptr, int32_t* row_ptr, int32_t* pair_cnt, void* stream_);
extern "C" int nnhip_graph_count_cells(const float* pos, const float* cell, int32_t n_atoms, float cutoff,
                                       const float* box_len_host, void* scratch, int32_t* mol_ptr, int32_t* row_ptr,
                                       void* stream_) {
  return count_cells_impl(pos, cell, n_atoms, cutoff, box_len_host, scratch, mol_ptr, row_ptr, nullptr, stream_);
}
extern "C" int nnhip_graph_count_cells_pairs(const float* pos, const float* cell, int32_t n_atoms, float cutoff,
                                             const float* box_len_host, void* scratch, int32_t* mol_ptr, int32_t* row_ptr,
                                             int32_t* pair_cnt, void* stream_) {
  if (!pair_cnt) {
    nnhip_set_error("nnhip_graph_count_cells_pairs: bad arguments");
    return NNHIP_E_INVALID;
  }
  return count_cells_impl(pos, cell, n_atoms, cutoff, box_len_host, scratch, mol_ptr, row_ptr, pair_cnt, stream_);
}
static int count_cells_impl(const float* pos, const float* cell, int32_t n_atoms, float cutoff, const float* box_len_host,
                            void* scratch, int32_t* mol_ptr, int32_t* row_ptr, int32_t* pair_cnt, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_atoms <= 0 || !scratch || !row_ptr || !mol_ptr) {
    nnhip_set_error("nnhip_graph_count_cells: bad arguments");
    return NNHIP_E_INVALID;
  }
  ScopedTimer tm(TC_GRAPH, stream);
  CellGrid g;
  int *bin_of, *bin_ptr, *cursor, *bin_atoms;
  const int rc = cells_common(pos, n_atoms, box_len_host, cutoff, scratch, g, bin_of, bin_ptr, cursor, bin_atoms, true, stream);
  if (rc) return rc;
  const int32_t mp[2] = {0, n_atoms};
  HIP_TRY(hipMemcpyAsync(mol_ptr, mp, sizeof(mp), hipMemcpyHostToDevice, stream));
  cells_count_wave_kernel<<<cdiv(n_atoms, 4), 256, 0, stream>>>(pos, cell, bin_of, bin_ptr, bin_atoms, g, n_atoms, cut2_of(cutoff), row_ptr,
                                                                pair_cnt);
  LAUNCH_CHECK();
  {
    const int rc2 = launch_scan(row_ptr, n_atoms, row_ptr, scan_tmp_of(scratch, n_atoms, box_len_host, cutoff), stream);
    if (rc2) return rc2;
  }
  return NNHIP_OK;
}

extern "C" int nnhip_graph_fill_cells(const float* pos, const float* cell, int32_t n_atoms, int32_t n_edges, float cutoff,
                                      const float* box_len_host, void* scratch, const int32_t* row_ptr, int32_t* col,
                                      int32_t* rev, float* disp, int64_t* edge_index, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_atoms <= 0 || n_edges < 0 || !scratch) {
    nnhip_set_error("nnhip_graph_fill_cells: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_edges == 0) return NNHIP_OK;
  ScopedTimer tm(TC_GRAPH, stream);
  CellGrid g;
  int *bin_of, *bin_ptr, *cursor, *bin_atoms;
  const int rc = cells_common(pos, n_atoms, box_len_host, cutoff, scratch, g, bin_of, bin_ptr, cursor, bin_atoms, false, stream);
  if (rc) return rc;
  cells_fill_wave_kernel<<<cdiv(n_atoms, 4), 256, 0, stream>>>(pos, cell, bin_of, bin_ptr, bin_atoms, g, n_atoms, cut2_of(cutoff), row_ptr,
                                                               col, rev, disp, edge_index, n_edges);
  LAUNCH_CHECK();
  edge_rev_kernel<<<cdiv(n_edges, 256), 256, 0, stream>>>(row_ptr, col, rev, n_edges, rev);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// nnhip_graph_fill_cells + pair ids + edge embedding in two launches (pair_ptr from nnhip_graph_count_cells_pairs, scanned by
// nnhip_graph_pair_scan): the cell-list counterpart of nnhip_graph_finish
extern "C" int nnhip_graph_finish_cells(const float* pos, const float* cell, int32_t n_atoms, int32_t n_edges, float cutoff,
                                        const float* box_len_host, void* scratch, const int32_t* row_ptr, const int32_t* pair_ptr,
                                        int32_t* col, int32_t* rev, int32_t* pid, float* disp, int64_t* edge_index,
                                        const float* frequencies, int32_t n_basis, float* geo, float* rbf, float* drbf, int32_t* xg,
                                        int32_t envelope, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_atoms <= 0 || n_edges < 0 || !scratch || !pair_ptr || n_basis < 1 || n_basis > NNHIP_MAX_NB ||
      (envelope < 0 && envelope != NNHIP_ENVELOPE_COSINE) || envelope > 64) {
    nnhip_set_error("nnhip_graph_finish_cells: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_edges == 0) return NNHIP_OK;
  ScopedTimer tm(TC_GRAPH, stream);
  CellGrid g;
  int *bin_of, *bin_ptr, *cursor, *bin_atoms;
  const int rc = cells_common(pos, n_atoms, box_len_host, cutoff, scratch, g, bin_of, bin_ptr, cursor, bin_atoms, false, stream);
  if (rc) return rc;
  cells_fill_wave_kernel<<<cdiv(n_atoms, 4), 256, 0, stream>>>(pos, cell, bin_of, bin_ptr, bin_atoms, g, n_atoms, cut2_of(cutoff), row_ptr,
                                                               col, rev, disp, edge_index, n_edges);
  LAUNCH_CHECK();
  edge_finish_kernel<<<cdiv(n_edges, 256), 256, 0, stream>>>(row_ptr, pair_ptr, col, rev, n_edges, rev, pid, disp, cutoff,
                                                             cut2_of(cutoff), envelope ? envelope : 9, frequencies, n_basis, geo,
                                                             rbf, drbf, reinterpret_cast<int2*>(xg));
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// =============================================================================================
// Undirected pairs.  The message of an edge, msg = (W_e rbf) * m[i] * m[j] (newtonnet.py:211), is symmetric under
// i <-> j, hence so is everything the two edge MLPs compute from it (equiv_message1/2, newtonnet.py:218,222):
// phi_k(i,j) == phi_k(j,i).  The hot path therefore evaluates msg / h / phi once per UNDIRECTED pair and lets both
// directed edges read the same row: half the MFMA work and half the [E,128] traffic of the dominant kernels.
//   pid[e]      pair index of directed edge e; pairs are numbered in CSR order of their upper edge (i < j), so the
//               upper edges of a row own a contiguous run of pair rows
//   pair_ptr[i] first pair owned by row i (exclusive scan of the number of upper edges per row)
// =============================================================================================
__global__ void __launch_bounds__(256)
pairs_count_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col, int n_atoms, int* __restrict__ n_upper) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  int c = 0;
  for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) c += (col[e] > i);
  n_upper[i] = c;
}

// pid in closed form, one pass: the pairs owned by row r are numbered pair_ptr[r] .. pair_ptr[r+1]) in the order of r's
// upper edges, which are the LAST n_upper(r) edges of the row (cols ascend).  So the upper edge at position e of row r
// has pid = pair_ptr[r+1] - (row_ptr[r+1] - e), and a lower edge (i, j), j < i, takes the number of its reverse (j, i).
__global__ void __launch_bounds__(256)
pairs_assign_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col, const int* __restrict__ rev,
                    const int* __restrict__ pair_ptr, int n_atoms, int* __restrict__ pid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  const int end = row_ptr[i + 1], pend = pair_ptr[i + 1];
  for (int e = row_ptr[i]; e < end; ++e) {
    const int j = col[e];
    pid[e] = (j > i) ? pend - (end - e) : pair_ptr[j + 1] - (row_ptr[j + 1] - rev[e]);
  }
}

extern "C" int nnhip_graph_pairs(const int32_t* row_ptr, const int32_t* col, const int32_t* rev, int32_t n_atoms,
                                 int32_t n_edges, int32_t* pair_ptr, int32_t* pid, int32_t* scan_scratch, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_atoms < 0 || n_edges < 0 || !pair_ptr || (n_edges && (!pid || !scan_scratch))) {
    nnhip_set_error("nnhip_graph_pairs: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_atoms == 0 || n_edges == 0) {
    HIP_TRY(hipMemsetAsync(pair_ptr, 0, sizeof(int32_t) * (n_atoms + 1), stream));
    return NNHIP_OK;
  }
  ScopedTimer tm(TC_GRAPH, stream);   // pairs_count + the scan write every pair_ptr entry
  pairs_count_kernel<<<cdiv(n_atoms, 64), 64, 0, stream>>>(row_ptr, col, n_atoms, pair_ptr);
  LAUNCH_CHECK();
  {
    const int rc = launch_scan(pair_ptr, n_atoms, pair_ptr, scan_scratch, stream);
    if (rc) return rc;
  }
  pairs_assign_kernel<<<cdiv(n_atoms, 64), 64, 0, stream>>>(row_ptr, col, rev, pair_ptr, n_atoms, pid);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// =============================================================================================
// Internal spatial order of ONE big system (round 6).  The step of a single molecule of >= 16 384 atoms runs on
// its atoms in Morton order of cells (models/newtonnet.py) so that the partner rows of a pair lie tens to hundreds of rows apart
// whatever order the caller stores the atoms in.  Round 5 built the permutation from torch ops (LUT gathers, a stable argsort, two
// index_selects; a second argsort over all edges when edge_index is asked for); here it is the library's own kernels:
//   1. bounding box of the positions (one workgroup); cells of max(cutoff, extent / 64) per axis, so at most 64^3 Morton keys
//   2. count atoms per key (integer atomics), scan, place atoms into their key's slots (atomic cursor), then ONE thread per key
//      sorts its few atoms by input index -- the order is "by key, then by input index", i.e. deterministic, as a stable sort's
//   3. z and pos gathered through the permutation in the same launch that writes perm / inv
// and, for callers that ask for the neighbor list, nnhip_edge_index_unpermute lists the permuted CSR in the reference's order for
// the CALLER's atom order (rows by ascending i, neighbors by ascending j, representations.py:74-98) with a scan and a rank-by-counting
// pass per row instead of a sort over all edges.
// =============================================================================================
#define SO_BITS 6
#define SO_CELLS (1 << SO_BITS)                    // cells per axis at most
#define SO_KEYS (1 << (3 * SO_BITS))               // 262 144 Morton keys
#define SO_SORT_MAX 2048                           // atoms of one key that are still sorted by input index
__device__ __forceinline__ unsigned so_spread(unsigned v) {      // 6 bits -> every third bit
  v &= 0x3fu;
  v = (v | (v << 8)) & 0x300fu;
  v = (v | (v << 4)) & 0x30c3u;
  v = (v | (v << 2)) & 0x9249u;
  return v;
}
__global__ void __launch_bounds__(1024) so_bbox_kernel(const float* __restrict__ pos, int n_atoms, float cutoff, float* __restrict__ box /*[6]*/) {
  __shared__ float red[16][6];
  float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (int i = threadIdx.x; i < n_atoms; i += 1024)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float p = pos[3 * i + k];
      lo[k] = fminf(lo[k], p);
      hi[k] = fmaxf(hi[k], p);
    }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      lo[k] = fminf(lo[k], __shfl_xor(lo[k], d));
      hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d));
    }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      red[threadIdx.x >> 6][k] = lo[k];
      red[threadIdx.x >> 6][3 + k] = hi[k];
    }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    float l = red[0][k], h = red[0][3 + k];
    for (int w = 1; w < 16; ++w) {
      l = fminf(l, red[w][k]);
      h = fmaxf(h, red[w][3 + k]);
    }
    const float ext = fmaxf(h - l, 0.0f);
    const float cell = fmaxf(cutoff, ext * (1.0f / ((float)SO_CELLS - 0.001f)));     // every coordinate lands in [0, SO_CELLS)
    box[k] = l;
    box[3 + k] = 1.0f / cell;
  }
}
__device__ __forceinline__ int so_key(const float* __restrict__ pos, int i, const float* __restrict__ box) {
  unsigned c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float s = (pos[3 * i + k] - box[k]) * box[3 + k];
    const int ci = (int)s;                               // (s >= 0 up to rounding: truncation = floor)
    c[k] = (unsigned)(ci < 0 ? 0 : (ci > SO_CELLS - 1 ? SO_CELLS - 1 : ci));
  }
  return (int)((so_spread(c[0]) << 2) | (so_spread(c[1]) << 1) | so_spread(c[2]));
}
__global__ void __launch_bounds__(256) so_count_kernel(const float* __restrict__ pos, int n_atoms, const float* __restrict__ box,
                                                       int* __restrict__ key_of, int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_atoms) return;
  const int key = so_key(pos, i, box);
  key_of[i] = key;
  atomicAdd(&cnt[key], 1);
}
__global__ void __launch_bounds__(256) so_fill_kernel(const int* __restrict__ key_of, const int* __restrict__ key_ptr, int n_atoms,
                                                      int* __restrict__ cursor, int* __restrict__ slots) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_atoms) return;
  const int key = key_of[i];
  slots[key_ptr[key] + atomicAdd(&cursor[key], 1)] = i;
}
// one thread per key: its atoms by ascending input index (a handful per key; whatever order the atomics placed them in, the
// result is the same), then perm / inv and the permuted z / pos
__global__ void __launch_bounds__(256) so_finish_kernel(const int* __restrict__ key_ptr, int* __restrict__ slots, const int64_t* __restrict__ z,
                                                        const float* __restrict__ pos, int32_t* __restrict__ perm, int32_t* __restrict__ inv,
                                                        int64_t* __restrict__ z_out, float* __restrict__ pos_out) {
  const int key = blockIdx.x * 256 + threadIdx.x;
  if (key >= SO_KEYS) return;
  const int b = key_ptr[key], e = key_ptr[key + 1];
  // (a cell of a real system holds a handful of atoms.  Thousands in ONE cell -- a broken input, e.g. every position equal -- would
  // make this quadratic loop run for minutes in one thread: such a cell keeps the order the atomics gave it, still a permutation)
  for (int a = b + 1; a < e && e - b <= SO_SORT_MAX; ++a) {          // insertion sort
    const int v = slots[a];
    int q = a - 1;
    while (q >= b && slots[q] > v) {
      slots[q + 1] = slots[q];
      --q;
    }
    slots[q + 1] = v;
  }
  for (int k = b; k < e; ++k) {
    const int i = slots[k];
    perm[k] = i;
    inv[i] = k;
    if (z_out) z_out[k] = z[i];
    if (pos_out) {
      pos_out[3 * k] = pos[3 * i];
      pos_out[3 * k + 1] = pos[3 * i + 1];
      pos_out[3 * k + 2] = pos[3 * i + 2];
    }
  }
}
// ints of scratch: box (8) | key_of [N] | cnt -> key_ptr [KEYS + 1] | cursor [KEYS] | slots [N] | scan tiles
extern "C" size_t nnhip_spatial_order_scratch_bytes(int32_t n_atoms) {
  if (n_atoms < 0) return 0;
  return sizeof(int32_t) * (8 + 2 * (size_t)n_atoms + 2 * (size_t)SO_KEYS + 1 + (size_t)SO_KEYS / SCAN_TILE + 2);
}
extern "C" int nnhip_spatial_order(const float* pos, const int64_t* z, int32_t n_atoms, float cutoff, int32_t* perm, int32_t* inv,
                                   int64_t* z_out, float* pos_out, void* scratch, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!pos || n_atoms < 1 || !(cutoff > 0.0f) || !perm || !inv || !scratch || (z_out && !z)) {
    nnhip_set_error("nnhip_spatial_order: bad arguments");
    return NNHIP_E_INVALID;
  }
  ScopedTimer tm(TC_GRAPH, stream);
  int* s = (int*)scratch;
  float* box = (float*)s;
  int* key_of = s + 8;
  int* key_ptr = key_of + n_atoms;            // counts, then (in place) their exclusive scan
  int* cursor = key_ptr + SO_KEYS + 1;
  int* slots = cursor + SO_KEYS;
  int* scan_tmp = slots + n_atoms;
  HIP_TRY(hipMemsetAsync(key_ptr, 0, sizeof(int) * (2 * (size_t)SO_KEYS + 1), stream));
  so_bbox_kernel<<<1, 1024, 0, stream>>>(pos, n_atoms, cutoff, box);
  LAUNCH_CHECK();
  so_count_kernel<<<cdiv(n_atoms, 256), 256, 0, stream>>>(pos, n_atoms, box, key_of, key_ptr);
  LAUNCH_CHECK();
  {
    const int rc = launch_scan(key_ptr, SO_KEYS, key_ptr, scan_tmp, stream);
    if (rc) return rc;
  }
  so_fill_kernel<<<cdiv(n_atoms, 256), 256, 0, stream>>>(key_of, key_ptr, n_atoms, cursor, slots);
  LAUNCH_CHECK();
  so_finish_kernel<<<SO_KEYS / 256, 256, 0, stream>>>(key_ptr, slots, z, pos, perm, inv, z_out, pos_out);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// out[k][0..width) = x[idx[k]][0..width)   (any width; the per-atom results of a permuted step back in the caller's order: idx = inv)
__global__ void __launch_bounds__(256) permute_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx, long n_elems,
                                                           int width, float* __restrict__ out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_elems) return;
  const long k = t / width;
  const int c = (int)(t - k * width);
  out[t] = x[(long)idx[k] * width + c];
}
extern "C" int nnhip_permute_rows(const float* x, const int32_t* idx, int32_t n_rows, int32_t width, float* out, void* stream_) {
  if (n_rows < 0 || width < 1 || (n_rows && (!x || !idx || !out))) {
    nnhip_set_error("nnhip_permute_rows: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_rows == 0) return NNHIP_OK;
  const long n = (long)n_rows * width;
  permute_rows_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream_>>>(x, idx, n, width, out);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// The neighbor list of a permuted step as the reference lists it for the caller's atom order.  Row a of the output is row inv[a] of
// the permuted CSR with every neighbor mapped back (j = perm[j_p]) and the row sorted by j: rank by counting inside the row (a wave
// per row; rows hold tens of entries).
__global__ void __launch_bounds__(256) unperm_degree_kernel(const int* __restrict__ row_ptr_p, const int32_t* __restrict__ inv, int n_atoms,
                                                            int* __restrict__ deg) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a < n_atoms) deg[a] = row_ptr_p[inv[a] + 1] - row_ptr_p[inv[a]];
}
__global__ void __launch_bounds__(256) unperm_rows_kernel(const int* __restrict__ row_ptr_p, const int* __restrict__ col_p,
                                                          const int32_t* __restrict__ perm, const int32_t* __restrict__ inv,
                                                          const int* __restrict__ start, int n_atoms, long n_edges,
                                                          int64_t* __restrict__ edge_index) {
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= n_atoms) return;
  const int lane = threadIdx.x & 63;
  const int rb = row_ptr_p[inv[a]], re = row_ptr_p[inv[a] + 1], d = re - rb;
  const long o = start[a];
  for (int c0 = 0; c0 < d; c0 += 64) {                 // my element(s)
    const int mine = c0 + lane < d ? perm[col_p[rb + c0 + lane]] : 0x7fffffff;
    int rank = 0;
    for (int q0 = 0; q0 < d; q0 += 64) {               // ... against every element of the row (distinct values: a neighbor occurs once)
      const int other = q0 + lane < d ? perm[col_p[rb + q0 + lane]] : 0x7fffffff;
      const int lim = min(64, d - q0);
      for (int t = 0; t < lim; ++t) rank += __shfl(other, t) < mine ? 1 : 0;
    }
    if (c0 + lane < d) {
      edge_index[o + rank] = a;
      edge_index[n_edges + o + rank] = mine;
    }
  }
}
// scratch: (n_atoms + 1 + n_atoms / 1024 + 2) ints
extern "C" int nnhip_edge_index_unpermute(const int32_t* row_ptr_p, const int32_t* col_p, const int32_t* perm, const int32_t* inv,
                                          int32_t n_atoms, int32_t n_edges, int64_t* edge_index, int32_t* scratch, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_atoms < 1 || n_edges < 0 || !row_ptr_p || !perm || !inv || !scratch || (n_edges && (!col_p || !edge_index))) {
    nnhip_set_error("nnhip_edge_index_unpermute: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_edges == 0) return NNHIP_OK;
  int* start = scratch;
  unperm_degree_kernel<<<cdiv(n_atoms, 256), 256, 0, stream>>>(row_ptr_p, inv, n_atoms, start);
  LAUNCH_CHECK();
  {
    const int rc = launch_scan(start, n_atoms, start, scratch + n_atoms + 1, stream);
    if (rc) return rc;
  }
  unperm_rows_kernel<<<cdiv(n_atoms, 4), 256, 0, stream>>>(row_ptr_p, col_p, perm, inv, start, n_atoms, (long)n_edges, edge_index);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
