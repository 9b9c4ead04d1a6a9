// Analytic elastic constants of crystals (gfx950, fp32): the strain tangent pass and the relaxed-ion term.
//
// A homogeneous strain eps maps every position x -> (1 + eps) x, the cell with it, so every stored displacement vector of the
// graph moves as d_e -> (1 + eps) d_e (d_e = r_e u_e already holds its periodic shift).  The tangent-over-reverse pass of the
// Hessian (csrc/train_step.hip: tangent_sweeps with the layer hook of csrc/hessian.hip) is generic in the edge tangent
// tgeo = (du, dx); seeded with dd_e = eta d_e instead of v_i - v_j it returns dg_d[e], the tangent of g_d[e] = dE/dd_e along
// the strain eta.  From it
//   dgrad[i] = sum_{e in row i} dg_d[e] - dg_d[rev e]      = d(dE/dpos_i)/d eta   (the row gather of the Hessian, unchanged)
//   S_ab     = sum_e dg_d[e]_a d_e,b                       = d(dE/d eps_ab)/d eta (strain_born_kernel; dE/d eps_ab = sum_e g_d_a d_b
//              is linear in d_e and d_e is linear in eps, so there is no g (x) dd term)
// Voigt components with engineering shears: eps = [[e1, e6/2, e5/2], [e6/2, e2, e4/2], [e5/2, e4/2, e3]]; every system of
// the batch has its own eta6, so R replicas of a batch carry R strains through one pass (newtonnet_amd/elastic.py).
//
// Relaxed-ion term of a crystal with n_b atoms per primitive cell (d = 3 n_b):
//   elastic_fold_kernel   Phi0[i a][j b] = sum over the supercell copies J of j of fc[i][a][J][b]  (the force constants at Gamma),
//                         symmetrised, packed [n_b][3][n_b][3] as the blocks of nnhip_eig_blocks; a crystal whose sc_atoms is no
//                         multiple of its atoms is not folded and says so in status
//   elastic_relax_kernel  R_IJ = sum_m (q_m . Lambda_I)(q_m . Lambda_J) / lambda_m over the eigenpairs of Phi0 with |lambda_m|
//                         above the crystal's zero threshold, ascending in lambda; one wave per crystal
// nnhip_strain_vp itself is in csrc/train_step.hip, next to the static sweeps it drives; the launchers of its two kernels are here.
// No float atomics: one writer per output, every sum in a fixed order with fp64 accumulators, so two calls are bitwise equal.
#include "common.h"

namespace {

// eps = sum_I e_I M_I as a symmetric 3 x 3 (xx, yy, zz, yz, xz, xy)
__device__ __forceinline__ void voigt_matrix(const float* __restrict__ e, float m[6]) {
  m[0] = e[0];
  m[1] = e[1];
  m[2] = e[2];
  m[3] = 0.5f * e[3];
  m[4] = 0.5f * e[4];
  m[5] = 0.5f * e[5];
}

// ---------------------------------------------------------------------------------------------
// the seed: tgeo[e] = (du, dx) of dd = eta (r u).  One lane per directed edge; a masked candidate of a reused list gets the same
// arithmetic as in edge_tan_geom_kernel (train.hip) -- its tangents are zeroed downstream by the xg test.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
strain_tan_geom_kernel(const int64_t* __restrict__ edge_index, const int64_t* __restrict__ batch, const float* __restrict__ geo,
                       const float* __restrict__ eta6, int n_edges, float inv_rc, float* __restrict__ tgeo) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const long i = edge_index[e];
  float m[6];
  voigt_matrix(eta6 + 6 * (size_t)batch[i], m);
  const float4 g = reinterpret_cast<const float4*>(geo)[e];
  const float dx = g.w * (m[0] * g.x + m[5] * g.y + m[4] * g.z);
  const float dy = g.w * (m[5] * g.x + m[1] * g.y + m[3] * g.z);
  const float dz = g.w * (m[4] * g.x + m[3] * g.y + m[2] * g.z);
  const float dr = g.x * dx + g.y * dy + g.z * dz;
  const float ir = 1.0f / g.w;
  reinterpret_cast<float4*>(tgeo)[e] = make_float4((dx - g.x * dr) * ir, (dy - g.y * dr) * ir, (dz - g.z * dr) * ir, dr * inv_rc);
}

// ---------------------------------------------------------------------------------------------
// d2[b][I] = sum_ab (d eps_ab / d e_I) S_ab,  S_ab = sum_e dg_d[e]_a d_e,b over the edges of system b: one wave per system, lane
// per atom row, fp64 sums and a fixed butterfly (as virial_kernel, edge.hip).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
strain_born_kernel(const float* __restrict__ dg_d, const float* __restrict__ geo, const int* __restrict__ row_ptr,
                   const int* __restrict__ mol_ptr, int n_mol, float* __restrict__ d2) {
  const int b = blockIdx.x;
  if (b >= n_mol) return;
  const int lane = threadIdx.x;
  double s[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s[k] = 0.0;
  for (int i = mol_ptr[b] + lane; i < mol_ptr[b + 1]; i += 64) {
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      const float4 t = reinterpret_cast<const float4*>(dg_d)[e];
      const float4 g = reinterpret_cast<const float4*>(geo)[e];
      const double dg[3] = {t.x, t.y, t.z};
      const double d[3] = {(double)g.w * g.x, (double)g.w * g.y, (double)g.w * g.z};
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int q = 0; q < 3; ++q) s[a * 3 + q] += dg[a] * d[q];
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    double v = s[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    s[k] = v;
  }
  if (lane == 0) {
    float* o = d2 + 6 * (size_t)b;
    o[0] = (float)s[0];
    o[1] = (float)s[4];
    o[2] = (float)s[8];
    o[3] = (float)(0.5 * (s[5] + s[7]));
    o[4] = (float)(0.5 * (s[2] + s[6]));
    o[5] = (float)(0.5 * (s[1] + s[3]));
  }
}

// ---------------------------------------------------------------------------------------------
// Phi0 of crystal b = blockIdx.x: the thread of element (p, q), p <= q (p = 3 i + a, q = 3 j + b), sums both fc[i][a][R n + j][b]
// and fc[j][b][R n + i][a] over the copies R ascending and writes their mean to (p, q) and (q, p): exactly symmetric.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
elastic_fold_kernel(const float* __restrict__ fc, const int64_t* __restrict__ fc_ptr, const int* __restrict__ cry_ptr,
                    const int* __restrict__ sc_atoms, const int64_t* __restrict__ out_ptr, float* __restrict__ phi0,
                    int* __restrict__ status) {
  const int b = blockIdx.x;
  const int n = cry_ptr[b + 1] - cry_ptr[b];
  const int N = sc_atoms[b];
  const bool bad = n < 0 || (n > 0 && (N < n || N % n != 0));   // sc_atoms is no multiple of the crystal's atoms (uniform)
  if (blockIdx.y == 0 && threadIdx.x == 0) status[b] = bad ? NNHIP_ELASTIC_STATUS_SIZE : 0;
  if (bad || n == 0) return;
  const int d = 3 * n, copies = N / n;
  const size_t ld = 3 * (size_t)N;
  const float* f = fc + fc_ptr[b];
  float* out = phi0 + out_ptr[b];
  for (int t = blockIdx.y * blockDim.x + threadIdx.x; t < d * d; t += gridDim.y * blockDim.x) {
    const int p = t / d, q = t - p * d;
    if (p > q) continue;
    const int i = p / 3, a = p - 3 * i, j = q / 3, c = q - 3 * j;
    double u = 0.0, l = 0.0;
    for (int r = 0; r < copies; ++r) {
      u += (double)f[(size_t)p * ld + 3 * (size_t)(r * n + j) + c];
      l += (double)f[(size_t)q * ld + 3 * (size_t)(r * n + i) + a];
    }
    const float v = (float)(0.5 * (u + l));
    out[(size_t)p * d + q] = v;
    out[(size_t)q * d + p] = v;
  }
}

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------
// R of crystal b: one wave, lanes stride over the d coordinates of a mode, fp64 projections and sums.  The butterfly leaves the
// same six projections on every lane, so the classification of a mode is wave-uniform.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
elastic_relax_kernel(const float* __restrict__ evals, const float* __restrict__ modes, const int64_t* __restrict__ blk_ptr,
                     const int* __restrict__ cry_ptr, const float* __restrict__ lam, const float* __restrict__ thr, int n_cry,
                     float* __restrict__ relax, int* __restrict__ n_zero, int* __restrict__ n_negative, int* __restrict__ status) {
  const int b = blockIdx.x;
  if (b >= n_cry) return;
  const int lane = threadIdx.x;
  const int a0 = cry_ptr[b];
  const int d = 3 * (cry_ptr[b + 1] - a0);
  const float* ev = evals + 3 * (size_t)a0;
  const float* Q = modes + blk_ptr[b];
  const float* L = lam + 18 * (size_t)a0;     // [d][6]
  const float tz = thr[b];
  double r[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) r[k] = 0.0;
  int nz = 0, nn = 0;
  for (int m = 0; m < d; ++m) {
    const float lm = ev[m];
    double p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = lane; c < d; c += 64) {
      const double q = (double)Q[(size_t)m * d + c];
#pragma unroll
      for (int I = 0; I < 6; ++I) p[I] += q * (double)L[6 * (size_t)c + I];
    }
#pragma unroll
    for (int I = 0; I < 6; ++I) p[I] = wave_sum64(p[I]);
    if (!(fabsf(lm) > tz)) {   // a zero mode (or a NaN): left out and counted
      ++nz;
      continue;
    }
    if (lm < 0.f) ++nn;
    const double il = 1.0 / (double)lm;
    int k = 0;
#pragma unroll
    for (int I = 0; I < 6; ++I)
#pragma unroll
      for (int J = I; J < 6; ++J) r[k++] += p[I] * p[J] * il;
  }
  if (lane == 0) {
    float* o = relax + 36 * (size_t)b;
    int k = 0;
#pragma unroll
    for (int I = 0; I < 6; ++I)
#pragma unroll
      for (int J = I; J < 6; ++J) {
        const float v = (float)r[k++];
        o[6 * I + J] = v;
        o[6 * J + I] = v;
      }
    n_zero[b] = nz;
    n_negative[b] = nn;
    status[b] = (nz != 3 ? NNHIP_ELASTIC_STATUS_ZERO : 0) | (nn > 0 ? NNHIP_ELASTIC_STATUS_NEGATIVE : 0);
  }
}

}  // namespace

int launch_strain_tan_geom(const int64_t* edge_index, const int64_t* batch, const float* geo, const float* eta6, int n_edges,
                           float cutoff, float* tgeo, hipStream_t s) {
  if (n_edges <= 0) return NNHIP_OK;
  strain_tan_geom_kernel<<<cdiv(n_edges, 256), 256, 0, s>>>(edge_index, batch, geo, eta6, n_edges, 1.0f / cutoff, tgeo);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

int launch_strain_born(const float* dg_d, const float* geo, const int* row_ptr, const int* mol_ptr, int n_mol, float* d2,
                       hipStream_t s) {
  if (n_mol <= 0) return NNHIP_OK;
  strain_born_kernel<<<n_mol, 64, 0, s>>>(dg_d, geo, row_ptr, mol_ptr, n_mol, d2);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// ---- per-stage exports (include/newtonnet_hip.h, "Per-stage entry points"): nnhip_strain_vp keeps calling the launchers ----
extern "C" int nnhip_strain_tan_geom(const int64_t* edge_index, const int64_t* batch, const float* geo, const float* eta6,
                                     int32_t n_edges, float cutoff, float* tgeo, void* stream) {
  ARG_CHECK(n_edges >= 0 && cutoff > 0.f && (n_edges == 0 || (edge_index && batch && geo && eta6 && tgeo)), "nnhip_strain_tan_geom");
  if (n_edges == 0) return NNHIP_OK;
  return launch_strain_tan_geom(edge_index, batch, geo, eta6, n_edges, cutoff, tgeo, (hipStream_t)stream);
}

extern "C" int nnhip_strain_born(const float* dg_d, const float* geo, const int32_t* row_ptr, const int32_t* mol_ptr, int32_t n_mol,
                                 float* d2, void* stream) {
  ARG_CHECK(n_mol >= 0 && (n_mol == 0 || (dg_d && geo && row_ptr && mol_ptr && d2)), "nnhip_strain_born");
  if (n_mol == 0) return NNHIP_OK;
  return launch_strain_born(dg_d, geo, row_ptr, mol_ptr, n_mol, d2, (hipStream_t)stream);
}

extern "C" int nnhip_elastic_fold(const float* fc, const int64_t* fc_ptr, const int32_t* cry_ptr, const int32_t* sc_atoms,
                                  const int64_t* out_ptr, int32_t n_cry, float* phi0, int32_t* status, void* stream) {
  ARG_CHECK(n_cry >= 0 && (n_cry == 0 || (fc && fc_ptr && cry_ptr && sc_atoms && out_ptr && phi0 && status)), "nnhip_elastic_fold");
  if (n_cry == 0) return NNHIP_OK;
  elastic_fold_kernel<<<dim3(n_cry, 4), 256, 0, (hipStream_t)stream>>>(fc, fc_ptr, cry_ptr, sc_atoms, out_ptr, phi0, status);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

extern "C" int nnhip_elastic_relax(const float* evals, const float* modes, const int64_t* blk_ptr, const int32_t* cry_ptr,
                                   const float* lambda, const float* threshold, int32_t n_cry, float* relax, int32_t* n_zero,
                                   int32_t* n_negative, int32_t* status, void* stream) {
  ARG_CHECK(n_cry >= 0 && (n_cry == 0 || (evals && modes && blk_ptr && cry_ptr && lambda && threshold && relax && n_zero &&
                                          n_negative && status)),
            "nnhip_elastic_relax");
  if (n_cry == 0) return NNHIP_OK;
  elastic_relax_kernel<<<n_cry, 64, 0, (hipStream_t)stream>>>(evals, modes, blk_ptr, cry_ptr, lambda, threshold, n_cry, relax,
                                                               n_zero, n_negative, status);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
