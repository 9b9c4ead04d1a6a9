// Analytic Hessian-vector products (gfx950, fp32): the last stage of "tangent over reverse".
//
// The reference's HessianOutput (newtonnet/models/output.py:134-152) forms H = d^2E/dpos^2 = -d(gradient_force)/dpos with a
// torch.vmap of 3N double-backward calls.  The training sweeps 3-4 (csrc/train.hip, csrc/train_step.hip) already differentiate the
// value reverse sweep in forward mode along a position direction v; run with sign +1 and the reverse seed 1 + eps 0, every
// tangent they form is the tangent of the value adjoint along v.  dE/dpos itself is assembled by nnhip_edge_embed_bwd from two
// per-layer inputs that sweep 4 never differentiates:
//   g_x[l][e]    = sum_f g_eps[p][f] eps'_f(x_e)                         (the pair's owner edge, i < j; 0 for the other direction)
//   g_u[l][e][k] = < gf_l[i][k], phi1_l[p] >                             (every directed edge, i = its receiver row)
// H v is the tangent of pos_grad = dE/dpos along v, so this file adds the three missing tangents:
//   dg_u[l][e][k] = < dgf_l[i][k], phi1_l[p] > + < gf_l[i][k], dphi1_l[p] >             (hvp_dgu_kernel, inside the layer loop)
//   dg_x[l][e]    = sum_f dg_eps[p][f] eps'_f(x) + g_eps[p][f] eps''_f(x) dx_e          (hvp_dgx_kernel)
//                   with eps_f(x) = sum_n W_e[f][n] rbf_n(x), rbf = env(x) sin(w x)/x evaluated analytically in fp64 (the radial
//                   filter table's Hermite derivative plane is too coarse to difference once more)
//   dg_d[e]       = tangent of g_d[e] = (g_x/rc) u + (g_u - (g_u.u) u)/r along (du, dr)  (hvp_geom_kernel)
//   hv[i]         = sum_{e in row i} dg_d[e] - dg_d[rev e]                                 (hvp_rows_kernel: the force gather)
// Periodic shifts are constant under a position change, so nothing else enters.  No float atomics anywhere: every output is
// written by exactly one lane, every sum runs in a fixed order, so repeated calls are bitwise identical.
//
// The Hessian driver (nnhip_hessian_blocks, csrc/train_step.hip) feeds one-hot directions: pass k perturbs coordinate dir % 3 of
// local atom dir / 3 of every molecule at once (dir = k * n_rep + replica), and the column H e_dir of every molecule's block is
// scattered into the packed per-molecule blocks [n_b][3][n_b][3] (hess_dirs_kernel / hess_scatter_kernel).
#include "edge_common.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------
// dg_u of one layer: one wave per receiver row i (gf / dgf rows of i stay in registers), lane = features 2 lane, 2 lane + 1,
// one wave reduction per edge.  Every directed edge of the row is written by its own row (deterministic).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
hvp_dgu_kernel(const float* __restrict__ gf, const float* __restrict__ dgf, const float* __restrict__ phi1,
               const float* __restrict__ dphi1, const int* __restrict__ row_ptr, const int* __restrict__ pid,
               const int2* __restrict__ xg, int n_atoms, float* __restrict__ dg_u /*[E][4]*/) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_atoms) return;
  const int lane = threadIdx.x & 63;
  const int c = 2 * lane;
  float2 g[3], dg[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    g[k] = *reinterpret_cast<const float2*>(gf + ((size_t)i * 3 + k) * NF + c);
    dg[k] = *reinterpret_cast<const float2*>(dgf + ((size_t)i * 3 + k) * NF + c);
  }
  const int beg = row_ptr[i], end = row_ptr[i + 1];
  for (int e = beg; e < end; ++e) {
    const size_t p = (size_t)pid[e];
    const float2 v1 = *reinterpret_cast<const float2*>(phi1 + p * NF + c);
    const float2 w1 = *reinterpret_cast<const float2*>(dphi1 + p * NF + c);
    float t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      t[k] = wave_sum(fmaf(dg[k].x, v1.x, fmaf(dg[k].y, v1.y, fmaf(g[k].x, w1.x, g[k].y * w1.y))));
    const bool masked = xg && xg[e].x == FT_ZERO_ROW;   // a candidate outside the cutoff (reused list): contributes nothing
    if (lane == 0)
      reinterpret_cast<float4*>(dg_u)[e] = masked ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(t[0], t[1], t[2], 0.f);
  }
}

// ---------------------------------------------------------------------------------------------
// Bessel x envelope basis: first and second derivative in x (fp64).  The envelope: PolynomialCutoff(p)
// (representations.py:138-171) or CosineCutoff (:177-203), as graph.hip:envelope_eval.
//   rbf = env b,  b = sin(w x)/x:   b' = (w cos(w x) - b)/x,   b'' = -w^2 b - 2 b'/x
//   rbf' = env' b + env b',  rbf'' = env'' b + 2 env' b' + env b''
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void envelope_d012(double x, int env, double& e, double& de, double& dde) {
  if (env == NNHIP_ENVELOPE_COSINE) {
    const double pi = 3.14159265358979323846;
    double sn, cs;
    sincos(pi * x, &sn, &cs);
    e = 0.5 * (1.0 + cs);
    de = -0.5 * pi * sn;
    dde = -0.5 * pi * pi * cs;
  } else {
    //  1 - (p+1)(p+2)/2 x^p + p(p+2) x^(p+1) - p(p+1)/2 x^(p+2);  e' = -K x^(p-1) (1-x)^2;  e'' = -K x^(p-2) (1-x) ((p-1) - (p+1) x)
    const double p = (double)env, K = 0.5 * p * (p + 1.0) * (p + 2.0);
    const double xp = pow(x, p);
    e = 1.0 - 0.5 * (p + 1.0) * (p + 2.0) * xp + p * (p + 2.0) * xp * x - 0.5 * p * (p + 1.0) * xp * x * x;
    de = -K * pow(x, p - 1.0) * (1.0 - x) * (1.0 - x);
    dde = env >= 2 ? -K * pow(x, p - 2.0) * (1.0 - x) * ((p - 1.0) - (p + 1.0) * x) : 2.0 * K * (1.0 - x);
  }
}

// ---------------------------------------------------------------------------------------------
// dg_x of one layer: one wave per directed edge (grid-stride), W_e [F][nb] staged in LDS once per workgroup.  Lanes n < nb
// evaluate rbf'_n(x), rbf''_n(x) dx in fp64 and broadcast them by shuffles; every lane forms eps'_f, eps''_f dx of its two
// features from the LDS rows and
// the wave sums  dg_eps eps' + g_eps eps'' dx.  Only the pair's owner edge (i < j) carries it, as msg_bwd's g_x; the other
// direction and masked candidates get 0.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
hvp_dgx_kernel(const int64_t* __restrict__ edge_index, const int* __restrict__ pid, const float* __restrict__ geo,
               const float* __restrict__ tgeo, const int2* __restrict__ xg, const float* __restrict__ g_eps,
               const float* __restrict__ dg_eps, const float* __restrict__ edge_w, const float* __restrict__ freq, int nb, int env,
               float inv_rc, int n_edges, float* __restrict__ dg_x /*[E]*/) {
  __shared__ float W[NF * NNHIP_MAX_NB];
  for (int t = threadIdx.x; t < NF * nb; t += blockDim.x) W[t] = edge_w[t];
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = 2 * lane;
  for (int e = blockIdx.x * 4 + wv; e < n_edges; e += gridDim.x * 4) {
    const bool owner = edge_index[e] < edge_index[(size_t)n_edges + e];
    const bool masked = xg && xg[e].x == FT_ZERO_ROW;
    const double x = (double)reinterpret_cast<const float4*>(geo)[e].w * (double)inv_rc;
    if (!owner || masked || !(x < 1.0)) {   // (wave-uniform branch)
      if (lane == 0) dg_x[e] = 0.f;
      continue;
    }
    const float dx = tgeo[4 * (size_t)e + 3];
    float my1 = 0.f, my2 = 0.f;
    if (lane < nb) {
      double en, den, dden;
      envelope_d012(x, env, en, den, dden);
      const double w = (double)freq[lane];
      double sn, cs;
      sincos(w * x, &sn, &cs);
      const double b = sn / x;
      const double db = (w * cs - b) / x;
      const double ddb = -w * w * b - 2.0 * db / x;
      my1 = (float)(den * b + en * db);
      my2 = (float)((dden * b + 2.0 * den * db + en * ddb) * (double)dx);
    }
    float e1a = 0.f, e1b = 0.f, e2a = 0.f, e2b = 0.f;
    for (int n = 0; n < nb; ++n) {
      const float a1 = __shfl(my1, n, 64), a2 = __shfl(my2, n, 64);
      const float wa = W[c * nb + n], wb = W[(c + 1) * nb + n];
      e1a = fmaf(wa, a1, e1a);
      e1b = fmaf(wb, a1, e1b);
      e2a = fmaf(wa, a2, e2a);
      e2b = fmaf(wb, a2, e2b);
    }
    const size_t p = (size_t)pid[e];
    const float2 g = *reinterpret_cast<const float2*>(g_eps + p * NF + c);
    const float2 dg = *reinterpret_cast<const float2*>(dg_eps + p * NF + c);
    const float s = wave_sum(fmaf(dg.x, e1a, fmaf(dg.y, e1b, fmaf(g.x, e2a, g.y * e2b))));
    if (lane == 0) dg_x[e] = s;
  }
}

// ---------------------------------------------------------------------------------------------
// tangent of edge_gd_kernel (edge.hip) along tgeo = (du, dx = dr / rc), all layers summed:
//   a = g_x / rc - (g_u.u) / r,  g_d = a u + g_u / r
//   da = dg_x / rc - (dg_u.u + g_u.du) / r + (g_u.u) dr / r^2,   dg_d = da u + a du + dg_u / r - g_u dr / r^2
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
hvp_geom_kernel(const float* __restrict__ g_x, const float* __restrict__ g_u, const float* __restrict__ dg_x,
                const float* __restrict__ dg_u, const float* __restrict__ geo, const float* __restrict__ tgeo, int n_edges,
                int n_layers, float cutoff, float* __restrict__ dg_d /*[E][4]*/) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  float gx = 0.f, dgx = 0.f;
  float3 gu = make_float3(0.f, 0.f, 0.f), dgu = make_float3(0.f, 0.f, 0.f);
  for (int l = 0; l < n_layers; ++l) {
    const size_t le = (size_t)l * n_edges + e;
    gx += g_x[le];
    dgx += dg_x[le];
    const float4 a = reinterpret_cast<const float4*>(g_u)[le];
    const float4 b = reinterpret_cast<const float4*>(dg_u)[le];
    gu.x += a.x;
    gu.y += a.y;
    gu.z += a.z;
    dgu.x += b.x;
    dgu.y += b.y;
    dgu.z += b.z;
  }
  const float4 g = reinterpret_cast<const float4*>(geo)[e];
  const float4 t = reinterpret_cast<const float4*>(tgeo)[e];
  const float ir = 1.0f / g.w, inv_rc = 1.0f / cutoff;
  const float dr = t.w * cutoff;
  const float gdu = gu.x * g.x + gu.y * g.y + gu.z * g.z;
  const float a = gx * inv_rc - gdu * ir;
  const float da = dgx * inv_rc - (dgu.x * g.x + dgu.y * g.y + dgu.z * g.z + gu.x * t.x + gu.y * t.y + gu.z * t.z) * ir +
                   gdu * dr * ir * ir;
  const float q = dr * ir * ir;
  reinterpret_cast<float4*>(dg_d)[e] = make_float4(da * g.x + a * t.x + dgu.x * ir - gu.x * q, da * g.y + a * t.y + dgu.y * ir - gu.y * q,
                                                   da * g.z + a * t.z + dgu.z * ir - gu.z * q, 0.f);
}

// hv[i] = sum_{e in row i} dg_d[e] - dg_d[rev e]   (edge.hip:force_out_kernel without the force's minus sign)
__global__ void __launch_bounds__(256)
hvp_rows_kernel(const float* __restrict__ dg_d, const int* __restrict__ row_ptr, const int* __restrict__ rev, int n_atoms,
                float* __restrict__ hv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  float hx = 0.f, hy = 0.f, hz = 0.f;
  for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
    const float4 a = reinterpret_cast<const float4*>(dg_d)[e];
    const float4 b = reinterpret_cast<const float4*>(dg_d)[rev[e]];
    hx += a.x - b.x;
    hy += a.y - b.y;
    hz += a.z - b.z;
  }
  hv[3 * (size_t)i] = hx;
  hv[3 * (size_t)i + 1] = hy;
  hv[3 * (size_t)i + 2] = hz;
}

// direction of pass k for atom i of molecule b (replica r = b / n_mol0 of molecule b % n_mol0): dir = k n_rep + r; the atom
// gets e_(dir % 3) when it is local atom dir / 3 of its molecule, else 0
__device__ __forceinline__ int hess_dir(const int64_t* batch, const int* mol_ptr, int i, int k, int n_rep, int n_mol0, int& b,
                                        int& a, int& nb) {
  b = (int)batch[i];
  a = i - mol_ptr[b];
  nb = mol_ptr[b + 1] - mol_ptr[b];
  return k * n_rep + b / n_mol0;
}
__global__ void __launch_bounds__(256)
hess_dirs_kernel(const int64_t* __restrict__ batch, const int* __restrict__ mol_ptr, int n_atoms, int k, int n_rep, int n_mol0,
                 float* __restrict__ v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  int b, a, nb;
  const int dir = hess_dir(batch, mol_ptr, i, k, n_rep, n_mol0, b, a, nb);
  const bool on = dir < 3 * nb && a == dir / 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) v[3 * (size_t)i + c] = on && c == dir % 3 ? 1.f : 0.f;
}
// blocks[blk_ptr[b0] + (a 3 + c) 3 n_b + dir] = hv[i][c]: column dir of molecule b0's block
__global__ void __launch_bounds__(256)
hess_scatter_kernel(const float* __restrict__ hv, const int64_t* __restrict__ batch, const int* __restrict__ mol_ptr,
                    const int64_t* __restrict__ blk_ptr, int n_atoms, int k, int n_rep, int n_mol0, float* __restrict__ blocks) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_atoms) return;
  int b, a, nb;
  const int dir = hess_dir(batch, mol_ptr, i, k, n_rep, n_mol0, b, a, nb);
  if (dir >= 3 * nb) return;
  float* blk = blocks + blk_ptr[b % n_mol0];
#pragma unroll
  for (int c = 0; c < 3; ++c) blk[(size_t)(3 * a + c) * (3 * nb) + dir] = hv[3 * (size_t)i + c];
}

}  // namespace

int launch_hvp_dgu(const float* gf, const float* dgf, const float* phi1, const float* dphi1, const int* row_ptr, const int* pid,
                   const int* xg, int n_atoms, float* dg_u, hipStream_t s) {
  if (n_atoms <= 0) return NNHIP_OK;
  hvp_dgu_kernel<<<cdiv(n_atoms, 4), 256, 0, s>>>(gf, dgf, phi1, dphi1, row_ptr, pid, reinterpret_cast<const int2*>(xg), n_atoms,
                                                   dg_u);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

int launch_hvp_dgx(const int64_t* edge_index, const int* pid, const float* geo, const float* tgeo, const int* xg, const float* g_eps,
                   const float* dg_eps, const float* edge_w, const float* freq, int nb, int env, float cutoff, int n_edges,
                   float* dg_x, hipStream_t s) {
  if (n_edges <= 0) return NNHIP_OK;
  if (nb < 1 || nb > NNHIP_MAX_NB) {
    nnhip_set_error("hessian: n_basis %d outside 1..%d", nb, NNHIP_MAX_NB);
    return NNHIP_E_UNSUPPORTED;
  }
  const int grid = cdiv(n_edges, 4) < 2048 ? cdiv(n_edges, 4) : 2048;
  hvp_dgx_kernel<<<grid, 256, 0, s>>>(edge_index, pid, geo, tgeo, reinterpret_cast<const int2*>(xg), g_eps, dg_eps, edge_w, freq, nb,
                                      env ? env : 9, 1.0f / cutoff, n_edges, dg_x);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

int launch_hvp_out(const float* g_x, const float* g_u, const float* dg_x, const float* dg_u, const float* geo, const float* tgeo,
                   const int* row_ptr, const int* rev, int n_atoms, int n_edges, int n_layers, float cutoff, float* dg_d, float* hv,
                   hipStream_t s) {
  if (n_edges > 0) {
    hvp_geom_kernel<<<cdiv(n_edges, 256), 256, 0, s>>>(g_x, g_u, dg_x, dg_u, geo, tgeo, n_edges, n_layers, cutoff, dg_d);
    LAUNCH_CHECK();
  }
  if (n_atoms > 0) {
    hvp_rows_kernel<<<cdiv(n_atoms, 256), 256, 0, s>>>(dg_d, row_ptr, rev, n_atoms, hv);
    LAUNCH_CHECK();
  }
  return NNHIP_OK;
}

int launch_hess_dirs(const int64_t* batch, const int* mol_ptr, int n_atoms, int k, int n_rep, int n_mol0, float* v, hipStream_t s) {
  if (n_atoms <= 0) return NNHIP_OK;
  hess_dirs_kernel<<<cdiv(n_atoms, 256), 256, 0, s>>>(batch, mol_ptr, n_atoms, k, n_rep, n_mol0, v);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

int launch_hess_scatter(const float* hv, const int64_t* batch, const int* mol_ptr, const int64_t* blk_ptr, int n_atoms, int k,
                        int n_rep, int n_mol0, float* blocks, hipStream_t s) {
  if (n_atoms <= 0) return NNHIP_OK;
  hess_scatter_kernel<<<cdiv(n_atoms, 256), 256, 0, s>>>(hv, batch, mol_ptr, blk_ptr, n_atoms, k, n_rep, n_mol0, blocks);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

// ---- per-stage exports (include/newtonnet_hip.h, "Per-stage entry points"): thin wrappers over the launchers above; the drivers in
// csrc/train_step.hip keep calling the launchers ----
extern "C" int nnhip_hvp_dgu(const float* gf, const float* dgf, const float* phi1, const float* dphi1, const int32_t* row_ptr,
                             const int32_t* pid, const int32_t* xg, int32_t n_atoms, float* dg_u, void* stream) {
  ARG_CHECK(n_atoms >= 0 && (n_atoms == 0 || (gf && dgf && phi1 && dphi1 && row_ptr && pid && dg_u)), "nnhip_hvp_dgu");
  if (n_atoms == 0) return NNHIP_OK;
  return launch_hvp_dgu(gf, dgf, phi1, dphi1, row_ptr, pid, xg, n_atoms, dg_u, (hipStream_t)stream);
}

extern "C" int nnhip_hvp_dgx(const int64_t* edge_index, const int32_t* pid, const float* geo, const float* tgeo, const int32_t* xg,
                             const float* g_eps, const float* dg_eps, const float* edge_w, const float* freq, int32_t n_basis,
                             int32_t envelope, float cutoff, int32_t n_edges, float* dg_x, void* stream) {
  ARG_CHECK(n_edges >= 0 && cutoff > 0.f && envelope >= NNHIP_ENVELOPE_COSINE &&
                (n_edges == 0 || (edge_index && pid && geo && tgeo && g_eps && dg_eps && edge_w && freq && dg_x)),
            "nnhip_hvp_dgx");
  if (n_basis < 1 || n_basis > NNHIP_MAX_NB) {
    nnhip_set_error("nnhip_hvp_dgx: n_basis %d outside 1..%d", n_basis, NNHIP_MAX_NB);
    return NNHIP_E_UNSUPPORTED;
  }
  if (n_edges == 0) return NNHIP_OK;
  return launch_hvp_dgx(edge_index, pid, geo, tgeo, xg, g_eps, dg_eps, edge_w, freq, n_basis, envelope, cutoff, n_edges, dg_x,
                        (hipStream_t)stream);
}

extern "C" int nnhip_hvp_out(const float* g_x, const float* g_u, const float* dg_x, const float* dg_u, const float* geo,
                             const float* tgeo, const int32_t* row_ptr, const int32_t* rev, int32_t n_atoms, int32_t n_edges,
                             int32_t n_layers, float cutoff, float* dg_d, float* hv, void* stream) {
  ARG_CHECK(n_atoms >= 0 && n_edges >= 0 && (n_edges == 0 || n_atoms > 0) && n_layers >= 1 && n_layers <= NNHIP_MAX_LAYERS &&
                cutoff > 0.f && (n_edges == 0 || (g_x && g_u && dg_x && dg_u && geo && tgeo && rev && dg_d)) &&
                (n_atoms == 0 || (row_ptr && hv)),
            "nnhip_hvp_out");
  if (n_atoms == 0) return NNHIP_OK;
  return launch_hvp_out(g_x, g_u, dg_x, dg_u, geo, tgeo, row_ptr, rev, n_atoms, n_edges, n_layers, cutoff, dg_d, hv,
                        (hipStream_t)stream);
}

extern "C" int nnhip_hess_dirs(const int64_t* batch, const int32_t* mol_ptr, int32_t n_atoms, int32_t k, int32_t n_rep,
                               int32_t n_mol0, float* v, void* stream) {
  ARG_CHECK(n_atoms >= 0 && k >= 0 && n_rep >= 1 && n_mol0 >= 1 && (n_atoms == 0 || (batch && mol_ptr && v)), "nnhip_hess_dirs");
  if (n_atoms == 0) return NNHIP_OK;
  return launch_hess_dirs(batch, mol_ptr, n_atoms, k, n_rep, n_mol0, v, (hipStream_t)stream);
}

extern "C" int nnhip_hess_scatter(const float* hv, const int64_t* batch, const int32_t* mol_ptr, const int64_t* blk_ptr,
                                  int32_t n_atoms, int32_t k, int32_t n_rep, int32_t n_mol0, float* blocks, void* stream) {
  ARG_CHECK(n_atoms >= 0 && k >= 0 && n_rep >= 1 && n_mol0 >= 1 && (n_atoms == 0 || (hv && batch && mol_ptr && blk_ptr && blocks)),
            "nnhip_hess_scatter");
  if (n_atoms == 0) return NNHIP_OK;
  return launch_hess_scatter(hv, batch, mol_ptr, blk_ptr, n_atoms, k, n_rep, n_mol0, blocks, (hipStream_t)stream);
}
