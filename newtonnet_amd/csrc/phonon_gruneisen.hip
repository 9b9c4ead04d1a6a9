// Strain slopes of phonon eigenvalues (gfx950, fp32): d lambda / d eta_k = e^H (dD / d eta_k) e of every mode of every (crystal, wave
// vector) problem and every strain plane k in ONE launch, and the mode Grueneisen parameters gamma_k = -dlam_k / (2 lambda), from
// n_planes planes of force-constant derivatives dPhi / d eta_k (each laid out as the force constants are), the image table and the
// eigenpairs nnhip_phonon_bands / nnhip_phonon_bands_large left in HBM.
//
// D is linear in the force constants, so dD_k(q) is D's own sum applied to plane k,
//     dD_k,ij = (m_i m_j)^-1/2 sum_J dPhi_k(i, J) (1 / m_iJ) sum_T exp(2 pi i q . x_T),   dD_k <- (dD_k + dD_k^H) / 2
// (ph_weight, ph_accumulate, ph_hermitian and ph_rsm of csrc/phonon_common.h: the phase in fp64, the copies R ascending, fmaf): the
// force constants themselves handed in as a plane give D(q) element for element as the solvers assemble it.  Modes are grouped by
// eigenvalue exactly as csrc/phonon_velocity.hip groups them (consecutive sorted eigenvalues no more than deg_tol apart, cap PG_GROUP).
// A group of one takes Re e^H dD_k e.  A group of g > 1 forms M_s = V^H dD_split V and M_k = V^H dD_k V, diagonalises M_s with
// ph_jacobi in LDS (eigenvalues ascending, ties by index), and its modes, in that order, take Re diag(U^H M_k U) -- degenerate
// perturbation theory along the split plane.
//
// One workgroup of PH_THREADS per (crystal, q, tile of modes, plane k): grid (n_q, tiles * n_planes, n_cry), blockIdx.y = tile *
// n_planes + k.  A workgroup streams at most TWO planes through LDS, the split plane (slot 0) and its own (slot 1), in the block scheme
// of the velocity kernel (PG_AI x PG_AJ atoms, the weights of PG_RCHUNK copies staged at a time); one plane where the two pointers are
// equal.  So the LDS stays below the velocity kernel's three planes at every d, plane k's result does not depend on n_planes, and the
// split plane's rotation, recomputed per plane by the same arithmetic, is the same bits in every workgroup.  Tiling as there: one tile of
// all modes up to d = PG_TILE_ONE, tiles of PG_TILE modes above, a group belongs to the tile of its first mode, a tile looks PG_GROUP - 1
// modes past its end.  No workspace, no float atomics; every sum has an order that belongs to its element; one writer per output
// (group, defined: plane 0; status: tile 0 of plane 0).
//
// The grouping and the rotate-and-rank tail restate those of phonon_velocity.hip, which is left exactly as it is.
#include "phonon_common.h"

#define PG_TILE_ONE 96    // d up to which one tile holds every mode
#define PG_TILE 64        // modes per tile above
#define PG_GROUP 16       // largest degenerate group served (phonons.MAX_DEGENERATE)
#define PG_AI 4           // atoms per block row of dD
#define PG_AJ 8           // atoms per block column
#define PG_RCHUNK 8       // supercell copies whose weights are staged at a time
#define PG_ROWS (3 * PG_AI)
#define PG_COLS (3 * PG_AJ)
#define PG_ELD (PG_COLS + 1)   // row stride of the staged modes (float2)
#define PG_JP (PG_GROUP + 1)   // row stride of the group's matrices
#define PG_SLOTS 2             // planes a workgroup streams at most: the split plane and its own
#define PG_MAX_PLANES 6

namespace {

struct PgArgs {
  const float* dfc;
  const float* dfc_split;
  int64_t plane_stride;
  const int64_t* fc_ptr;
  const int* cry_ptr;
  const int* sc_atoms;
  const int64_t* img_ptr;
  const int* img_start;
  const double* img_off;
  const float* masses;
  const int64_t* out_ptr;
  const double* q;
  const float* evals;
  const float* modes;
  const float* deg_tol;
  const float* zero_tol;
  float* dlam;
  float* gamma;
  int* group;
  uint8_t* defined;
  int* status;
  int n_q, n_planes, d_cap, te_cap;
};

__host__ __device__ inline int pg_gcap(int te_cap) { return te_cap < PG_GROUP ? te_cap : PG_GROUP; }

// bytes of LDS of a workgroup that serves up to d_cap coordinates with up to te_cap modes in view (the layout of pg_kernel)
__host__ __device__ inline size_t pg_lds_bytes(int d_cap, int te_cap) {
  const size_t f64 = (size_t)((d_cap / 3 + 2) & ~1) + 2 * PG_GROUP;   // (even: the float4 behind it stays aligned)
  const size_t f2 = 2 * (size_t)PG_SLOTS * PG_ROWS * PG_COLS + 2 * (size_t)PG_RCHUNK * PG_AI * PG_AJ + (size_t)te_cap * PG_ELD +
                    (size_t)PG_SLOTS * PG_ROWS * te_cap + (size_t)PG_SLOTS * te_cap * pg_gcap(te_cap);
  const size_t f32 = (size_t)d_cap + 4 * (size_t)PG_GROUP * PG_JP + 2 * PG_GROUP;
  const size_t i32 = 2 * (size_t)d_cap + PG_GROUP + 4;
  return 8 * f64 + 16 * (PG_GROUP / 2) + 8 * f2 + 4 * f32 + 4 * i32 + 2 * 64;
}

// the outputs of mode `idx` (its index over the whole call) for plane kp: dl = d lambda / d eta_k, zero for a capped group
__device__ __forceinline__ void pg_write(const PgArgs& g, size_t idx, int kp, int first, float lam, float ztol, float dl, bool capped) {
  const bool live = !capped && fabsf(lam) > ztol;
  if (capped) dl = 0.f;
  g.dlam[idx * g.n_planes + kp] = dl;
  g.gamma[idx * g.n_planes + kp] = live ? -dl / (2.f * lam) : 0.f;
  if (kp == 0) {
    if (g.group) g.group[idx] = first;
    g.defined[idx] = live ? 1 : 0;
  }
}

__global__ void __launch_bounds__(PH_THREADS)
pg_kernel(PgArgs g) {
  extern __shared__ __align__(16) char pg_smem[];
  const int t = threadIdx.x;
  const int qi = blockIdx.x, b = blockIdx.z;
  const int tile = blockIdx.y / g.n_planes, kp = blockIdx.y - tile * g.n_planes;
  const bool writer = tile == 0 && kp == 0;   // of the problem's status
  const int a0 = g.cry_ptr[b];
  const int n = g.cry_ptr[b + 1] - a0;
  if (n <= 0) return;   // (uniform)
  const int d = 3 * n;
  const int TM = d <= PG_TILE_ONE ? d : PG_TILE;
  const int t0 = tile * TM;
  if (t0 >= d) return;
  const size_t prob = (size_t)b * g.n_q + qi;
  if (d > g.d_cap) {   // cry_ptr and cry_ptr_host disagree: this launch's LDS and grid are too small for the crystal
    if (t == 0 && writer) g.status[prob] = NNHIP_EIG_STATUS_SIZE;
    return;
  }
  int bad_mass = 0;
  for (int i = 0; i < n; ++i) {
    const float m = g.masses ? g.masses[a0 + i] : 1.f;
    bad_mass |= !(m > 0.f && m <= 3.4e38f);
  }
  if (bad_mass) {   // (uniform: every thread looked at every mass)
    if (t == 0 && writer) g.status[prob] = NNHIP_EIG_STATUS_MASS;
    return;
  }
  const int t1 = t0 + TM < d ? t0 + TM : d;                                       // the tile's own modes: t0 .. t1 - 1
  const int te = (t1 + PG_GROUP - 1 < d ? t1 + PG_GROUP - 1 : d) - t0;            // the modes in view
  const int d_cap = g.d_cap, te_cap = g.te_cap, gcap = pg_gcap(g.te_cap);
  if (te > te_cap) {   // (cry_ptr and cry_ptr_host disagree within d_cap: the tile sees more modes than the LDS was sized for)
    if (t == 0 && writer) g.status[prob] = NNHIP_EIG_STATUS_SIZE;
    return;
  }

  double* rsm = reinterpret_cast<double*>(pg_smem);                // [d_cap / 3, rounded up to even] 1 / sqrt(m_i)
  double* rowo = rsm + ((d_cap / 3 + 2) & ~1);                     // [PG_GROUP] scratch of ph_jacobi ...
  double* rowd = rowo + PG_GROUP;
  float4* cst = reinterpret_cast<float4*>(rowd + PG_GROUP);        // [PG_GROUP / 2]
  float2* Gd = reinterpret_cast<float2*>(cst + PG_GROUP / 2);      // [PG_SLOTS][PG_ROWS][PG_COLS] sums of the block, then dD itself
  float2* Gt = Gd + PG_SLOTS * PG_ROWS * PG_COLS;                  // ... of the transposed block
  float2* wd = Gt + PG_SLOTS * PG_ROWS * PG_COLS;                  // [PG_RCHUNK][ai][aj] weights of the block's pairs
  float2* wt = wd + PG_RCHUNK * PG_AI * PG_AJ;                     // [PG_RCHUNK][aj][ai] ... of the transposed pairs
  float2* E = wt + PG_RCHUNK * PG_AI * PG_AJ;                      // [te_cap][PG_ELD] the modes in view at the block's columns
  float2* Y = E + (size_t)te_cap * PG_ELD;                         // [PG_SLOTS][te_cap][PG_ROWS]
  float2* Mg = Y + (size_t)PG_SLOTS * PG_ROWS * te_cap;            // [PG_SLOTS][te_cap][gcap]: M[s][t] at [slot][t][s - first(t)]
  float* lam = reinterpret_cast<float*>(Mg + (size_t)PG_SLOTS * te_cap * gcap);   // [d_cap]
  float* Are = lam + d_cap;                                        // [PG_GROUP][PG_JP] x 4: the group's M_s and its vectors
  float* Aim = Are + PG_GROUP * PG_JP;
  float* Wre = Aim + PG_GROUP * PG_JP;
  float* Wim = Wre + PG_GROUP * PG_JP;
  float* dlt = Wim + PG_GROUP * PG_JP;                             // [PG_GROUP]
  float* dg = dlt + PG_GROUP;                                      // [PG_GROUP]
  int* gs = reinterpret_cast<int*>(dg + PG_GROUP);                 // [d_cap] first mode of the mode's group
  int* ge = gs + d_cap;                                            // [d_cap] one past its last
  int* rank = ge + d_cap;                                          // [PG_GROUP]
  int* flag = rank + PG_GROUP;                                     // [4]
  unsigned short* tab = reinterpret_cast<unsigned short*>(flag + 4);   // [<= 36]

  const float* evals = g.evals + (size_t)g.n_q * 3 * a0 + (size_t)qi * d;
  const float2* modes = reinterpret_cast<const float2*>(g.modes) + (size_t)g.n_q * g.out_ptr[b] + (size_t)qi * d * d;
  const size_t out0 = (size_t)g.n_q * 3 * a0 + (size_t)qi * d;

  // ---- the eigenpairs are finite, or nothing is computed ---------------------------------------------------------------------
  if (t < 4) flag[t] = 0;
  __syncthreads();
  int bad = 0;
  for (int i = t; i < d; i += PH_THREADS) {
    const float v = evals[i];
    lam[i] = v;
    bad |= !(fabsf(v) <= 3.4e38f);
  }
  for (int e = t; e < d * d; e += PH_THREADS) {
    const float2 v = modes[e];
    bad |= !(fabsf(v.x) <= 3.4e38f && fabsf(v.y) <= 3.4e38f);
  }
  if (bad) flag[0] = 1;
  for (int i = t; i < n; i += PH_THREADS) rsm[i] = ph_rsm(g.masses, a0 + i);
  __syncthreads();
  if (flag[0]) {   // (uniform)
    if (kp == 0)
      for (int k = t0 + t; k < t1; k += PH_THREADS) g.defined[out0 + k] = 0;
    if (t == 0 && writer) g.status[prob] = NNHIP_PHONON_STATUS_NONFINITE;
    return;
  }

  // ---- groups ----------------------------------------------------------------------------------------------------------------
  const float dtol = g.deg_tol[b], ztol = g.zero_tol[b];
  for (int k = t; k < d; k += PH_THREADS) {
    int s = k, e = k + 1;
    while (s > 0 && lam[s] - lam[s - 1] <= dtol) --s;
    while (e < d && lam[e] - lam[e - 1] <= dtol) ++e;
    gs[k] = s;
    ge[k] = e;
    if (e - s > PG_GROUP) flag[1] = 1;
  }
  for (int e = t; e < PG_SLOTS * te_cap * gcap; e += PH_THREADS) Mg[e] = make_float2(0.f, 0.f);
  __syncthreads();
  if (t == 0 && writer) g.status[prob] = flag[1] ? NNHIP_PHONON_STATUS_GROUP : 0;

  // ---- the planes of this workgroup: slot 0 the split plane, slot own its own (the same slot where the pointers are equal) ------
  const float* plane_own = g.dfc + (size_t)kp * g.plane_stride + g.fc_ptr[b];
  const float* plane[PG_SLOTS];
  plane[0] = g.dfc_split + g.fc_ptr[b];
  plane[1] = plane_own;
  const int np = plane[0] == plane[1] ? 1 : 2;
  const int own = np - 1;
  const double q0 = g.q[3 * (size_t)qi], q1 = g.q[3 * (size_t)qi + 1], q2 = g.q[3 * (size_t)qi + 2];

  // ---- M = V^H dD V of the tile's groups, dD streamed block by block ---------------------------------------------------------------
  const int N = g.sc_atoms[b];
  const int nR = N / n;
  const int* ist = g.img_start + g.img_ptr[b];
  for (int I0 = 0; I0 < n; I0 += PG_AI) {
    const int ai = n - I0 < PG_AI ? n - I0 : PG_AI;
    const int rows = 3 * ai;
    for (int J0 = 0; J0 < n; J0 += PG_AJ) {
      const int aj = n - J0 < PG_AJ ? n - J0 : PG_AJ;
      const int cols = 3 * aj;
      __syncthreads();   // the block before this one has been used (E, G) and, at J0 = 0, the block row before it (Y)
      for (int e = t; e < te * cols; e += PH_THREADS) {
        const int tt = e / cols, jc = e - tt * cols;
        E[tt * PG_ELD + jc] = modes[(size_t)(t0 + tt) * d + 3 * J0 + jc];
      }
      const int wr = ai * aj;   // weights per copy
      for (int R0 = 0; R0 < nR; R0 += PG_RCHUNK) {
        const int rc = nR - R0 < PG_RCHUNK ? nR - R0 : PG_RCHUNK;
        if (R0 > 0) __syncthreads();   // the chunk before this one has been summed
        for (int x = t; x < rc * ai * aj; x += PH_THREADS) {
          const int r = x / (ai * aj), rem = x - r * ai * aj;
          const int ii = rem / aj, jj = rem - ii * aj;
          wd[x] = ph_weight(ist, g.img_off, (size_t)(I0 + ii) * N + (size_t)(R0 + r) * n + (J0 + jj), q0, q1, q2);
          wt[(r * aj + jj) * ai + ii] = ph_weight(ist, g.img_off, (size_t)(J0 + jj) * N + (size_t)(R0 + r) * n + (I0 + ii), q0, q1, q2);
        }
        __syncthreads();
        for (int e = t; e < rows * cols; e += PH_THREADS) {
          const int ir = e / cols, jc = e - ir * cols;
          const int ii = ir / 3, al = ir - 3 * ii, jj = jc / 3, be = jc - 3 * jj;
          const size_t od = ((size_t)(3 * I0 + ir) * N + (size_t)R0 * n + (J0 + jj)) * 3 + be;
          const size_t ot = ((size_t)(3 * J0 + jc) * N + (size_t)R0 * n + (I0 + ii)) * 3 + al;
          for (int p = 0; p < np; ++p) {
            const int ge_ = p * PG_ROWS * PG_COLS + ir * PG_COLS + jc;
            float2 sd = R0 ? Gd[ge_] : make_float2(0.f, 0.f), st = R0 ? Gt[ge_] : make_float2(0.f, 0.f);
            ph_accumulate(plane[p] + od, n, wd + (ii * aj + jj), wr, rc, sd.x, sd.y);
            ph_accumulate(plane[p] + ot, n, wt + (jj * ai + ii), wr, rc, st.x, st.y);
            Gd[ge_] = sd;
            Gt[ge_] = st;
          }
        }
      }
      for (int e = t; e < rows * cols; e += PH_THREADS) {   // (the thread that summed element e)
        const int ir = e / cols, jc = e - ir * cols;
        const float f = (float)(rsm[I0 + ir / 3] * rsm[J0 + jc / 3]);
        for (int p = 0; p < np; ++p) {
          const int ge_ = p * PG_ROWS * PG_COLS + ir * PG_COLS + jc;
          if (nR == 0) Gd[ge_] = Gt[ge_] = make_float2(0.f, 0.f);
          const float2 sd = Gd[ge_], st = Gt[ge_];
          float re, im;
          ph_hermitian(sd.x, sd.y, st.x, st.y, f, 3 * I0 + ir == 3 * J0 + jc, re, im);
          Gd[ge_] = make_float2(re, im);
        }
      }
      __syncthreads();
      for (int x = t; x < rows * te; x += PH_THREADS) {
        const int tt = x / rows, ir = x - tt * rows;
        const int k = t0 + tt, s = gs[k];
        if (s < t0 || s >= t1 || ge[k] - s > PG_GROUP) continue;   // the group is another tile's, or above the cap
        for (int p = 0; p < np; ++p) {
          const int yi = (p * te_cap + tt) * PG_ROWS + ir;
          float2 acc = J0 ? Y[yi] : make_float2(0.f, 0.f);
          const float2* gr = Gd + p * PG_ROWS * PG_COLS + ir * PG_COLS;
          for (int jc = 0; jc < cols; ++jc) {
            const float2 gv = gr[jc], ev = E[tt * PG_ELD + jc];
            acc.x = fmaf(gv.x, ev.x, fmaf(-gv.y, ev.y, acc.x));
            acc.y = fmaf(gv.x, ev.y, fmaf(gv.y, ev.x, acc.y));
          }
          Y[yi] = acc;
        }
      }
    }
    __syncthreads();
    for (int x = t; x < te * gcap; x += PH_THREADS) {
      const int tt = x / gcap, so = x - tt * gcap;
      const int k = t0 + tt, s0 = gs[k];
      if (s0 < t0 || s0 >= t1 || ge[k] - s0 > PG_GROUP || so >= ge[k] - s0) continue;
      const float2* es = modes + (size_t)(s0 + so) * d + 3 * I0;
      for (int p = 0; p < np; ++p) {
        float2 acc = Mg[(size_t)p * te_cap * gcap + x];
        const float2* y = Y + (p * te_cap + tt) * PG_ROWS;
        for (int ir = 0; ir < rows; ++ir) {
          const float2 ev = es[ir], yv = y[ir];
          acc.x = fmaf(ev.x, yv.x, fmaf(ev.y, yv.y, acc.x));
          acc.y = fmaf(ev.x, yv.y, fmaf(-ev.y, yv.x, acc.y));
        }
        Mg[(size_t)p * te_cap * gcap + x] = acc;
      }
    }
  }
  __syncthreads();

  // ---- groups of one, and groups above the cap ---------------------------------------------------------------------------------
  const size_t mstride = (size_t)te_cap * gcap;
  for (int k = t0 + t; k < d; k += PH_THREADS) {
    const int s = gs[k], sz = ge[k] - s;
    if (s < t0 || s >= t1) continue;
    if (sz > PG_GROUP) {
      pg_write(g, out0 + k, kp, s, lam[k], ztol, 0.f, true);
    } else if (sz == 1) {
      pg_write(g, out0 + k, kp, s, lam[k], ztol, Mg[own * mstride + (size_t)(k - t0) * gcap].x, false);
    }
  }

  // ---- degenerate groups: diagonalise M_s, rotate M_k ------------------------------------------------------------------------------
  for (int k0 = t0; k0 < t1; ++k0) {
    const int sz = ge[k0] - k0;
    if (gs[k0] != k0 || sz < 2 || sz > PG_GROUP) continue;   // (uniform)
    const int tt0 = k0 - t0;
    const int Mp = (sz + 1) & ~1, P = Mp >> 1;
    __syncthreads();   // the group before this one is done with the matrices
    for (int e = t; e < Mp * PG_JP; e += PH_THREADS) {
      Are[e] = 0.f;
      Aim[e] = 0.f;
    }
    for (int e = t; e < P * P; e += PH_THREADS) {
      const int k = e / P, l = e - k * P;
      if (k <= l) tab[k * P - k * (k - 1) / 2 + (l - k)] = (unsigned short)(k | l << 8);
    }
    __syncthreads();
    for (int e = t; e < sz * sz; e += PH_THREADS) {
      const int s = e / sz, c = e - s * sz;
      if (s > c) continue;   // the thread of (s, c), s <= c, writes both halves
      const float2 m = Mg[(size_t)(tt0 + c) * gcap + s];   // slot 0: the split plane
      const float re = m.x;
      const float im = s == c ? 0.f : m.y;
      Are[s * PG_JP + c] = re;
      Are[c * PG_JP + s] = re;
      Aim[s * PG_JP + c] = im;
      Aim[c * PG_JP + s] = -im;
    }
    __syncthreads();
    bool converged;
    ph_jacobi<false>(Are, Aim, Wre, Wim, Mp, PG_JP, rowo, rowd, cst, dlt, tab, true, EIG_EPS2, EIG_MAX_SWEEPS, t, converged);
    __syncthreads();
    if (t < sz) dg[t] = Are[t * PG_JP + t];
    __syncthreads();
    if (t < sz) {
      const float di = dg[t];
      int r = 0;
      for (int j = 0; j < sz; ++j) {
        const float dj = dg[j];
        r += dj < di || (dj == di && j < t) ? 1 : 0;
      }
      // Re u^H M_k u with u = row t of W, s then c ascending
      float acc = 0.f;
      for (int s = 0; s < sz; ++s) {
        const float usr = Wre[t * PG_JP + s], usi = Wim[t * PG_JP + s];
        float zr = 0.f, zi = 0.f;   // sum_c M_k[s][c] u[c]
        for (int c = 0; c < sz; ++c) {
          const float2 m = Mg[own * mstride + (size_t)(tt0 + c) * gcap + s];
          const float ucr = Wre[t * PG_JP + c], uci = Wim[t * PG_JP + c];
          zr = fmaf(m.x, ucr, fmaf(-m.y, uci, zr));
          zi = fmaf(m.x, uci, fmaf(m.y, ucr, zi));
        }
        acc = fmaf(usr, zr, fmaf(usi, zi, acc));
      }
      const int k = k0 + r;
      pg_write(g, out0 + k, kp, k0, lam[k], ztol, acc, false);
    }
  }
}

}  // namespace

extern "C" int nnhip_phonon_strain_slopes(const float* dfc, int32_t n_planes, int64_t plane_stride, const float* dfc_split,
                                          const int64_t* fc_ptr, const int32_t* cry_ptr, const int32_t* cry_ptr_host,
                                          const int32_t* sc_atoms, const int64_t* img_ptr, const int32_t* img_start,
                                          const double* img_off, const float* masses, const int64_t* out_ptr, int32_t n_cry,
                                          const double* q, int32_t n_q, const float* evals, const float* modes, const float* deg_tol,
                                          const float* zero_tol, float* dlam, float* gamma, int32_t* group, uint8_t* defined,
                                          int32_t* status, void* stream) {
  if (n_cry < 0 || n_q < 0 || plane_stride < 0 ||
      (n_cry > 0 && n_q > 0 && (!dfc || !dfc_split || !fc_ptr || !cry_ptr || !cry_ptr_host || !sc_atoms || !img_ptr || !img_start ||
                                !img_off || !out_ptr || !q || !evals || !modes || !deg_tol || !zero_tol || !dlam || !gamma ||
                                !defined || !status))) {
    nnhip_set_error("nnhip_phonon_strain_slopes: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_planes < 1 || n_planes > PG_MAX_PLANES) {
    nnhip_set_error("nnhip_phonon_strain_slopes: n_planes = %d, outside 1 .. %d", n_planes, PG_MAX_PLANES);
    return NNHIP_E_INVALID;
  }
  if (n_cry > 65535) {
    nnhip_set_error("nnhip_phonon_strain_slopes: %d crystals in one call, above the 65535 a launch addresses", n_cry);
    return NNHIP_E_UNSUPPORTED;
  }
  const int bound = nnhip_phonon_large_max_dim();
  int d_cap = 0, te_cap = 0;
  for (int b = 0; b < n_cry; ++b) {
    const int m = 3 * (cry_ptr_host[b + 1] - cry_ptr_host[b]);
    if (m < 0) {
      nnhip_set_error("nnhip_phonon_strain_slopes: cry_ptr_host decreases at crystal %d", b);
      return NNHIP_E_INVALID;
    }
    if (m > bound) {
      nnhip_set_error("nnhip_phonon_strain_slopes: crystal %d has dimension 3 x %d = %d, above the supported %d "
                      "(nnhip_phonon_large_max_dim)", b, m / 3, m, bound);
      return NNHIP_E_UNSUPPORTED;
    }
    d_cap = m > d_cap ? m : d_cap;
    const int te = m <= PG_TILE_ONE ? m : PG_TILE + PG_GROUP - 1;   // the modes a tile of this crystal has in view
    te_cap = te > te_cap ? te : te_cap;
  }
  if (d_cap == 0 || n_q == 0) return NNHIP_OK;
  PgArgs g;
  g.dfc = dfc;
  g.dfc_split = dfc_split;
  g.plane_stride = plane_stride;
  g.fc_ptr = fc_ptr;
  g.cry_ptr = cry_ptr;
  g.sc_atoms = sc_atoms;
  g.img_ptr = img_ptr;
  g.img_start = img_start;
  g.img_off = img_off;
  g.masses = masses;
  g.out_ptr = out_ptr;
  g.q = q;
  g.evals = evals;
  g.modes = modes;
  g.deg_tol = deg_tol;
  g.zero_tol = zero_tol;
  g.dlam = dlam;
  g.gamma = gamma;
  g.group = group;
  g.defined = defined;
  g.status = status;
  g.n_q = n_q;
  g.n_planes = n_planes;
  g.d_cap = d_cap;
  g.te_cap = te_cap;
  const int tiles = d_cap <= PG_TILE_ONE ? 1 : cdiv(d_cap, PG_TILE);
  const size_t lds = pg_lds_bytes(g.d_cap, g.te_cap);
  if (lds > 64 * 1024)   // above the default limit a kernel has to ask for its dynamic LDS
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)pg_lds_bytes(nnhip_phonon_large_max_dim(), PG_TILE_ONE)));
  pg_kernel<<<dim3(n_q, tiles * n_planes, n_cry), PH_THREADS, lds, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
