// Phonon group velocities (gfx950, fp32): d lambda / d q_cart of every mode of every (crystal, wave vector) problem in ONE launch,
// from the force constants, the image table and the eigenpairs nnhip_phonon_bands / nnhip_phonon_bands_large left in HBM.
//
// Hellmann-Feynman: d lambda_s / d q_a = e_s^H G_a e_s with G_a = d D / d q_cart,a, a = x, y, z.  G_a is D's own sum with one more
// factor per image,
//     G_a,ij = (m_i m_j)^-1/2 sum_J Phi(i, J) (1 / m_iJ) sum_T (i r_a) exp(2 pi i q . x_T),   G_a <- (G_a + G_a^H) / 2,
// r = x @ cell: the exact derivative of the symmetrised D the solvers diagonalise (ph_dweight, ph_accumulate and ph_hermitian of
// csrc/phonon_common.h: the phase in fp64, the copies R ascending, fmaf).  Modes are grouped by eigenvalue (consecutive sorted
// eigenvalues no more than deg_tol apart).  A group of one takes Re e^H G_a e.  A group of g > 1 (g <= PV_GROUP) forms
// M_a = V^H G_a V, diagonalises M_n = sum_a n_a M_a (n: the direction of the problem) with ph_jacobi in LDS, eigenvalues ascending,
// and its modes, in that order, take Re diag(U^H M_a U) -- degenerate perturbation theory along n.
//
// One workgroup of 256 threads per (crystal, q, tile of modes).  d <= PV_TILE_ONE: one tile holds every mode; above, a tile has
// PV_TILE modes, and a group belongs to the tile of its first mode, so a tile also looks at the PV_GROUP - 1 modes behind it.
// The workgroup streams G through LDS in blocks of PV_AI x PV_AJ atoms (12 x 24 elements, three components): the phase weights
// of PV_RCHUNK copies are staged at a time, the block and its transposed partner are summed element by element as D's are,
// then y_a,t[i] += sum_j G_a[i][j] e_t[j] over the block's columns (j ascending, the blocks ascending) for the tile's modes t,
// and once a block row is complete M_a[s][t] += conj(e_s[i]) y_a,t[i] (i ascending) for the s of t's group.  G is assembled once per
// tile: once per problem up to d = 96, twelve times at d = 768.  No workspace.
// Every sum has an order that belongs to its element; no float atomics; one writer per output (status: tile 0): a problem's
// result depends neither on the other problems of the launch nor on the run.
#include "phonon_common.h"

#define PV_TILE_ONE 96    // d up to which one tile holds every mode
#define PV_TILE 64        // modes per tile above
#define PV_GROUP 16       // largest degenerate group served (phonons.MAX_DEGENERATE)
#define PV_AI 4           // atoms per block row of G
#define PV_AJ 8           // atoms per block column
#define PV_RCHUNK 8       // supercell copies whose weights are staged at a time
#define PV_ROWS (3 * PV_AI)
#define PV_COLS (3 * PV_AJ)
#define PV_ELD (PV_COLS + 1)   // row stride of the staged modes (float2)
#define PV_JP (PV_GROUP + 1)   // row stride of the group's planes

namespace {

struct PvArgs {
  const float* fc;
  const int64_t* fc_ptr;
  const int* cry_ptr;
  const int* sc_atoms;
  const int64_t* img_ptr;
  const int* img_start;
  const double* img_off;
  const float* masses;
  const int64_t* out_ptr;
  const double* cells;
  const double* q;
  const double* direction;
  const float* evals;
  const float* modes;
  const float* deg_tol;
  const float* zero_tol;
  float* vel;
  float* dlam;
  int* group;
  uint8_t* defined;
  int* status;
  int n_q, d_cap, te_cap;
};

__host__ __device__ inline int pv_gcap(int te_cap) { return te_cap < PV_GROUP ? te_cap : PV_GROUP; }

// bytes of LDS of a workgroup that serves up to d_cap coordinates with up to te_cap modes in view (the layout of pv_kernel)
__host__ __device__ inline size_t pv_lds_bytes(int d_cap, int te_cap) {
  const size_t f64 = (size_t)((d_cap / 3 + 2) & ~1) + 2 * PV_GROUP;   // (even: the float4 behind it stays aligned)
  const size_t f2 = 2 * (size_t)3 * PV_ROWS * PV_COLS + 2 * (size_t)PV_RCHUNK * PV_AI * PV_AJ * 3 + (size_t)te_cap * PV_ELD +
                    (size_t)3 * PV_ROWS * te_cap + (size_t)3 * te_cap * pv_gcap(te_cap);
  const size_t f32 = (size_t)d_cap + 4 * (size_t)PV_GROUP * PV_JP + 2 * PV_GROUP;
  const size_t i32 = 2 * (size_t)d_cap + PV_GROUP + 4;
  return 8 * f64 + 16 * (PV_GROUP / 2) + 8 * f2 + 4 * f32 + 4 * i32 + 2 * 64;
}

// the outputs of mode `idx` (its index over the whole call): dl = d lambda / d q_cart, zero and undefined for a capped group
__device__ __forceinline__ void pv_write(const PvArgs& g, size_t idx, int first, float lam, float ztol, float dx, float dy, float dz,
                                         bool capped) {
  const float al = fabsf(lam);
  const bool def = !capped && al > ztol;
  const float h = def ? 0.5f / sqrtf(al) : 0.f;
  if (capped) dx = dy = dz = 0.f;
  g.vel[3 * idx] = def ? dx * h : 0.f;
  g.vel[3 * idx + 1] = def ? dy * h : 0.f;
  g.vel[3 * idx + 2] = def ? dz * h : 0.f;
  if (g.dlam) {
    g.dlam[3 * idx] = dx;
    g.dlam[3 * idx + 1] = dy;
    g.dlam[3 * idx + 2] = dz;
  }
  if (g.group) g.group[idx] = first;
  g.defined[idx] = def ? 1 : 0;
}

__global__ void __launch_bounds__(PH_THREADS)
pv_kernel(PvArgs g) {
  extern __shared__ __align__(16) char pv_smem[];
  const int t = threadIdx.x;
  const int qi = blockIdx.x, b = blockIdx.z;
  const int a0 = g.cry_ptr[b];
  const int n = g.cry_ptr[b + 1] - a0;
  if (n <= 0) return;   // (uniform)
  const int d = 3 * n;
  const int TM = d <= PV_TILE_ONE ? d : PV_TILE;
  const int t0 = blockIdx.y * TM;
  if (t0 >= d) return;
  const size_t prob = (size_t)b * g.n_q + qi;
  if (d > g.d_cap) {   // cry_ptr and cry_ptr_host disagree: this launch's LDS and grid are too small for the crystal
    if (t == 0 && blockIdx.y == 0) g.status[prob] = NNHIP_EIG_STATUS_SIZE;
    return;
  }
  int bad_mass = 0;
  for (int i = 0; i < n; ++i) {
    const float m = g.masses ? g.masses[a0 + i] : 1.f;
    bad_mass |= !(m > 0.f && m <= 3.4e38f);
  }
  if (bad_mass) {   // (uniform: every thread looked at every mass)
    if (t == 0 && blockIdx.y == 0) g.status[prob] = NNHIP_EIG_STATUS_MASS;
    return;
  }
  const int t1 = t0 + TM < d ? t0 + TM : d;                                       // the tile's own modes: t0 .. t1 - 1
  const int te = (t1 + PV_GROUP - 1 < d ? t1 + PV_GROUP - 1 : d) - t0;            // the modes in view
  const int d_cap = g.d_cap, te_cap = g.te_cap, gcap = pv_gcap(g.te_cap);
  if (te > te_cap) {   // (cry_ptr and cry_ptr_host disagree within d_cap: the tile sees more modes than the LDS was sized for)
    if (t == 0 && blockIdx.y == 0) g.status[prob] = NNHIP_EIG_STATUS_SIZE;
    return;
  }

  double* rsm = reinterpret_cast<double*>(pv_smem);                // [d_cap / 3, rounded up to even] 1 / sqrt(m_i)
  double* rowo = rsm + ((d_cap / 3 + 2) & ~1);                            // [PV_GROUP] scratch of ph_jacobi ...
  double* rowd = rowo + PV_GROUP;
  float4* cst = reinterpret_cast<float4*>(rowd + PV_GROUP);        // [PV_GROUP / 2]
  float2* Gd = reinterpret_cast<float2*>(cst + PV_GROUP / 2);      // [3][PV_ROWS][PV_COLS] sums of the block, then G itself
  float2* Gt = Gd + 3 * PV_ROWS * PV_COLS;                         // ... of the transposed block
  float2* wd = Gt + 3 * PV_ROWS * PV_COLS;                         // [PV_RCHUNK][ai][aj][3] weights of the block's pairs
  float2* wt = wd + PV_RCHUNK * PV_AI * PV_AJ * 3;                 // [PV_RCHUNK][aj][ai][3] ... of the transposed pairs
  float2* E = wt + PV_RCHUNK * PV_AI * PV_AJ * 3;                  // [te_cap][PV_ELD] the modes in view at the block's columns
  float2* Y = E + (size_t)te_cap * PV_ELD;                         // [3][te_cap][PV_ROWS]
  float2* Mg = Y + (size_t)3 * PV_ROWS * te_cap;                   // [3][te_cap][gcap]: M_a[s][t] at [a][t][s - first(t)]
  float* lam = reinterpret_cast<float*>(Mg + (size_t)3 * te_cap * gcap);   // [d_cap]
  float* Are = lam + d_cap;                                        // [PV_GROUP][PV_JP] x 4: the group's M_n and its vectors
  float* Aim = Are + PV_GROUP * PV_JP;
  float* Wre = Aim + PV_GROUP * PV_JP;
  float* Wim = Wre + PV_GROUP * PV_JP;
  float* dlt = Wim + PV_GROUP * PV_JP;                             // [PV_GROUP]
  float* dg = dlt + PV_GROUP;                                      // [PV_GROUP]
  int* gs = reinterpret_cast<int*>(dg + PV_GROUP);                 // [d_cap] first mode of the mode's group
  int* ge = gs + d_cap;                                            // [d_cap] one past its last
  int* rank = ge + d_cap;                                          // [PV_GROUP]
  int* flag = rank + PV_GROUP;                                     // [4]
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
    for (int k = t0 + t; k < t1; k += PH_THREADS) g.defined[out0 + k] = 0;
    if (t == 0 && blockIdx.y == 0) g.status[prob] = NNHIP_PHONON_STATUS_NONFINITE;
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
    if (e - s > PV_GROUP) flag[1] = 1;
  }
  for (int e = t; e < 3 * te_cap * gcap; e += PH_THREADS) Mg[e] = make_float2(0.f, 0.f);
  __syncthreads();
  if (t == 0 && blockIdx.y == 0) g.status[prob] = flag[1] ? NNHIP_PHONON_STATUS_GROUP : 0;

  // ---- the direction of the problem ------------------------------------------------------------------------------------------
  double cell[9];
  for (int c = 0; c < 9; ++c) cell[c] = g.cells[9 * (size_t)b + c];
  const double q0 = g.q[3 * (size_t)qi], q1 = g.q[3 * (size_t)qi + 1], q2 = g.q[3 * (size_t)qi + 2];
  float nx, ny, nz;
  if (g.direction) {
    nx = (float)g.direction[3 * (size_t)qi];
    ny = (float)g.direction[3 * (size_t)qi + 1];
    nz = (float)g.direction[3 * (size_t)qi + 2];
  } else {   // q_cart / |q_cart|, q_cart = 2 pi q_frac @ inv(cell)^T: the reciprocal vectors are the cross products / V
    const double bx0 = cell[4] * cell[8] - cell[5] * cell[7], by0 = cell[5] * cell[6] - cell[3] * cell[8],
                 bz0 = cell[3] * cell[7] - cell[4] * cell[6];
    const double bx1 = cell[7] * cell[2] - cell[8] * cell[1], by1 = cell[8] * cell[0] - cell[6] * cell[2],
                 bz1 = cell[6] * cell[1] - cell[7] * cell[0];
    const double bx2 = cell[1] * cell[5] - cell[2] * cell[4], by2 = cell[2] * cell[3] - cell[0] * cell[5],
                 bz2 = cell[0] * cell[4] - cell[1] * cell[3];
    const double vol = cell[0] * bx0 + cell[1] * by0 + cell[2] * bz0;
    const double cx = (q0 * bx0 + q1 * bx1 + q2 * bx2) / vol, cy = (q0 * by0 + q1 * by1 + q2 * by2) / vol,
                 cz = (q0 * bz0 + q1 * bz1 + q2 * bz2) / vol;
    const double nn = sqrt(cx * cx + cy * cy + cz * cz);
    nx = nn > 0.0 ? (float)(cx / nn) : 1.f;
    ny = nn > 0.0 ? (float)(cy / nn) : 0.f;
    nz = nn > 0.0 ? (float)(cz / nn) : 0.f;
  }

  // ---- M_a = V^H G_a V of the tile's groups, G streamed block by block -------------------------------------------------------
  const int N = g.sc_atoms[b];
  const int nR = N / n;
  const float* fc = g.fc + g.fc_ptr[b];
  const int* ist = g.img_start + g.img_ptr[b];
  for (int I0 = 0; I0 < n; I0 += PV_AI) {
    const int ai = n - I0 < PV_AI ? n - I0 : PV_AI;
    const int rows = 3 * ai;
    for (int J0 = 0; J0 < n; J0 += PV_AJ) {
      const int aj = n - J0 < PV_AJ ? n - J0 : PV_AJ;
      const int cols = 3 * aj;
      __syncthreads();   // the block before this one has been used (E, G) and, at J0 = 0, the block row before it (Y)
      for (int e = t; e < te * cols; e += PH_THREADS) {
        const int tt = e / cols, jc = e - tt * cols;
        E[tt * PV_ELD + jc] = modes[(size_t)(t0 + tt) * d + 3 * J0 + jc];
      }
      const int wr = ai * aj * 3;   // weights per copy
      for (int R0 = 0; R0 < nR; R0 += PV_RCHUNK) {
        const int rc = nR - R0 < PV_RCHUNK ? nR - R0 : PV_RCHUNK;
        if (R0 > 0) __syncthreads();   // the chunk before this one has been summed
        for (int x = t; x < rc * ai * aj; x += PH_THREADS) {
          const int r = x / (ai * aj), rem = x - r * ai * aj;
          const int ii = rem / aj, jj = rem - ii * aj;
          ph_dweight(ist, g.img_off, (size_t)(I0 + ii) * N + (size_t)(R0 + r) * n + (J0 + jj), q0, q1, q2, cell, wd + (size_t)x * 3);
          ph_dweight(ist, g.img_off, (size_t)(J0 + jj) * N + (size_t)(R0 + r) * n + (I0 + ii), q0, q1, q2, cell,
                     wt + (size_t)((r * aj + jj) * ai + ii) * 3);
        }
        __syncthreads();
        for (int e = t; e < rows * cols; e += PH_THREADS) {
          const int ir = e / cols, jc = e - ir * cols;
          const int ii = ir / 3, al = ir - 3 * ii, jj = jc / 3, be = jc - 3 * jj;
          const float* fd = fc + ((size_t)(3 * I0 + ir) * N + (size_t)R0 * n + (J0 + jj)) * 3 + be;
          const float* ft = fc + ((size_t)(3 * J0 + jc) * N + (size_t)R0 * n + (I0 + ii)) * 3 + al;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const int ge_ = a * PV_ROWS * PV_COLS + ir * PV_COLS + jc;
            float2 sd = R0 ? Gd[ge_] : make_float2(0.f, 0.f), st = R0 ? Gt[ge_] : make_float2(0.f, 0.f);
            ph_accumulate(fd, n, wd + (ii * aj + jj) * 3 + a, wr, rc, sd.x, sd.y);
            ph_accumulate(ft, n, wt + (jj * ai + ii) * 3 + a, wr, rc, st.x, st.y);
            Gd[ge_] = sd;
            Gt[ge_] = st;
          }
        }
      }
      for (int e = t; e < rows * cols; e += PH_THREADS) {   // (the thread that summed element e)
        const int ir = e / cols, jc = e - ir * cols;
        if (nR == 0) {
          for (int a = 0; a < 3; ++a) Gd[a * PV_ROWS * PV_COLS + ir * PV_COLS + jc] = Gt[a * PV_ROWS * PV_COLS + ir * PV_COLS + jc] = make_float2(0.f, 0.f);
        }
        const float f = (float)(rsm[I0 + ir / 3] * rsm[J0 + jc / 3]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const int ge_ = a * PV_ROWS * PV_COLS + ir * PV_COLS + jc;
          const float2 sd = Gd[ge_], st = Gt[ge_];
          float re, im;
          ph_hermitian(sd.x, sd.y, st.x, st.y, f, 3 * I0 + ir == 3 * J0 + jc, re, im);
          Gd[ge_] = make_float2(re, im);
        }
      }
      __syncthreads();
      for (int p = t; p < rows * te; p += PH_THREADS) {
        const int tt = p / rows, ir = p - tt * rows;
        const int k = t0 + tt, s = gs[k];
        if (s < t0 || s >= t1 || ge[k] - s > PV_GROUP) continue;   // the group is another tile's, or above the cap
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const int yi = (a * te_cap + tt) * PV_ROWS + ir;
          float2 acc = J0 ? Y[yi] : make_float2(0.f, 0.f);
          const float2* gr = Gd + a * PV_ROWS * PV_COLS + ir * PV_COLS;
          for (int jc = 0; jc < cols; ++jc) {
            const float2 gv = gr[jc], ev = E[tt * PV_ELD + jc];
            acc.x = fmaf(gv.x, ev.x, fmaf(-gv.y, ev.y, acc.x));
            acc.y = fmaf(gv.x, ev.y, fmaf(gv.y, ev.x, acc.y));
          }
          Y[yi] = acc;
        }
      }
    }
    __syncthreads();
    for (int p = t; p < te * gcap; p += PH_THREADS) {
      const int tt = p / gcap, so = p - tt * gcap;
      const int k = t0 + tt, s0 = gs[k];
      if (s0 < t0 || s0 >= t1 || ge[k] - s0 > PV_GROUP || so >= ge[k] - s0) continue;
      const float2* es = modes + (size_t)(s0 + so) * d + 3 * I0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        float2 acc = Mg[(size_t)a * te_cap * gcap + p];
        const float2* y = Y + (a * te_cap + tt) * PV_ROWS;
        for (int ir = 0; ir < rows; ++ir) {
          const float2 ev = es[ir], yv = y[ir];
          acc.x = fmaf(ev.x, yv.x, fmaf(ev.y, yv.y, acc.x));
          acc.y = fmaf(ev.x, yv.y, fmaf(-ev.y, yv.x, acc.y));
        }
        Mg[(size_t)a * te_cap * gcap + p] = acc;
      }
    }
  }
  __syncthreads();

  // ---- groups of one, and groups above the cap ---------------------------------------------------------------------------------
  const size_t mstride = (size_t)te_cap * gcap;
  for (int k = t0 + t; k < d; k += PH_THREADS) {
    const int s = gs[k], sz = ge[k] - s;
    if (s < t0 || s >= t1) continue;
    if (sz > PV_GROUP) {
      pv_write(g, out0 + k, s, lam[k], ztol, 0.f, 0.f, 0.f, true);
    } else if (sz == 1) {
      const size_t p = (size_t)(k - t0) * gcap;
      pv_write(g, out0 + k, s, lam[k], ztol, Mg[p].x, Mg[mstride + p].x, Mg[2 * mstride + p].x, false);
    }
  }

  // ---- degenerate groups: diagonalise M_n, rotate the M_a ------------------------------------------------------------------------
  for (int k0 = t0; k0 < t1; ++k0) {
    const int sz = ge[k0] - k0;
    if (gs[k0] != k0 || sz < 2 || sz > PV_GROUP) continue;   // (uniform)
    const int tt0 = k0 - t0;
    const int Mp = (sz + 1) & ~1, P = Mp >> 1;
    __syncthreads();   // the group before this one is done with the planes
    for (int e = t; e < Mp * PV_JP; e += PH_THREADS) {
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
      const size_t p = (size_t)(tt0 + c) * gcap + s;
      const float2 mx = Mg[p], my = Mg[mstride + p], mz = Mg[2 * mstride + p];
      const float re = fmaf(nz, mz.x, fmaf(ny, my.x, nx * mx.x));
      const float im = s == c ? 0.f : fmaf(nz, mz.y, fmaf(ny, my.y, nx * mx.y));
      Are[s * PV_JP + c] = re;
      Are[c * PV_JP + s] = re;
      Aim[s * PV_JP + c] = im;
      Aim[c * PV_JP + s] = -im;
    }
    __syncthreads();
    bool converged;
    ph_jacobi<false>(Are, Aim, Wre, Wim, Mp, PV_JP, rowo, rowd, cst, dlt, tab, true, EIG_EPS2, EIG_MAX_SWEEPS, t, converged);
    __syncthreads();
    if (t < sz) dg[t] = Are[t * PV_JP + t];
    __syncthreads();
    if (t < sz) {
      const float di = dg[t];
      int r = 0;
      for (int j = 0; j < sz; ++j) {
        const float dj = dg[j];
        r += dj < di || (dj == di && j < t) ? 1 : 0;
      }
      // Re u^H M_a u with u = row t of W, s then c ascending
      float dl[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        float acc = 0.f;
        for (int s = 0; s < sz; ++s) {
          const float usr = Wre[t * PV_JP + s], usi = Wim[t * PV_JP + s];
          float zr = 0.f, zi = 0.f;   // sum_c M_a[s][c] u[c]
          for (int c = 0; c < sz; ++c) {
            const float2 m = Mg[a * mstride + (size_t)(tt0 + c) * gcap + s];
            const float ucr = Wre[t * PV_JP + c], uci = Wim[t * PV_JP + c];
            zr = fmaf(m.x, ucr, fmaf(-m.y, uci, zr));
            zi = fmaf(m.x, uci, fmaf(m.y, ucr, zi));
          }
          acc = fmaf(usr, zr, fmaf(usi, zi, acc));
        }
        dl[a] = acc;
      }
      const int k = k0 + r;
      pv_write(g, out0 + k, k0, lam[k], ztol, dl[0], dl[1], dl[2], false);
    }
  }
}

}  // namespace

extern "C" int nnhip_phonon_velocities(const float* fc, const int64_t* fc_ptr, const int32_t* cry_ptr, const int32_t* cry_ptr_host,
                                       const int32_t* sc_atoms, const int64_t* img_ptr, const int32_t* img_start,
                                       const double* img_off, const float* masses, const int64_t* out_ptr, int32_t n_cry,
                                       const double* cells, const double* q, int32_t n_q, const double* direction,
                                       const float* evals, const float* modes, const float* deg_tol, const float* zero_tol,
                                       float* vel, float* dlam, int32_t* group, uint8_t* defined, int32_t* status, void* stream) {
  if (n_cry < 0 || n_q < 0 ||
      (n_cry > 0 && n_q > 0 && (!fc || !fc_ptr || !cry_ptr || !cry_ptr_host || !sc_atoms || !img_ptr || !img_start || !img_off ||
                                !out_ptr || !cells || !q || !evals || !modes || !deg_tol || !zero_tol || !vel || !defined ||
                                !status))) {
    nnhip_set_error("nnhip_phonon_velocities: bad arguments");
    return NNHIP_E_INVALID;
  }
  if (n_cry > 65535) {
    nnhip_set_error("nnhip_phonon_velocities: %d crystals in one call, above the 65535 a launch addresses", n_cry);
    return NNHIP_E_UNSUPPORTED;
  }
  const int bound = nnhip_phonon_large_max_dim();
  int d_cap = 0, te_cap = 0;
  for (int b = 0; b < n_cry; ++b) {
    const int m = 3 * (cry_ptr_host[b + 1] - cry_ptr_host[b]);
    if (m < 0) {
      nnhip_set_error("nnhip_phonon_velocities: cry_ptr_host decreases at crystal %d", b);
      return NNHIP_E_INVALID;
    }
    if (m > bound) {
      nnhip_set_error("nnhip_phonon_velocities: crystal %d has dimension 3 x %d = %d, above the supported %d "
                      "(nnhip_phonon_large_max_dim)", b, m / 3, m, bound);
      return NNHIP_E_UNSUPPORTED;
    }
    d_cap = m > d_cap ? m : d_cap;
    const int te = m <= PV_TILE_ONE ? m : PV_TILE + PV_GROUP - 1;   // the modes a tile of this crystal has in view
    te_cap = te > te_cap ? te : te_cap;
  }
  if (d_cap == 0 || n_q == 0) return NNHIP_OK;
  PvArgs g;
  g.fc = fc;
  g.fc_ptr = fc_ptr;
  g.cry_ptr = cry_ptr;
  g.sc_atoms = sc_atoms;
  g.img_ptr = img_ptr;
  g.img_start = img_start;
  g.img_off = img_off;
  g.masses = masses;
  g.out_ptr = out_ptr;
  g.cells = cells;
  g.q = q;
  g.direction = direction;
  g.evals = evals;
  g.modes = modes;
  g.deg_tol = deg_tol;
  g.zero_tol = zero_tol;
  g.vel = vel;
  g.dlam = dlam;
  g.group = group;
  g.defined = defined;
  g.status = status;
  g.n_q = n_q;
  g.d_cap = d_cap;
  g.te_cap = te_cap;
  const int tiles = d_cap <= PV_TILE_ONE ? 1 : cdiv(d_cap, PV_TILE);
  const size_t lds = pv_lds_bytes(g.d_cap, g.te_cap);
  if (lds > 64 * 1024)   // above the default limit a kernel has to ask for its dynamic LDS
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)pv_lds_bytes(nnhip_phonon_large_max_dim(), PV_TILE_ONE)));
  pv_kernel<<<dim3(n_q, tiles, n_cry), PH_THREADS, lds, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
