// Batched normal-mode analysis (gfx950, fp32): one workgroup per molecule diagonalises its mass-weighted Hessian block in LDS.
//
// nnhip_hessian_blocks (csrc/train_step.hip, csrc/hessian.hip) leaves one small dense symmetric matrix per molecule on the
// device, M = 3 n_b, mutually independent.  What a user wants from it is the spectrum, so this file does in ONE launch per batch:
//   1. load H_b from the packed blocks, symmetrise (H + H^T)/2 (the fp32 Hessian is symmetric only to rounding), mass-weight
//      A[ia][jb] = H[ia][jb] / sqrt(m_i m_j)                                                    (masses == null: unit masses)
//   2. optionally project the translations and rotations out: d_k = the translation / rotation vectors of the molecule in
//      mass-weighted coordinates about the centre of mass, orthonormalised by modified Gram-Schmidt in fp64 (a vector whose remainder
//      is not above 1e-5 of its own norm before is dropped: a linear molecule loses one rotation, one atom all three; a periodic
//      molecule -- any non-zero cell entry -- keeps the translations only), A <- P A P with P = I - sum_k d_k d_k^T, formed as
//      A - D U^T - U D^T with W = A D, G = D^T W, U = W - D G / 2, everything of this step in fp64
//   3. cyclic Jacobi with the round-robin ("tournament") ordering: Mp = M rounded up to even, P = Mp/2 disjoint rotations per step,
//      Mp - 1 steps per sweep.  Step s pairs (Mp - 1, s) and ((s + k) mod (Mp - 1), (s - k) mod (Mp - 1)), k = 1 .. P - 1 (the circle
//      method in closed form: no index tables).  A step is two barrier-separated phases:
//        a. thread k < P forms (c, s, t) of pair k from a_pp, a_qq, a_pq                                 (Rutishauser's formulas)
//        b. A <- J^T A J in 2 x 2 tiles: the thread of tile (k, l), k <= l, reads rows {p_k, q_k} x columns {p_l, q_l}, applies pair
//           k's rotation from the left and pair l's from the right in registers and writes the tile AND its mirror image -- the
//           row and the column phase of the textbook method in one pass over half the matrix, A stays exactly symmetric, no
//           element is touched by two threads; the diagonal tiles are written in closed form (a_pq = 0 exactly).  Rows p_k, q_k
//           of V^T take pair k's rotation in the same phase.
//      A and V^T live in LDS in fp32 with row stride Mp + 1 (odd: the column walks of the tiles, the symmetrisation and the
//      projection hit distinct banks).  V^T is kept rather than V so that its updates are row operations and row k is mode k.
//      After every sweep off(A)^2 and ||A||_F^2 are summed in a fixed order (fp64); stop at off(A) <= 2^-24 ||A||_F or after
//      EIG_MAX_SWEEPS sweeps (status bit 0).  A molecule with a mass that is not positive and finite is not computed (status bit 2).  An odd M idles on the padding index: its row and column are zero, so its rotations are
//      the identity.
//   4. rank the eigenvalues by counting (index as tie-break), fix each mode's sign (largest |component| positive, lowest index on a
//      tie) and write evals at 3 mol_ptr[b] and the modes, ROW k = mode k, at blk_ptr[b].
// No float atomics, every sum in a fixed order: two calls on the same input are bitwise identical.  modes == null skips V^T
// altogether (half the LDS, about half the work); A's arithmetic does not depend on V, so the eigenvalues are bitwise the same.
#include "eig_common.h"   // the steps themselves: shared with csrc/eig_large.hip

namespace {

// bytes of the region V^T and the projection scratch share (a multiple of 8)
__host__ __device__ inline size_t eig_x_bytes(int mp_max, bool want_v) {
  const size_t v = want_v ? 4 * (size_t)mp_max * (mp_max + 1) : 0, d = 8 * (12 * (size_t)mp_max + 36);
  return v > d ? v : d;
}

__global__ void __launch_bounds__(EIG_THREADS)
eig_kernel(EigArgs g) {
  extern __shared__ __align__(16) double smem_d[];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const int a0 = g.mol_ptr[b];
  const int nb = g.mol_ptr[b + 1] - a0;
  if (nb <= 0) return;   // (uniform over the workgroup)
  if (t == 0) {
    g.n_proj[b] = 0;
    g.sweeps[b] = 0;
    g.status[b] = 0;
  }
  const int M = 3 * nb;
  const int Mp = (M + 1) & ~1;
  if (Mp > g.mp_max) {   // mol_ptr and mol_ptr_host disagree: the LDS of this launch is too small for the molecule (uniform)
    if (t == 0) g.status[b] = NNHIP_EIG_STATUS_SIZE;
    return;
  }
  const int P = Mp >> 1;
  const int ld = Mp + 1;
  const bool want_v = g.modes != nullptr;
  // LDS carve-up, sized by the host for the largest molecule of the batch (g.mp_max).  The fp64 scratch of the projection (D, U,
  // G) shares its space with V^T, which is not needed before the Jacobi sweeps: an aspirin (Mp = 64) with modes takes 38 176
  // bytes, four workgroups per CU.
  const int mpx = g.mp_max;
  double* red = smem_d;                    // [EIG_THREADS]
  double* rsm = red + EIG_THREADS;         // [mpx] 1 / sqrt(m_i) (n_b entries used)
  float* cst = reinterpret_cast<float*>(rsm + mpx);             // [mpx / 2][4]  (c, s, t, -) of the step's pairs
  float* dg = cst + 4 * (mpx / 2);         // [mpx]  eigenvalues before sorting
  int* rank = reinterpret_cast<int*>(dg + mpx);                 // [mpx]
  float* sgn = reinterpret_cast<float*>(rank + mpx);            // [mpx]
  float* A = sgn + mpx;                    // [mpx][mpx + 1] (this molecule uses [Mp][ld])
  float* Vt = A + mpx * (mpx + 1);         // the same again when modes are wanted ...
  double* D = reinterpret_cast<double*>(Vt);   // ... [6][mpx] orthonormal translation / rotation vectors
  double* U = D + 6 * mpx;                 // [6][mpx]  W = A D, then U = W - D G / 2
  double* G = U + 6 * mpx;                 // [36]
  unsigned short* tab = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(Vt) + eig_x_bytes(mpx, want_v));   // [P (P + 1) / 2] tiles k <= l as k | l << 8
  eig_fill_tab(tab, P);

  // ---- 1. load, symmetrise, mass-weight; 2. projection ------------------------------------------------------------------
  if (!eig_load_project(g, b, a0, nb, Mp, A, ld, rsm, D, U, G, mpx, red)) {   // (uniform) its outputs keep what the caller put there
    if (t == 0) g.status[b] = NNHIP_EIG_STATUS_MASS;
    return;
  }

  // ---- 3. Jacobi ----------------------------------------------------------------------------------------------------------
  bool converged;
  const int n_sweeps = eig_jacobi(A, Vt, Mp, ld, cst, tab, red, want_v, EIG_EPS2, EIG_MAX_SWEEPS, converged);
  if (t == 0) {
    g.sweeps[b] = n_sweeps;
    g.status[b] = converged ? 0 : NNHIP_EIG_STATUS_SWEEPS;
  }

  // ---- 4. sort, fix signs, write ---------------------------------------------------------------------------------------
  eig_sort_write(A, Vt, M, ld, dg, rank, sgn, g.evals + 3 * (size_t)a0, want_v ? g.modes + g.blk_ptr[b] : nullptr, want_v);
}

size_t eig_lds_bytes(int mp_max, bool want_v) {
  const int p = mp_max / 2;
  return 8 * ((size_t)EIG_THREADS + mp_max) + 4 * (5 * (size_t)mp_max + (size_t)mp_max * (mp_max + 1)) + eig_x_bytes(mp_max, want_v) +
         2 * (size_t)(p * (p + 1) / 2);
}

}  // namespace

extern "C" int nnhip_eig_max_dim(void) { return EIG_MAX_DIM; }

extern "C" int nnhip_eig_blocks(const float* blocks, const int64_t* blk_ptr, const int32_t* mol_ptr, const int32_t* mol_ptr_host,
                                int32_t n_mol, const float* pos, const float* cell, const float* masses, int32_t flags, float* evals,
                                float* modes, int32_t* n_proj, int32_t* sweeps, int32_t* status, void* stream) {
  if (n_mol < 0 || (n_mol > 0 && (!blocks || !blk_ptr || !mol_ptr || !mol_ptr_host || !evals || !n_proj || !sweeps || !status)) ||
      ((flags & NNHIP_EIG_PROJECT) && n_mol > 0 && (!pos || !cell)) || (flags & ~NNHIP_EIG_PROJECT)) {
    nnhip_set_error("nnhip_eig_blocks: bad arguments");
    return NNHIP_E_INVALID;
  }
  int m_max = 0;
  for (int b = 0; b < n_mol; ++b) {
    const int m = 3 * (mol_ptr_host[b + 1] - mol_ptr_host[b]);
    if (m < 0) {
      nnhip_set_error("nnhip_eig_blocks: mol_ptr_host decreases at molecule %d", b);
      return NNHIP_E_INVALID;
    }
    if (m > EIG_MAX_DIM) {
      nnhip_set_error("nnhip_eig_blocks: molecule %d has dimension 3 x %d = %d, above the supported %d (one workgroup holds the "
                      "matrix and its eigenvectors in LDS)", b, m / 3, m, EIG_MAX_DIM);
      return NNHIP_E_UNSUPPORTED;
    }
    m_max = m > m_max ? m : m_max;
  }
  if (m_max == 0) return NNHIP_OK;
  EigArgs g;
  g.blocks = blocks;
  g.blk_ptr = blk_ptr;
  g.mol_ptr = mol_ptr;
  g.pos = pos;
  g.cell = cell;
  g.masses = masses;
  g.evals = evals;
  g.modes = modes;
  g.n_proj = n_proj;
  g.sweeps = sweeps;
  g.status = status;
  g.n_mol = n_mol;
  g.project = (flags & NNHIP_EIG_PROJECT) ? 1 : 0;
  g.mp_max = (m_max + 1) & ~1;
  const size_t lds = eig_lds_bytes(g.mp_max, modes != nullptr);
  if (lds > 64 * 1024)   // above the default limit a kernel has to ask for its dynamic LDS
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(eig_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)eig_lds_bytes((EIG_MAX_DIM + 1) & ~1, true)));
  eig_kernel<<<n_mol, EIG_THREADS, lds, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
