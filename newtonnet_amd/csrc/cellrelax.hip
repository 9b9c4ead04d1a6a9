// Variable-cell geometry relaxation on the device (gfx950, fp32): one launch per optimisation step moves the atoms AND the cell of
// every periodic system of a batch by one L-BFGS step.  The method is ASE's UnitCellFilter (ase/filters.py) under ASE's L-BFGS:
// the state of system b is the deformation gradient F and the reference-frame positions q, with  h = h0 F^T  and  x = q F^T  (h:
// the cell, rows are lattice vectors; h0: the cell the relaxation started from; x: Cartesian positions).  The optimiser sees
//   generalised coordinates  X = [q ; c F]                  n + 3 rows of 3     (c = cell_factor)
//   generalised forces       G = [f F ; Wc / c]             Wc = (W - p V I) F^-T, then hydrostatic / mask / constant volume
// and one step is lbfgs_chain::step on (X, G) -- the recursion of nnhip_lbfgs_step, one text (lbfgs_chain.h), through a policy over
// the generalised rows.  A step of the driver (newtonnet_amd/cellrelax.py) is  model(pos, cell) -> cell_lbfgs_step.
//
// Launch shape and discipline are relax.hip's: one wave64 per system, four systems per workgroup, grid-stride; no LDS, no float
// atomics; every operation an explicit __f*_rn; every decision uniform over the wave; a system's bits do not depend on the rest of
// the batch or on its place in it.  The arrays X, G, G_prev, S[k], Y[k], work have N + 3 B rows; system b owns the rows
// [mol_ptr[b] + 3 b, mol_ptr[b+1] + 3 b + 3): its n atom rows, then its 3 cell rows.  Row r of a system belongs to lane r % 64 in
// EVERY sweep (the chain's ownership), so a lane only re-reads what it wrote itself.
//
// The prologue, for one system (every lane forms the 3x3 quantities itself from the same loads, so they are uniform by
// construction; dot3(a, b) = fma(a2, b2, fma(a1, b1, a0 b0));  cof(A): C0 = A1 x A2, C1 = A2 x A0, C2 = A0 x A1 with
// (u x v)_0 = fma(u1, v2, -(u2 v1)), (u x v)_1 = fma(u2, v0, -(u0 v2)), (u x v)_2 = fma(u0, v1, -(u1 v0));  det(A) = dot3(A0, C0)):
//   F_jk   = X[n + j][k] / c                                       (nine quotients: exactly the F' the step before derived the cell from)
//   V      = det(cell_in)                                          (triple product form)
//   FinvT  = cof(F) / det(F)                                       (adjugate over determinant, nine quotients)
//   Wp     = W,  Wp_ii = W_ii - p V                                (p V one product)
//   Wc_ij  = fma(Wp_i2, FinvT_2j, fma(Wp_i1, FinvT_1j, Wp_i0 FinvT_0j))
//   hydrostatic:      t = ((Wc_00 + Wc_11) + Wc_22) / 3;  Wc = t I
//   mask:             Wc_ij = Wc_ij when the Voigt flag of (i, j) is set, else +0
//   constant volume:  t = ((Wc_00 + Wc_11) + Wc_22) / 3;  Wc_ii = Wc_ii - t
//   G cell row i  = Wc_i / c                                       (three quotients)
//   G atom row a  = (dot3 over k of f_ak F_kj)_j  for a free atom, exactly 0 for a fixed one
//   fmax2 = max_rows dot3(G_r, G_r);  fmax_out = sqrt(fmax2);  converged iff fmax2 < tol2
// then lbfgs_chain::step (pair, two-loop, clamp over all n + 3 rows, X_out = X + (-z), S[head] = X_out - X, G_prev = G), and the
// epilogue (the cell rows of X_out reach every lane by __shfl from their owners):
//   F'_jk  = X_out[n + j][k] / c
//   cell_out_ij = dot3 over k of h0_ik F'_jk                       (h0 F'^T)
//   pos_out_aj  = dot3 over k of q_ak F'_jk                        (q_out F'^T; q_out = the atom rows of X_out)
// tests/cellrelax_ref.py restates all of it in fp64 with one 2^-24 per operation.
//
// A second kernel, cell_lbfgs_step_wg_kernel (nnhip_cell_lbfgs_step_wg), gives a system one workgroup of NNHIP_LBFGS_WG_THREADS
// threads: the same text (cell_system below) instantiated with lbfgs_chain::BlockTeam (lbfgs_chain.h has the method and the rules).
// There thread t owns row t, t + 1024, ...; the cell rows of G are stored by their owners, and the epilogue's three cell rows of
// X_out reach every thread through LDS and a barrier.
#include "common.h"
#include "lbfgs_chain.h"

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_MAX_BLOCKS = 2048;
constexpr int CR_ALL_FLAGS = NNHIP_CELL_LBFGS_CHECK_ONLY | NNHIP_CELL_LBFGS_HYDROSTATIC | NNHIP_CELL_LBFGS_CONSTANT_VOLUME;

struct CellRelaxArgs {
  const float* x_in;
  const float* pos_in;
  const float* force;
  const float* virial;
  const float* cell_in;
  const float* h0;
  const uint8_t* free_mask;
  const int32_t* mol_ptr;
  const float* pressure;
  const float* cell_factor;
  int32_t* converged;
  int32_t* n_steps;
  int32_t* n_pairs;
  int32_t* head;
  float* S;
  float* Y;
  float* rho;
  float* g_prev;
  float* work;
  float* G;
  float* x_out;
  float* pos_out;
  float* cell_out;
  float* fmax_out;
  float tol2, alpha, maxstep;
  int flags, strain_mask, n_mol, n_atoms, memory;
  int wg_min_atoms;      // systems of at least this many atoms belong to cell_lbfgs_step_wg_kernel (<= 0: all)
};


__device__ __forceinline__ void cross3(const float* u, const float* v, float* c) {
  c[0] = __fmaf_rn(u[1], v[2], -__fmul_rn(u[2], v[1]));
  c[1] = __fmaf_rn(u[2], v[0], -__fmul_rn(u[0], v[2]));
  c[2] = __fmaf_rn(u[0], v[1], -__fmul_rn(u[1], v[0]));
}

// the cofactor matrix of A (rows) and its determinant
__device__ __forceinline__ float cof3(const float (*A)[3], float (*C)[3]) {
  cross3(A[1], A[2], C[0]);
  cross3(A[2], A[0], C[1]);
  cross3(A[0], A[1], C[2]);
  return dot3(A[0], C[0]);
}

__device__ __forceinline__ bool finite3x3(const float (*A)[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) ok = ok && isfinite(A[k / 3][k % 3]);
  return ok;
}

// row j of  v A^T:  out_j = dot3 over k of v_k A_jk
__device__ __forceinline__ void times_transposed(const float* v, const float (*A)[3], float* out) {
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = dot3(v, A[j]);
}

// the optimiser's view of this launch (lbfgs_chain.h): the generalised forces as the prologue stored them (a lane reads its own
// rows back), the step goes from x_in to x_out.  i counts generalised rows; the atom of an atom row is i - 3 b
struct CellPolicy {
  const CellRelaxArgs& g;
  int atom_shift, cell_row0;      // 3 b;  the system's first cell row
  __device__ __forceinline__ void force(int i, float* f) const { load3(g.G, 3 * (size_t)i, f); }
  __device__ __forceinline__ bool is_free(int i) const {
    return i >= cell_row0 || ::is_free(g, i - atom_shift);
  }
  __device__ __forceinline__ void load_x(size_t o, float* x) const { load3(g.x_in, o, x); }
  __device__ __forceinline__ void store_x(size_t o, const float* x_out, const float*) const { store3(g.x_out, o, x_out); }
};

// one system of a launch, by the team that owns it (relax.hip's relax_system, with the prologue and the epilogue of the cell).
// Every branch is taken on values all members of the team loaded from the same address or formed from such loads, or on a reduced
// value (the reductions of BlockTeam hold barriers); the state words are loaded before the first reduction, and member 0 stores
// them after it (converged) or after the reductions of the step (n_steps, n_pairs, head)
template <class Team>
__device__ __forceinline__ void cell_system(const CellRelaxArgs& g, Team& team, int b, int a0, int a1, bool bad_ptr) {
  const int m = g.memory;
  const int n_rows = g.n_atoms + 3 * g.n_mol;
  // state words no step can have left behind (or a mol_ptr that leaves the arrays): the system is not touched, fmax_out = NaN
  if (bad_ptr) {
    if (team.first() == 0) g.fmax_out[b] = __builtin_nanf("");
    return;
  }
  const int steps = g.n_steps[b];
  int np = g.n_pairs[b], head = g.head[b];
  const bool was = g.converged[b] != 0;
  if (steps < 0 || np < 0 || np > m || head < 0 || head >= m) {
    if (team.first() == 0) g.fmax_out[b] = __builtin_nanf("");
    return;
  }
  const int n = a1 - a0, r0 = a0 + 3 * b, rc = a1 + 3 * b, r1 = rc + 3;
  // ---- prologue: the 3x3 quantities, the same in every lane
  const float c = g.cell_factor[b], p = g.pressure[b];
  float F[3][3], h[3][3], W[3][3], C[3][3], FinvT[3][3], Wc[3][3], Gc[3][3];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    F[k / 3][k % 3] = __fdiv_rn(g.x_in[3 * (size_t)rc + k], c);
    h[k / 3][k % 3] = g.cell_in[9 * (size_t)b + k];
    W[k / 3][k % 3] = g.virial[9 * (size_t)b + k];
  }
  const float V = cof3(h, C);
  const float detF = cof3(F, C);
  // a cell no step can work with: det F <= 0, F or V not finite (or c, p that the host wrapper cannot see on the device)
  if (!(detF > 0.f) || !isfinite(detF) || !isfinite(V) || !finite3x3(F) || !(c > 0.f) || !isfinite(c) || !isfinite(p)) {
    if (team.first() == 0) g.fmax_out[b] = __builtin_nanf("");
    return;
  }
  const float pv = __fmul_rn(p, V);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) FinvT[i][j] = __fdiv_rn(C[i][j], detF);
    W[i][i] = __fsub_rn(W[i][i], pv);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      Wc[i][j] = __fmaf_rn(W[i][2], FinvT[2][j], __fmaf_rn(W[i][1], FinvT[1][j], __fmul_rn(W[i][0], FinvT[0][j])));
  if (g.flags & NNHIP_CELL_LBFGS_HYDROSTATIC) {
    const float t = __fdiv_rn(__fadd_rn(__fadd_rn(Wc[0][0], Wc[1][1]), Wc[2][2]), 3.0f);
#pragma unroll
    for (int k = 0; k < 9; ++k) Wc[k / 3][k % 3] = k / 3 == k % 3 ? t : 0.f;
  }
  {
    // Voigt order xx, yy, zz, yz, xz, xy: bit k of strain_mask frees that component
    const int voigt[3][3] = {{0, 5, 4}, {5, 1, 3}, {4, 3, 2}};
#pragma unroll
    for (int k = 0; k < 9; ++k)
      if (!((g.strain_mask >> voigt[k / 3][k % 3]) & 1)) Wc[k / 3][k % 3] = 0.f;
  }
  if (g.flags & NNHIP_CELL_LBFGS_CONSTANT_VOLUME) {
    const float t = __fdiv_rn(__fadd_rn(__fadd_rn(Wc[0][0], Wc[1][1]), Wc[2][2]), 3.0f);
#pragma unroll
    for (int i = 0; i < 3; ++i) Wc[i][i] = __fsub_rn(Wc[i][i], t);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) Gc[k / 3][k % 3] = __fdiv_rn(Wc[k / 3][k % 3], c);
  // ---- the lane's own rows of G, first for fmax alone (a frozen system's G buffer is not touched).  The three cell rows are the
  // same in every lane, so every lane takes them into its maximum (a maximum does not mind) and no lane selects a row by index
  auto atom_row = [&](int i, float* out) {
    const int a = i - 3 * b;
    float f[3];
    load3(g.force, 3 * (size_t)a, f);
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] = __fmaf_rn(f[2], F[2][j], __fmaf_rn(f[1], F[1][j], __fmul_rn(f[0], F[0][j])));
    if (g.free_mask && !g.free_mask[a]) out[0] = out[1] = out[2] = 0.f;
  };
  float f2 = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) f2 = fmaxf(f2, dot3(Gc[k], Gc[k]));
  for (int i = r0 + team.first(); i < rc; i += Team::STRIDE) {
    float gr[3];
    atom_row(i, gr);
    f2 = fmaxf(f2, dot3(gr, gr));
  }
  const float fmax2 = team.max(f2);
  const bool now = fmax2 < g.tol2;
  if (team.first() == 0) {
    g.fmax_out[b] = __fsqrt_rn(fmax2);
    if (now && !was) g.converged[b] = 1;
  }
  if (was || now || (g.flags & NNHIP_CELL_LBFGS_CHECK_ONLY)) {
    for (int i = r0 + team.first(); i < r1; i += Team::STRIDE) {
      float x[3];
      load3(g.x_in, 3 * (size_t)i, x);
      store3(g.x_out, 3 * (size_t)i, x);
    }
    for (int i = a0 + team.first(); i < a1; i += Team::STRIDE) {
      float x[3];
      load3(g.pos_in, 3 * (size_t)i, x);
      store3(g.pos_out, 3 * (size_t)i, x);
    }
    if (team.first() < 9) g.cell_out[9 * (size_t)b + team.first()] = g.cell_in[9 * (size_t)b + team.first()];
    return;
  }
  for (int i = r0 + team.first(); i < rc; i += Team::STRIDE) {
    float gr[3];
    atom_row(i, gr);
    store3(g.G, 3 * (size_t)i, gr);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (team.first() == (n + k) % Team::STRIDE) store3(g.G, 3 * (size_t)(rc + k), Gc[k]);   // (by the row's owner in the chain)
  // ---- the pending pair, the two-loop, the step: on the generalised rows
  const CellPolicy policy{g, 3 * b, rc};
  lbfgs_chain::History hist;
  hist.S = g.S, hist.Y = g.Y, hist.rho = g.rho, hist.f_prev = g.g_prev, hist.work = g.work;
  hist.alpha = g.alpha, hist.maxstep = g.maxstep, hist.memory = m, hist.n_atoms = n_rows;
  lbfgs_chain::step(hist, policy, team, b, r0, r1, steps > 0, np, head);
  if (team.first() == 0) {
    g.n_steps[b] = steps + 1;
    g.n_pairs[b] = np;
    g.head[b] = head;
  }
  // ---- epilogue: the new deformation gradient from the owners of the three cell rows, then the cell and the positions
  // (an owner reads back the row it stored itself; the others get it from the team: __shfl in a wave, LDS and a barrier in a
  // workgroup -- no member re-reads global memory another one wrote)
  float Fn[3][3];
  int owner[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    owner[k] = (n + k) % Team::STRIDE;
    Fn[k][0] = Fn[k][1] = Fn[k][2] = 0.f;
    if (team.first() == owner[k]) load3(g.x_out, 3 * (size_t)(rc + k), Fn[k]);
  }
  team.share_rows(owner, Fn);
#pragma unroll
  for (int k = 0; k < 9; ++k) Fn[k / 3][k % 3] = __fdiv_rn(Fn[k / 3][k % 3], c);
  if (team.first() < 3) {
    float h0r[3], row[3];
    load3(g.h0, 9 * (size_t)b + 3 * team.first(), h0r);
    times_transposed(h0r, Fn, row);
    store3(g.cell_out, 9 * (size_t)b + 3 * team.first(), row);
  }
  for (int i = r0 + team.first(); i < rc; i += Team::STRIDE) {
    float q[3], x[3];
    load3(g.x_out, 3 * (size_t)i, q);
    times_transposed(q, Fn, x);
    store3(g.pos_out, 3 * (size_t)(i - 3 * b), x);
  }
}

// (which of the two kernels below a system belongs to: lbfgs_chain::wave_owns; wg_min_atoms counts ATOMS, not generalised rows)
__global__ void __launch_bounds__(CR_THREADS)
cell_lbfgs_step_kernel(CellRelaxArgs g) {
  const int waves = CR_THREADS / 64;
  lbfgs_chain::WaveTeam team{(int)(threadIdx.x & 63)};
  for (int b = blockIdx.x * waves + (threadIdx.x >> 6); b < g.n_mol; b += gridDim.x * waves) {   // (uniform over a wave)
    const int a0 = g.mol_ptr[b], a1 = g.mol_ptr[b + 1];
    const bool bad_ptr = a0 < 0 || a1 < a0 || a1 > g.n_atoms;
    if (!lbfgs_chain::wave_owns(g.wg_min_atoms, a0, a1, bad_ptr)) continue;
    cell_system(g, team, b, a0, a1, bad_ptr);
  }
}

// The workgroup-per-system form: one workgroup of NNHIP_LBFGS_WG_THREADS threads per system, grid-stride over the systems
// (lbfgs_chain.h: BlockTeam has the method, the barrier argument and the rules).  The `continue` below is uniform over the
// workgroup (mol_ptr[b], mol_ptr[b + 1] and the arguments are the same loads in every thread), and so is every return of
// cell_system.  Thread t owns the generalised rows r0 + t, + 1024, ... of its system
__global__ void __launch_bounds__(NNHIP_LBFGS_WG_THREADS)
cell_lbfgs_step_wg_kernel(CellRelaxArgs g) {
  __shared__ float red[lbfgs_chain::BlockTeam::RED_FLOATS];
  __shared__ float rows[lbfgs_chain::BlockTeam::ROW_FLOATS];
  lbfgs_chain::BlockTeam team{red, rows, (int)threadIdx.x, 0};
  for (int b = blockIdx.x; b < g.n_mol; b += gridDim.x) {
    const int a0 = g.mol_ptr[b], a1 = g.mol_ptr[b + 1];
    const bool bad_ptr = a0 < 0 || a1 < a0 || a1 > g.n_atoms;
    if (lbfgs_chain::wave_owns(g.wg_min_atoms, a0, a1, bad_ptr)) continue;
    cell_system(g, team, b, a0, a1, bad_ptr);
  }
}

}  // namespace

// the checks and the launches of both entry points.  wave: launch cell_lbfgs_step_kernel; wg: launch cell_lbfgs_step_wg_kernel
static int cell_lbfgs_step_launch(const char* who, const float* x_in, const float* pos_in, const float* force, const float* virial,
                                  const float* cell_in, const float* h0, const uint8_t* free_mask, const int32_t* mol_ptr,
                                  const float* pressure, const float* cell_factor, int32_t n_mol, int32_t n_atoms, int32_t memory,
                                  float tol2, float alpha, float maxstep, int32_t strain_mask, int32_t wg_min_atoms, bool wave,
                                  bool wg, int32_t flags, int32_t* converged, int32_t* n_steps, int32_t* n_pairs, int32_t* head,
                                  float* S, float* Y, float* rho, float* g_prev, float* work, float* G, float* x_out, float* pos_out,
                                  float* cell_out, float* fmax_out, void* stream) {
  if (n_mol < 0 || n_atoms < 0 || memory < 1 || memory > NNHIP_LBFGS_MAX_MEMORY || (flags & ~CR_ALL_FLAGS) || strain_mask < 0 ||
      strain_mask > 63) {
    nnhip_set_error("%s: bad arguments (n_mol %d, n_atoms %d, memory %d: 1 .. %d, flags %d: bits of "
                    "NNHIP_CELL_LBFGS_*, strain_mask %d: 0 .. 63)", who, n_mol, n_atoms, memory, NNHIP_LBFGS_MAX_MEMORY, flags,
                    strain_mask);
    return NNHIP_E_INVALID;
  }
  if (!(tol2 >= 0.f) || !(alpha > 0.f) || !(maxstep > 0.f) || !(alpha <= 3.402823466e38f) || !(maxstep <= 3.402823466e38f)) {
    nnhip_set_error("%s: tol2 >= 0 and finite alpha > 0 and maxstep > 0 expected (got %g, %g, %g)", who, (double)tol2,
                    (double)alpha, (double)maxstep);
    return NNHIP_E_INVALID;
  }
  if (n_mol == 0) return NNHIP_OK;
  const size_t rows = (size_t)n_atoms + 3 * (size_t)n_mol;
  if (rows > 0x7fffffffu / 3) {
    nnhip_set_error("%s: n_atoms + 3 n_mol = %zu rows do not fit the 32-bit row index", who, rows);
    return NNHIP_E_INVALID;
  }
  if (!x_in || !virial || !cell_in || !h0 || !mol_ptr || !pressure || !cell_factor || !converged || !n_steps || !n_pairs || !head ||
      !S || !Y || !rho || !g_prev || !G || !x_out || !cell_out || !fmax_out || (rows > 64 && !work)) {
    nnhip_set_error("%s: null pointer (x_in, virial, cell_in, h0, mol_ptr, pressure, cell_factor, the state "
                    "arrays, G, x_out, cell_out and fmax_out are mandatory; work [N + 3 B, 3] when N + 3 B > 64)", who);
    return NNHIP_E_INVALID;
  }
  if (n_atoms > 0 && (!pos_in || !force || !pos_out)) {
    nnhip_set_error("%s: null pointer (pos_in, force and pos_out are mandatory when n_atoms > 0)", who);
    return NNHIP_E_INVALID;
  }
  if (overlap(x_in, x_out, 3 * rows) || overlap(cell_in, cell_out, 9 * (size_t)n_mol) ||
      (n_atoms > 0 && overlap(pos_in, pos_out, 3 * (size_t)n_atoms))) {
    nnhip_set_error("%s: x_out, pos_out and cell_out may not alias x_in, pos_in and cell_in (a forward call that "
                    "has to be repeated reads pos_in and cell_in again)", who);
    return NNHIP_E_INVALID;
  }
  CellRelaxArgs g;
  g.x_in = x_in;
  g.pos_in = pos_in;
  g.force = force;
  g.virial = virial;
  g.cell_in = cell_in;
  g.h0 = h0;
  g.free_mask = free_mask;
  g.mol_ptr = mol_ptr;
  g.pressure = pressure;
  g.cell_factor = cell_factor;
  g.converged = converged;
  g.n_steps = n_steps;
  g.n_pairs = n_pairs;
  g.head = head;
  g.S = S;
  g.Y = Y;
  g.rho = rho;
  g.g_prev = g_prev;
  g.work = work;
  g.G = G;
  g.x_out = x_out;
  g.pos_out = pos_out;
  g.cell_out = cell_out;
  g.fmax_out = fmax_out;
  g.tol2 = tol2;
  g.alpha = alpha;
  g.maxstep = maxstep;
  g.flags = flags;
  g.strain_mask = strain_mask;
  g.n_mol = n_mol;
  g.n_atoms = n_atoms;
  g.memory = memory;
  g.wg_min_atoms = wg_min_atoms;
  if (wave) {
    const int waves = CR_THREADS / 64;
    int blocks = (n_mol + waves - 1) / waves;
    blocks = blocks > CR_MAX_BLOCKS ? CR_MAX_BLOCKS : blocks;
    cell_lbfgs_step_kernel<<<blocks, CR_THREADS, 0, (hipStream_t)stream>>>(g);
    LAUNCH_CHECK();
  }
  if (wg) {
    const int blocks = n_mol > CR_MAX_BLOCKS ? CR_MAX_BLOCKS : n_mol;
    cell_lbfgs_step_wg_kernel<<<blocks, NNHIP_LBFGS_WG_THREADS, 0, (hipStream_t)stream>>>(g);
    LAUNCH_CHECK();
  }
  return NNHIP_OK;
}

extern "C" int nnhip_cell_lbfgs_step(const float* x_in, const float* pos_in, const float* force, const float* virial,
                                     const float* cell_in, const float* h0, const uint8_t* free_mask, const int32_t* mol_ptr,
                                     const float* pressure, const float* cell_factor, int32_t n_mol, int32_t n_atoms, int32_t memory,
                                     float tol2, float alpha, float maxstep, int32_t strain_mask, int32_t flags, int32_t* converged,
                                     int32_t* n_steps, int32_t* n_pairs, int32_t* head, float* S, float* Y, float* rho, float* g_prev,
                                     float* work, float* G, float* x_out, float* pos_out, float* cell_out, float* fmax_out,
                                     void* stream) {
  // (a threshold no system reaches: the wave kernel takes every system)
  return cell_lbfgs_step_launch("nnhip_cell_lbfgs_step", x_in, pos_in, force, virial, cell_in, h0, free_mask, mol_ptr, pressure,
                                cell_factor, n_mol, n_atoms, memory, tol2, alpha, maxstep, strain_mask, 0x7fffffff, true, false, flags,
                                converged, n_steps, n_pairs, head, S, Y, rho, g_prev, work, G, x_out, pos_out, cell_out, fmax_out,
                                stream);
}

extern "C" int nnhip_cell_lbfgs_step_wg(const float* x_in, const float* pos_in, const float* force, const float* virial,
                                        const float* cell_in, const float* h0, const uint8_t* free_mask, const int32_t* mol_ptr,
                                        const float* pressure, const float* cell_factor, int32_t n_mol, int32_t n_atoms,
                                        int32_t memory, float tol2, float alpha, float maxstep, int32_t strain_mask,
                                        int32_t wg_min_atoms, int32_t flags, int32_t* converged, int32_t* n_steps, int32_t* n_pairs,
                                        int32_t* head, float* S, float* Y, float* rho, float* g_prev, float* work, float* G,
                                        float* x_out, float* pos_out, float* cell_out, float* fmax_out, void* stream) {
  return cell_lbfgs_step_launch("nnhip_cell_lbfgs_step_wg", x_in, pos_in, force, virial, cell_in, h0, free_mask, mol_ptr, pressure,
                                cell_factor, n_mol, n_atoms, memory, tol2, alpha, maxstep, strain_mask, wg_min_atoms,
                                wg_min_atoms > 0, true, flags, converged, n_steps, n_pairs, head, S, Y, rho, g_prev, work, G, x_out,
                                pos_out, cell_out, fmax_out, stream);
}
