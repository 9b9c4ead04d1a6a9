// The pair predicate of the neighbour list (csrc/graph.hip) and of everything that must agree with it bit for bit (the pair-distance
// histogram of csrc/observables.hip): the cell of a system, and the displacement of a pair under the reference's single-image shift.
#pragma once
#include "common.h"

struct CellInfo {
  bool pbc;
  bool diag;     // orthorhombic box along the axes: the fractional coordinate is an exact division (see pair_disp)
  float c[9];    // cell, rows = lattice vectors (ASE convention, ase_interface.py:136)
  float inv[9];  // inverse of cell^T (fp32 of an fp64 inverse)
};

__device__ __forceinline__ CellInfo load_cell(const float* __restrict__ cell, long b) {
  CellInfo ci;
  bool any = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    ci.c[k] = cell[b * 9 + k];
    any |= (ci.c[k] != 0.0f);
  }
  ci.pbc = any;
  ci.diag = ci.c[1] == 0.f && ci.c[2] == 0.f && ci.c[3] == 0.f && ci.c[5] == 0.f && ci.c[6] == 0.f && ci.c[7] == 0.f &&
            ci.c[0] != 0.f && ci.c[4] != 0.f && ci.c[8] != 0.f;
  if (any) {
    // A = cell^T ; frac = A^{-1} d   (representations.py:92)
    double a[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) a[r * 3 + c] = (double)ci.c[c * 3 + r];
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    const double id = 1.0 / det;
    ci.inv[0] = (float)(c00 * id);
    ci.inv[1] = (float)((a[2] * a[7] - a[1] * a[8]) * id);
    ci.inv[2] = (float)((a[1] * a[5] - a[2] * a[4]) * id);
    ci.inv[3] = (float)(c01 * id);
    ci.inv[4] = (float)((a[0] * a[8] - a[2] * a[6]) * id);
    ci.inv[5] = (float)((a[2] * a[3] - a[0] * a[5]) * id);
    ci.inv[6] = (float)(c02 * id);
    ci.inv[7] = (float)((a[1] * a[6] - a[0] * a[7]) * id);
    ci.inv[8] = (float)((a[0] * a[4] - a[1] * a[3]) * id);
  }
  return ci;
}

// disp = pos_i - pos_j with the reference's single-image shift; returns ||disp||^2 (see cut2_of in graph.hip for the predicate).  fp32 with compiler FMA contraction
// switched off and every rounding written out, so that the count and fill passes agree with each other AND with the
// reference's fp32 CPU evaluation on the strict `< r` predicate (representations.py:96, pinned by
// tests/golden/case_boundary.npz: pairs within a few ulp of the cutoff):
//   * dist.norm(dim=1) on torch CPU is sqrt(fma(z, z, fma(y, y, x * x))) -- measured: 0 of 200,000 tie-range vectors differ
//     (the plain (x*x + y*y) + z*z differs from it in 9.5 % of them, 1 % of the predicates);
//   * torch.linalg.solve(cell^T, d) for an axis-aligned box is the exact division d_k / L_k (0 of 300,000 differ; the product
//     with a rounded 1/L differs in 28 %).  For a general (triclinic) cell the reference goes through MKL's LU solve, whose
//     roundings are not reproducible from outside (they also depend on the CPU dispatch): the product with the fp32 image of
//     the fp64 inverse used here differs from it by <= 2 ulp, which can pick the other image only for a pair whose
//     fractional separation is within 2 ulp of +-0.5 -- and then changes the edge SET only if that pair also sits within
//     a few ulp of the cutoff (tests count those double ties).
// The reference's predicate is sqrt_rn(r2) < cutoff.  gfx950 has no correctly rounded fp32 square root (v_sqrt_f32 is
// 1 ulp; hipcc emits it bare for sqrtf and __fsqrt_rn alike -- on the boundary fixture it admitted 162 pairs the reference
// rejects), so the host turns the cutoff into the equivalent threshold on r2 once: the smallest float T with
// sqrt_rn(T) >= cutoff (the host's sqrtf IS correctly rounded, and sqrt is monotone), and the kernels test r2 < T.
// (cut2_of itself is host code of graph.hip.)
__device__ __forceinline__ float pair_disp(float xi, float yi, float zi, float xj, float yj, float zj,
                                           const CellInfo& ci, float& dx, float& dy, float& dz) {
#pragma clang fp contract(off)
  dx = xi - xj;
  dy = yi - yj;
  dz = zi - zj;
  if (ci.pbc) {
    float f0, f1, f2;
    if (ci.diag) {
      f0 = __fdiv_rn(dx, ci.c[0]);
      f1 = __fdiv_rn(dy, ci.c[4]);
      f2 = __fdiv_rn(dz, ci.c[8]);
    } else {
      f0 = (ci.inv[0] * dx + ci.inv[1] * dy) + ci.inv[2] * dz;
      f1 = (ci.inv[3] * dx + ci.inv[4] * dy) + ci.inv[5] * dz;
      f2 = (ci.inv[6] * dx + ci.inv[7] * dy) + ci.inv[8] * dz;
    }
    const float n0 = rintf(f0), n1 = rintf(f1), n2 = rintf(f2);  // round-half-even == torch.round
    // d -= cell @ n   (as the reference writes it, representations.py:93)
    dx = dx - ((ci.c[0] * n0 + ci.c[1] * n1) + ci.c[2] * n2);
    dy = dy - ((ci.c[3] * n0 + ci.c[4] * n1) + ci.c[5] * n2);
    dz = dz - ((ci.c[6] * n0 + ci.c[7] * n1) + ci.c[8] * n2);
  }
  return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));   // |disp|^2; callers compare with cut2_of(cutoff)
}
