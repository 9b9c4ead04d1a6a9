// Bond-length constraints for molecular dynamics on the device (gfx950, fp32): one launch per MD step integrates every molecule of
// a batch between two force evaluations and keeps its constrained distances, |x_i - x_j| = d_c.
//
// The scheme is constrained BAOAB ("g-BAOAB", Leimkuhler & Matthews 2016, one RATTLE per half drift); with c1 = 1 and no noise it
// is velocity-Verlet RATTLE in two half drifts.  For one molecule, in this order (include/newtonnet_hip.h spells the contract out,
// tests/rattle_ref.py restates the chain in fp64 and emulates it in fp32; half_kick, kinetic and o_step are nnhip_md_step's, from
// csrc/md_chain.h):
//   finish (flag bit 0):  half_kick;  PROJECT v at y;  ke_i = kinetic                            (ke only when ke_out != NULL)
//   begin  (flag bit 1):  half_kick;  PROJECT v at y;  DRIFT;  [o_step;  PROJECT v at y]  DRIFT   (the bracket only with noise)
//   DRIFT:                r = y;  y = fma(dth, v, r);  D = 0;  SHAKE y with the directions r, every update also added into D;
//                         v = fma(D, inv_dth, v);  PROJECT v at y
//                         (D = y'' - y' is the SUM of the applied updates, not the difference of the two positions: the difference
//                         carries the rounding of |y|, 2^-24 |y| / dth per update in the velocities, and that is what an NVE
//                         run at 0.5 fs showed as energy drift -- DESIGN.md section 17)
//   project (flag bit 2, alone):  r = y;  SHAKE y with the directions r;  PROJECT v at y
// y = x - x_first is the molecule-relative position (one fp32 subtraction of the first atom's INPUT position per coordinate) and
// x_out = x_first + y (one fp32 addition): the solver's convergence then does not depend on where a molecule sits (DESIGN.md
// section 17 has the measurement).  An atom with inv_mass = 0 gets pos_out = pos_in bit for bit.
//
// SHAKE and PROJECT are Gauss-Seidel sweeps over the molecule's constraints in COLOUR order: the host colours each molecule's
// constraint graph so that no two constraints of a colour share an atom; the lanes take the constraints of one colour side by side
// (c = first + lane, + 64, ...) and the colours follow in sequence.  The result therefore does not depend on which lane takes which
// constraint: bitwise repeatable, and a molecule's outputs do not depend on the rest of the batch or on its place in it.
//   SHAKE, constraint (i, j, d2):  s = y_i - y_j;  r = r_i - r_j;  e = d2 - s.s;  applied while |e| > tol d2:
//                                  g = e / ((2 (w_i + w_j)) (s.r));  y_i = fma(g w_i, r, y_i);  y_j = fma(-(g w_j), r, y_j)
//                                  (and D_i, D_j by the same two fmas)
//   PROJECT, constraint (i, j, d2): r = y_i - y_j;  q = r.(v_i - v_j);  applied while |q| dth > tol d2:
//                                  g = q / ((w_i + w_j) d2);  v_i = fma(-(g w_i), r, v_i);  v_j = fma(g w_j, r, v_j)
// A solve ends when a whole sweep applied no update or after max_iter sweeps (then the molecule is marked failed).  Breakdown guard:
// a SHAKE constraint with s.r <= NNHIP_MDC_GUARD d2 (the bond turned by almost a right angle within half a step), one with
// w_i + w_j <= 0 or d2 <= 0, and one whose atoms lie outside its molecule is skipped and marks the molecule failed: nothing divides
// by a vanishing number.  Every arithmetic operation is an explicit __fmaf_rn / __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn.
//
// One wave64 per molecule, four molecules per workgroup (as md_kinetic_kernel and relax.hip).  y, r, v and w of the molecule live
// in the wave's slice of LDS (13 floats per atom; NNHIP_MDC_MAX_ATOMS atoms), because constraints of successive colours touch each
// other's atoms.  Lanes of one wave exchange data through LDS only: its LDS instructions execute in program order, so what is
// needed between a colour and the next (and between an atom-wise and a constraint-wise pass) is that the COMPILER keeps the
// order and re-reads LDS -- a wavefront-scope release/acquire fence pair around a wave barrier (wave_sync).  No workgroup barrier:
// the four waves of a workgroup share nothing.  A molecule without constraints takes nnhip_md_step's chain (the same functions of
// csrc/md_chain.h, one atom per lane), bit for bit, without LDS or relative coordinates.  This kernel is for batches of molecules,
// not for one large system: a molecule is one wave's work.
#include "md_chain.h"

namespace {

constexpr int RT_THREADS = 256;
constexpr int RT_WAVES = RT_THREADS / 64;
constexpr int RT_MAX_BLOCKS = 2048;
constexpr int RT_MAX_ATOMS = NNHIP_MDC_MAX_ATOMS;

struct RattleArgs {
  const float* pos_in;
  float* vel;
  const float* force;
  const float* hk;
  const float* mass;
  const float* inv_mass;
  const float* sigma;
  const float* noise;
  const int32_t* mol_ptr;
  const int32_t* con_pair;
  const float* con_d2;
  const int32_t* mol_col_ptr;
  const int32_t* col_ptr;
  float* pos_out;
  float* ke_out;
  int32_t* n_failed;
  int32_t* n_sweeps;
  float dth, inv_dth, c1, tol;
  int flags, n_atoms, n_mol, n_col, n_con, max_iter;
};

__device__ __forceinline__ float dot3(const float* a, const float* b) {
  return __fmaf_rn(a[2], b[2], __fmaf_rn(a[1], b[1], __fmul_rn(a[0], b[0])));
}

// what one lane wrote to LDS before this point, every lane of the wave reads after it
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the constraint c of a molecule of n atoms: false when its table entries cannot be used
__device__ __forceinline__ bool constraint(const RattleArgs& g, int c, int n, int& i, int& j, float& d2) {
  i = g.con_pair[2 * (size_t)c];
  j = g.con_pair[2 * (size_t)c + 1];
  d2 = g.con_d2[c];
  return (unsigned)i < (unsigned)n && (unsigned)j < (unsigned)n && i != j && d2 > 0.f;
}

// colour k's constraints [c0, c1), kept inside the tables
__device__ __forceinline__ void colour_range(const RattleArgs& g, int k, int& c0, int& c1) {
  c0 = g.col_ptr[k];
  c1 = g.col_ptr[k + 1];
  c0 = c0 < 0 ? 0 : c0;
  c1 = c1 > g.n_con ? g.n_con : c1;
}

// One solve: Gauss-Seidel sweeps over the constraints of the colours [k0, k1) of a molecule of n atoms, the lanes side by side within
// a colour, until a whole sweep applied no update or max_iter sweeps are done (then the molecule is marked).  body(i, j, d2) treats
// one constraint and returns 1 (updated), 0 (within tolerance) or -1 (skipped by the guard: marks the molecule).  Returns the sweeps.
template <typename Body>
__device__ __forceinline__ int solve(const RattleArgs& g, int n, int k0, int k1, int lane, bool& fail, Body body) {
  int sweeps = 0;
  bool more = true;
  while (more && sweeps < g.max_iter) {
    bool updated = false;
    for (int k = k0; k < k1; ++k) {
      int c0, c1;
      colour_range(g, k, c0, c1);
      for (int c = c0 + lane; c < c1; c += 64) {
        int i, j;
        float d2;
        const int what = constraint(g, c, n, i, j, d2) ? body(i, j, d2) : -1;
        updated |= what > 0;
        fail |= what < 0;
      }
      wave_sync();
    }
    ++sweeps;
    more = __any(updated);
  }
  if (more) fail = true;
  return sweeps;
}

// SHAKE y [n,3] onto the constraints of the colours [k0, k1) with the directions of r; returns the number of sweeps
// every update is also added into disp [n,3] (zeroed by the caller): the displacement the solve applied, for the velocities
__device__ int shake(const RattleArgs& g, float* y, float* disp, const float* r, const float* w, int n, int k0, int k1, int lane,
                     bool& fail) {
  return solve(g, n, k0, k1, lane, fail, [&](int i, int j, float d2) -> int {
    float s[3], q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s[a] = __fsub_rn(y[3 * i + a], y[3 * j + a]);
      q[a] = __fsub_rn(r[3 * i + a], r[3 * j + a]);
    }
    const float e = __fsub_rn(d2, dot3(s, s));
    if (!(fabsf(e) > __fmul_rn(g.tol, d2))) return 0;
    const float sr = dot3(s, q);
    const float wi = w[i], wj = w[j];
    const float ws = __fadd_rn(wi, wj);
    if (!(sr > __fmul_rn(NNHIP_MDC_GUARD, d2)) || !(ws > 0.f)) return -1;
    const float gm = __fdiv_rn(e, __fmul_rn(__fmul_rn(2.f, ws), sr));
    const float gi = __fmul_rn(gm, wi), gj = -__fmul_rn(gm, wj);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      y[3 * i + a] = __fmaf_rn(gi, q[a], y[3 * i + a]);
      y[3 * j + a] = __fmaf_rn(gj, q[a], y[3 * j + a]);
      disp[3 * i + a] = __fmaf_rn(gi, q[a], disp[3 * i + a]);
      disp[3 * j + a] = __fmaf_rn(gj, q[a], disp[3 * j + a]);
    }
    return 1;
  });
}

// make v [n,3] tangent to the constraints of the colours [k0, k1) at the positions y; returns the number of sweeps
__device__ int project(const RattleArgs& g, const float* y, float* v, const float* w, int n, int k0, int k1, int lane, bool& fail) {
  return solve(g, n, k0, k1, lane, fail, [&](int i, int j, float d2) -> int {
    float q[3], u[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      q[a] = __fsub_rn(y[3 * i + a], y[3 * j + a]);
      u[a] = __fsub_rn(v[3 * i + a], v[3 * j + a]);
    }
    const float qu = dot3(q, u);
    if (!(__fmul_rn(fabsf(qu), g.dth) > __fmul_rn(g.tol, d2))) return 0;
    const float wi = w[i], wj = w[j];
    const float ws = __fadd_rn(wi, wj);
    if (!(ws > 0.f)) return -1;
    const float gm = __fdiv_rn(qu, __fmul_rn(ws, d2));
    const float gi = -__fmul_rn(gm, wi), gj = __fmul_rn(gm, wj);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[3 * i + a] = __fmaf_rn(gi, q[a], v[3 * i + a]);
      v[3 * j + a] = __fmaf_rn(gj, q[a], v[3 * j + a]);
    }
    return 1;
  });
}

// nnhip_md_step's chain for the atoms [a0, a1) of a molecule without constraints
__device__ void unconstrained(const RattleArgs& g, int a0, int a1, int lane) {
  const bool finish = g.flags & NNHIP_MD_FINISH, begin = g.flags & NNHIP_MD_BEGIN;
  for (int i = a0 + lane; i < a1; i += 64) {
    const size_t o = 3 * (size_t)i;
    if (g.flags & NNHIP_MDC_PROJECT) {
#pragma unroll
      for (int k = 0; k < 3; ++k) g.pos_out[o + k] = g.pos_in[o + k];
      continue;
    }
    const float hk = g.hk[i];
    float v[3] = {g.vel[o], g.vel[o + 1], g.vel[o + 2]};
    const float f[3] = {g.force[o], g.force[o + 1], g.force[o + 2]};
    if (finish) {
      md_chain::half_kick(v, hk, f);
      if (g.ke_out) g.ke_out[i] = md_chain::kinetic(v, g.mass[i]);
    }
    if (begin) {
      const float sigma = g.noise ? g.sigma[i] : 0.f;
      md_chain::begin<false>(v, hk, f, g.pos_in + o, g.pos_out + o, g.dth, sigma, g.noise ? g.noise + o : nullptr, g.c1, 1.f, 1.f);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) g.vel[o + k] = v[k];
  }
}

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

__global__ void __launch_bounds__(RT_THREADS)
md_step_constrained_kernel(RattleArgs g) {
  __shared__ float lds[RT_WAVES][13 * RT_MAX_ATOMS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* y = lds[wave];
  float* r = y + 3 * RT_MAX_ATOMS;
  float* v = r + 3 * RT_MAX_ATOMS;
  float* disp = v + 3 * RT_MAX_ATOMS;
  float* w = disp + 3 * RT_MAX_ATOMS;
  const bool finish = g.flags & NNHIP_MD_FINISH, begin = g.flags & NNHIP_MD_BEGIN, proj = g.flags & NNHIP_MDC_PROJECT;
  for (int b = blockIdx.x * RT_WAVES + wave; b < g.n_mol; b += gridDim.x * RT_WAVES) {   // (uniform over a wave)
    const int a0 = g.mol_ptr[b], a1 = g.mol_ptr[b + 1];
    const int k0 = g.mol_col_ptr[b], k1 = g.mol_col_ptr[b + 1];
    // offsets that leave the arrays: the molecule is not touched and counts as failed
    if (a0 < 0 || a1 < a0 || a1 > g.n_atoms || k0 < 0 || k1 < k0 || k1 > g.n_col) {
      if (lane == 0) {
        g.n_failed[b] += 1;
        g.n_sweeps[b] = 0;
      }
      continue;
    }
    const int n = a1 - a0;
    if (k1 == k0) {
      unconstrained(g, a0, a1, lane);
      if (lane == 0) g.n_sweeps[b] = 0;
      continue;
    }
    if (n > RT_MAX_ATOMS) {                    // (refused on the host; never reached through nnhip_md_step_constrained)
      if (lane == 0) {
        g.n_failed[b] += 1;
        g.n_sweeps[b] = 0;
      }
      continue;
    }
    bool fail = false;
    int sweeps = 0;
    const float x0[3] = {g.pos_in[3 * (size_t)a0], g.pos_in[3 * (size_t)a0 + 1], g.pos_in[3 * (size_t)a0 + 2]};
    wave_sync();                               // (the previous molecule of this wave is done with the LDS slice)
    for (int i = lane; i < n; i += 64) {
      const size_t o = 3 * (size_t)(a0 + i);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        y[3 * i + k] = __fsub_rn(g.pos_in[o + k], x0[k]);
        v[3 * i + k] = g.vel[o + k];
      }
      w[i] = g.inv_mass[a0 + i];
    }
    wave_sync();
    if (proj) {
      for (int i = lane; i < n; i += 64) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          r[3 * i + k] = y[3 * i + k];
          disp[3 * i + k] = 0.f;
        }
      }
      wave_sync();
      sweeps = imax(sweeps, shake(g, y, disp, r, w, n, k0, k1, lane, fail));
      sweeps = imax(sweeps, project(g, y, v, w, n, k0, k1, lane, fail));
    }
    if (finish) {
      for (int i = lane; i < n; i += 64) md_chain::half_kick(v + 3 * i, g.hk[a0 + i], g.force + 3 * (size_t)(a0 + i));
      wave_sync();
      sweeps = imax(sweeps, project(g, y, v, w, n, k0, k1, lane, fail));
      if (g.ke_out) {
        for (int i = lane; i < n; i += 64) g.ke_out[a0 + i] = md_chain::kinetic(v + 3 * i, g.mass[a0 + i]);
      }
    }
    if (begin) {
      for (int i = lane; i < n; i += 64) md_chain::half_kick(v + 3 * i, g.hk[a0 + i], g.force + 3 * (size_t)(a0 + i));
      wave_sync();
      sweeps = imax(sweeps, project(g, y, v, w, n, k0, k1, lane, fail));
      for (int half = 0; half < 2; ++half) {
        if (half == 1 && g.noise) {
          for (int i = lane; i < n; i += 64)
            md_chain::o_step(v + 3 * i, g.sigma[a0 + i], g.noise + 3 * (size_t)(a0 + i), g.c1);
          wave_sync();
          sweeps = imax(sweeps, project(g, y, v, w, n, k0, k1, lane, fail));
        }
        for (int i = lane; i < n; i += 64) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float yk = y[3 * i + k];
            r[3 * i + k] = yk;
            y[3 * i + k] = __fmaf_rn(g.dth, v[3 * i + k], yk);
            disp[3 * i + k] = 0.f;
          }
        }
        wave_sync();
        sweeps = imax(sweeps, shake(g, y, disp, r, w, n, k0, k1, lane, fail));
        for (int i = lane; i < n; i += 64) {
#pragma unroll
          for (int k = 0; k < 3; ++k) v[3 * i + k] = __fmaf_rn(disp[3 * i + k], g.inv_dth, v[3 * i + k]);
        }
        wave_sync();
        sweeps = imax(sweeps, project(g, y, v, w, n, k0, k1, lane, fail));
      }
    }
    for (int i = lane; i < n; i += 64) {
      const size_t o = 3 * (size_t)(a0 + i);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        g.vel[o + k] = v[3 * i + k];
        if (begin || proj) g.pos_out[o + k] = w[i] == 0.f ? g.pos_in[o + k] : __fadd_rn(x0[k], y[3 * i + k]);
      }
    }
    const bool failed = __any(fail);
    if (lane == 0) {
      if (failed) g.n_failed[b] += 1;
      g.n_sweeps[b] = sweeps;
    }
  }
}

// a [n + 1] offset table: starts at 0, never decreases, ends at `last`
inline bool offsets_ok(const int32_t* p, int n, int last) {
  if (p[0] != 0 || p[n] != last) return false;
  for (int k = 0; k < n; ++k)
    if (p[k + 1] < p[k]) return false;
  return true;
}

}  // namespace

extern "C" int nnhip_md_constrained_max_atoms(void) { return RT_MAX_ATOMS; }

extern "C" int nnhip_md_step_constrained(const float* pos_in, float* vel, const float* force, const float* hk, const float* mass,
                                         const float* inv_mass, const float* sigma, const float* noise, float dth, float inv_dth,
                                         float c1, int32_t flags, int32_t n_atoms, const int32_t* mol_ptr,
                                         const int32_t* mol_ptr_host, int32_t n_mol, const int32_t* con_pair, const float* con_d2,
                                         const int32_t* mol_col_ptr, const int32_t* mol_col_ptr_host, const int32_t* col_ptr,
                                         const int32_t* col_ptr_host, int32_t n_col, float tol, int32_t max_iter, float* pos_out,
                                         float* ke_out, int32_t* n_failed, int32_t* n_sweeps, void* stream) {
  const bool flags_ok = flags == NNHIP_MDC_PROJECT || (flags >= 1 && flags <= (NNHIP_MD_FINISH | NNHIP_MD_BEGIN));
  if (n_atoms < 0 || n_mol < 0 || n_col < 0 || !flags_ok) {
    nnhip_set_error("nnhip_md_step_constrained: bad arguments (n_atoms %d, n_mol %d, n_col %d, flags %d: bit 0 = finish, bit 1 = "
                    "begin, or NNHIP_MDC_PROJECT alone)", n_atoms, n_mol, n_col, flags);
    return NNHIP_E_INVALID;
  }
  if (!(tol > 0.f) || max_iter < 1) {
    nnhip_set_error("nnhip_md_step_constrained: tol > 0 and max_iter >= 1 expected (got %g, %d)", (double)tol, max_iter);
    return NNHIP_E_INVALID;
  }
  if ((sigma == nullptr) != (noise == nullptr)) {
    nnhip_set_error("nnhip_md_step_constrained: sigma and noise come together (both given or both null)");
    return NNHIP_E_INVALID;
  }
  if (n_atoms == 0) return NNHIP_OK;
  const bool project = flags == NNHIP_MDC_PROJECT, moves = project || (flags & NNHIP_MD_BEGIN);
  if (!pos_in || !vel || !inv_mass || (!project && (!force || !hk)) || (moves && !pos_out) ||
      (ke_out && (!mass || !(flags & NNHIP_MD_FINISH) || project))) {
    nnhip_set_error("nnhip_md_step_constrained: bad arguments (pos_in, vel and inv_mass always; force and hk unless project; pos_out "
                    "with begin or project; ke_out needs mass and finish)");
    return NNHIP_E_INVALID;
  }
  if (!mol_ptr || !mol_ptr_host || !mol_col_ptr || !mol_col_ptr_host || !col_ptr || !col_ptr_host || !n_failed || !n_sweeps) {
    nnhip_set_error("nnhip_md_step_constrained: null table (mol_ptr, mol_col_ptr, col_ptr and their host copies, n_failed and "
                    "n_sweeps are mandatory)");
    return NNHIP_E_INVALID;
  }
  if (n_mol == 0 || !offsets_ok(mol_ptr_host, n_mol, n_atoms) || !offsets_ok(mol_col_ptr_host, n_mol, n_col) ||
      col_ptr_host[0] != 0) {
    nnhip_set_error("nnhip_md_step_constrained: unsorted tables (mol_ptr_host: 0 .. n_atoms = %d and mol_col_ptr_host: 0 .. n_col = "
                    "%d, neither decreasing, over n_mol = %d >= 1 molecules; col_ptr_host starts at 0)", n_atoms, n_col, n_mol);
    return NNHIP_E_INVALID;
  }
  for (int k = 0; k < n_col; ++k) {
    if (col_ptr_host[k + 1] < col_ptr_host[k]) {
      nnhip_set_error("nnhip_md_step_constrained: unsorted tables (col_ptr_host decreases at colour %d)", k);
      return NNHIP_E_INVALID;
    }
  }
  const int n_con = col_ptr_host[n_col];
  if (n_con > 0 && (!con_pair || !con_d2)) {
    nnhip_set_error("nnhip_md_step_constrained: null table (con_pair and con_d2 of %d constraints)", n_con);
    return NNHIP_E_INVALID;
  }
  for (int b = 0; b < n_mol; ++b) {
    const int n = mol_ptr_host[b + 1] - mol_ptr_host[b];
    if (mol_col_ptr_host[b + 1] > mol_col_ptr_host[b] && n > RT_MAX_ATOMS) {
      nnhip_set_error("nnhip_md_step_constrained: molecule %d has constraints and %d atoms, above the %d the LDS form takes "
                      "(nnhip_md_constrained_max_atoms)", b, n, RT_MAX_ATOMS);
      return NNHIP_E_INVALID;
    }
  }
  if (moves && overlap(pos_in, pos_out, 3 * (size_t)n_atoms)) {
    nnhip_set_error("nnhip_md_step_constrained: pos_out may not alias pos_in (a forward call that has to be repeated reads pos_in "
                    "again)");
    return NNHIP_E_INVALID;
  }
  RattleArgs g;
  g.pos_in = pos_in;
  g.vel = vel;
  g.force = force;
  g.hk = hk;
  g.mass = mass;
  g.inv_mass = inv_mass;
  g.sigma = sigma;
  g.noise = noise;
  g.mol_ptr = mol_ptr;
  g.con_pair = con_pair;
  g.con_d2 = con_d2;
  g.mol_col_ptr = mol_col_ptr;
  g.col_ptr = col_ptr;
  g.pos_out = pos_out;
  g.ke_out = ke_out;
  g.n_failed = n_failed;
  g.n_sweeps = n_sweeps;
  g.dth = dth;
  g.inv_dth = inv_dth;
  g.c1 = c1;
  g.tol = tol;
  g.flags = flags;
  g.n_atoms = n_atoms;
  g.n_mol = n_mol;
  g.n_col = n_col;
  g.n_con = n_con;
  g.max_iter = max_iter;
  int blocks = (n_mol + RT_WAVES - 1) / RT_WAVES;
  blocks = blocks > RT_MAX_BLOCKS ? RT_MAX_BLOCKS : blocks;
  md_step_constrained_kernel<<<blocks, RT_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
