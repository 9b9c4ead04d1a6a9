// Bias potentials on collective variables (gfx950, fp32): one launch per MD step turns the model's forces into the forces of the
// biased potential -- harmonic restraints (umbrella windows) plus the Gaussian hills the walkers of a group share (multiple-walker,
// well-tempered metadynamics) -- and, at a deposit step, writes one new hill per walker.  The driver is
// newtonnet_amd/metadynamics.py:  model(pos) -> bias_step -> md_step.  include/newtonnet_hip.h spells the contract out.
//
// One workgroup of four waves per molecule, the molecules of a batch by a grid-stride loop.  Every thread reads the molecule's two
// variable definitions and forms the variables and their <= 8 gradient rows itself (<= 8 atoms: the same answer in every thread, no
// communication, as remd.hip does for its ladder checks).  Thread t then adds the hills t, t + 256, ... of the molecule's group in
// ascending order -- consecutive threads read consecutive 16-byte rows -- and the three partial sums (V, G_0, G_1) go through a
// fixed tree: a butterfly over the wave (an fp32 add is commutative, so every lane ends with the same bits), one LDS word per wave
// and sum, ONE barrier, and every thread adds the four words in wave order.  All threads then walk the molecule's atoms for the
// copy-and-add.  A second barrier closes the loop body (the LDS words belong to the next molecule from there).  Every barrier is
// reached by every thread: a skipped molecule skips the work, never the barrier.  No float atomics, no communication between
// workgroups.  The positions are taken as stored: unwrapped, no minimum image.
//
// A deposit writes row n_deposits W + j of the group's hill list; the sums read rows below n_deposits W only, and the count is a host
// integer: no race, no counter on the device.
#include "common.h"

namespace {

constexpr int BIAS_THREADS = NNHIP_BIAS_THREADS;
constexpr int BIAS_WAVES = BIAS_THREADS / 64;
constexpr int BIAS_MAX_BLOCKS = 4096;
constexpr float TWO_PI_F = 6.28318530717958647692f;

struct BiasArgs {
  const float* pos;
  const float* force_in;
  const int32_t* mol_ptr;
  const int32_t* group_ptr;
  const int32_t* cv_def;
  const float* restraint;
  const float* hill_par;
  float* hills;
  float* force_out;
  float* cv_out;
  float* bias_out;
  int32_t* status_out;
  int capacity, n_deposits, deposit, n_groups, n_mol, n_atoms;
};

struct Vec3 {
  float x, y, z;
};

__device__ __forceinline__ Vec3 load3(const float* p, size_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ Vec3 sub3(Vec3 a, Vec3 b) { return {__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z)}; }
__device__ __forceinline__ Vec3 add3(Vec3 a, Vec3 b) { return {__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z)}; }
__device__ __forceinline__ Vec3 neg3(Vec3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ Vec3 scale3(float c, Vec3 a) { return {__fmul_rn(c, a.x), __fmul_rn(c, a.y), __fmul_rn(c, a.z)}; }
__device__ __forceinline__ float dot3(Vec3 a, Vec3 b) { return __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, __fmul_rn(a.x, b.x))); }
// a x b, two roundings per component: the second product, then the fma
__device__ __forceinline__ Vec3 cross3(Vec3 a, Vec3 b) {
  return {__fmaf_rn(a.y, b.z, -__fmul_rn(a.z, b.y)), __fmaf_rn(a.z, b.x, -__fmul_rn(a.x, b.z)),
          __fmaf_rn(a.x, b.y, -__fmul_rn(a.y, b.x))};
}
__device__ __forceinline__ bool finite3(Vec3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// one collective variable: its value, the local indices of its atoms (-1: none) and its gradient rows
struct Cv {
  float s;
  float period;      // fl32(2 pi) for a torsion, 0 otherwise
  int idx[4];
  Vec3 g[4];
  bool degenerate;
};

__device__ __forceinline__ Cv make_cv(int kind, const int32_t* def, const float* pos, size_t base) {
  Cv cv;
  cv.s = 0.f;
  cv.period = 0.f;
  cv.degenerate = false;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    cv.idx[r] = -1;
    cv.g[r] = {0.f, 0.f, 0.f};
  }
  if (kind == NNHIP_BIAS_DISTANCE) {
    const Vec3 r = sub3(load3(pos, base + def[1]), load3(pos, base + def[0]));
    const float d2 = dot3(r, r);
    cv.s = __fsqrt_rn(d2);
    const Vec3 gj = scale3(__fdiv_rn(1.f, cv.s), r);
    cv.idx[0] = def[0];
    cv.idx[1] = def[1];
    cv.g[0] = neg3(gj);
    cv.g[1] = gj;
    cv.degenerate = !(d2 > 0.f) || !finite3(gj);
  } else if (kind == NNHIP_BIAS_ANGLE) {
    const Vec3 xj = load3(pos, base + def[1]);
    const Vec3 a = sub3(load3(pos, base + def[0]), xj), b = sub3(load3(pos, base + def[2]), xj);
    const Vec3 c = cross3(a, b);
    const float c2 = dot3(c, c);
    const float cn = __fsqrt_rn(c2);
    cv.s = atan2f(cn, dot3(a, b));
    const Vec3 gi = scale3(__fdiv_rn(1.f, __fmul_rn(dot3(a, a), cn)), cross3(a, c));
    const Vec3 gk = scale3(__fdiv_rn(1.f, __fmul_rn(dot3(b, b), cn)), cross3(c, b));
    cv.idx[0] = def[0];
    cv.idx[1] = def[1];
    cv.idx[2] = def[2];
    cv.g[0] = gi;
    cv.g[1] = neg3(add3(gi, gk));
    cv.g[2] = gk;
    cv.degenerate = !(c2 > 0.f) || !finite3(gi) || !finite3(gk);
  } else if (kind == NNHIP_BIAS_TORSION) {
    const Vec3 xi = load3(pos, base + def[0]), xj = load3(pos, base + def[1]), xk = load3(pos, base + def[2]),
               xl = load3(pos, base + def[3]);
    const Vec3 b1 = sub3(xj, xi), b2 = sub3(xk, xj), b3 = sub3(xl, xk);
    const Vec3 n1 = cross3(b1, b2), n2 = cross3(b2, b3);
    const float b22 = dot3(b2, b2);
    const float b2n = __fsqrt_rn(b22);
    cv.s = atan2f(__fmul_rn(b2n, dot3(b1, n2)), dot3(n1, n2));
    cv.period = TWO_PI_F;
    const float n12 = dot3(n1, n1), n22 = dot3(n2, n2);
    const Vec3 gi = scale3(-__fdiv_rn(b2n, n12), n1);
    const Vec3 gl = scale3(__fdiv_rn(b2n, n22), n2);
    const float p = __fdiv_rn(dot3(b1, b2), b22), q = __fdiv_rn(dot3(b3, b2), b22);
    const Vec3 t = sub3(scale3(q, gl), scale3(p, gi));
    cv.idx[0] = def[0];
    cv.idx[1] = def[1];
    cv.idx[2] = def[2];
    cv.idx[3] = def[3];
    cv.g[0] = gi;
    cv.g[1] = sub3(t, gi);
    cv.g[2] = neg3(add3(t, gl));
    cv.g[3] = gl;
    cv.degenerate = !(n12 > 0.f) || !(n22 > 0.f) || !finite3(gi) || !finite3(gl) || !finite3(cv.g[1]) || !finite3(cv.g[2]);
  }
  if (cv.degenerate) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {                 // no force of it, whatever its coefficient turns out to be
      cv.idx[r] = -1;
      cv.g[r] = {0.f, 0.f, 0.f};
    }
    if (!isfinite(cv.s)) cv.s = 0.f;
  }
  return cv;
}

// delta - P rint(delta / P) with inv = fl32(1 / P); P == 0: delta as it is
__device__ __forceinline__ float wrap(float delta, float period, float inv) {
  return period > 0.f ? __fmaf_rn(-period, rintf(__fmul_rn(delta, inv)), delta) : delta;
}

struct HillSum {
  float v, g0, g1;
};

// The hills rows[0 .. n_hills - 1] at the point (s0, s1), for the whole workgroup: every thread returns the same three sums.
// Contains ONE barrier, which every thread of the workgroup must reach; the caller owns the barrier that lets `red` be reused.
__device__ __forceinline__ HillSum block_hill_sum(const float4* rows, int n_hills, float s0, float s1, float is0, float is1, float p0,
                                                  float p1, float (*red)[BIAS_WAVES]) {
  const int t = threadIdx.x;
  const float ip0 = p0 > 0.f ? __fdiv_rn(1.f, p0) : 0.f, ip1 = p1 > 0.f ? __fdiv_rn(1.f, p1) : 0.f;
  float v = 0.f, g0 = 0.f, g1 = 0.f;
  for (int h = t; h < n_hills; h += BIAS_THREADS) {
    const float4 row = rows[h];
    const float d0 = wrap(__fsub_rn(s0, row.x), p0, ip0), d1 = wrap(__fsub_rn(s1, row.y), p1, ip1);
    const float a0 = __fmul_rn(d0, is0), a1 = __fmul_rn(d1, is1);
    const float e = __fmaf_rn(a1, d1, __fmul_rn(a0, d0));
    const float term = __fmul_rn(row.z, expf(__fmul_rn(-0.5f, e)));
    v = __fadd_rn(v, term);
    g0 = __fmaf_rn(term, a0, g0);
    g1 = __fmaf_rn(term, a1, g1);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    v = __fadd_rn(v, __shfl_xor(v, m, 64));
    g0 = __fadd_rn(g0, __shfl_xor(g0, m, 64));
    g1 = __fadd_rn(g1, __shfl_xor(g1, m, 64));
  }
  if ((t & 63) == 0) {
    red[0][t >> 6] = v;
    red[1][t >> 6] = g0;
    red[2][t >> 6] = g1;
  }
  __syncthreads();
  HillSum out;
  out.v = __fadd_rn(__fadd_rn(red[0][0], red[0][1]), __fadd_rn(red[0][2], red[0][3]));
  out.g0 = __fadd_rn(__fadd_rn(red[1][0], red[1][1]), __fadd_rn(red[1][2], red[1][3]));
  out.g1 = __fadd_rn(__fadd_rn(red[2][0], red[2][1]), __fadd_rn(red[2][2], red[2][3]));
  return out;
}

__device__ __forceinline__ int arity(int kind) { return kind == 0 ? 0 : kind + 1; }      // distance 2, angle 3, torsion 4

__global__ void __launch_bounds__(BIAS_THREADS)
bias_step_kernel(BiasArgs g) {
  __shared__ float s_red[3][BIAS_WAVES];
  const int t = threadIdx.x;
  for (int b = blockIdx.x; b < g.n_mol; b += gridDim.x) {         // (uniform over the workgroup)
    // ---- the molecule as every thread sees it
    const int a0 = g.mol_ptr[b], a1 = g.mol_ptr[b + 1];
    const int n = a1 - a0;
    const bool inside = a0 >= 0 && n >= 0 && a1 <= g.n_atoms;
    // its group: the last gi with group_ptr[gi] <= b
    int lo = 0, hi = g.n_groups;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (g.group_ptr[mid] <= b) lo = mid; else hi = mid;
    }
    const int grp = lo;
    const int m0 = g.group_ptr[grp], m1 = g.group_ptr[grp + 1];
    const int W = m1 - m0, j = b - m0;
    const long n_hills = (long)g.n_deposits * W;
    bool bad = !(m0 <= b && b < m1) || n_hills + (g.deposit ? W : 0) > (long)g.capacity;
    int kind[NNHIP_BIAS_MAX_CVS] = {0, 0};
    const int32_t* def = g.cv_def + (size_t)b * (NNHIP_BIAS_MAX_CVS * 5);
    if (inside && !bad) {
#pragma unroll
      for (int d = 0; d < NNHIP_BIAS_MAX_CVS; ++d) {
        kind[d] = def[5 * d];
        if (kind[d] < 0 || kind[d] > NNHIP_BIAS_TORSION) {
          bad = true;
          kind[d] = 0;
        }
        for (int r = 0; r < arity(kind[d]); ++r) {
          const int i = def[5 * d + 1 + r];
          bad = bad || i < 0 || i >= n;
        }
      }
    }
    const bool work = inside && !bad;
    Cv cv0 = make_cv(work ? kind[0] : 0, def + 1, g.pos, (size_t)(inside ? a0 : 0));
    Cv cv1 = make_cv(work ? kind[1] : 0, def + 6, g.pos, (size_t)(inside ? a0 : 0));
    // ---- the hills of the group (a skipped molecule sums none, and reaches the barrier inside)
    const float* par = g.hill_par + 4 * (size_t)grp;
    const float4* rows = reinterpret_cast<const float4*>(g.hills) + (size_t)grp * (size_t)g.capacity;
    const HillSum sum = block_hill_sum(rows, work ? (int)n_hills : 0, cv0.s, cv1.s, work ? par[0] : 0.f, work ? par[1] : 0.f,
                                       cv0.period, cv1.period, s_red);
    if (inside) {
      // ---- the restraints and the chain rule
      float c0 = 0.f, c1 = 0.f, u = 0.f;
      if (work) {
        const float* res = g.restraint + (size_t)b * (NNHIP_BIAS_MAX_CVS * 2);
        const float r0 = wrap(__fsub_rn(cv0.s, res[1]), cv0.period, cv0.period > 0.f ? __fdiv_rn(1.f, cv0.period) : 0.f);
        const float r1 = wrap(__fsub_rn(cv1.s, res[3]), cv1.period, cv1.period > 0.f ? __fdiv_rn(1.f, cv1.period) : 0.f);
        const float k0 = kind[0] ? __fmul_rn(res[0], r0) : 0.f, k1 = kind[1] ? __fmul_rn(res[2], r1) : 0.f;
        u = __fadd_rn(__fmul_rn(__fmul_rn(0.5f, k0), r0), __fmul_rn(__fmul_rn(0.5f, k1), r1));
        c0 = __fsub_rn(k0, sum.g0);
        c1 = __fsub_rn(k1, sum.g1);
      }
      for (int i = t; i < n; i += BIAS_THREADS) {
        const size_t row = (size_t)a0 + (size_t)i;
        float bx = 0.f, by = 0.f, bz = 0.f;
        bool has = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (cv0.idx[r] == i) {
            bx = __fmul_rn(c0, cv0.g[r].x);
            by = __fmul_rn(c0, cv0.g[r].y);
            bz = __fmul_rn(c0, cv0.g[r].z);
            has = true;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (cv1.idx[r] == i) {
            bx = has ? __fmaf_rn(c1, cv1.g[r].x, bx) : __fmul_rn(c1, cv1.g[r].x);
            by = has ? __fmaf_rn(c1, cv1.g[r].y, by) : __fmul_rn(c1, cv1.g[r].y);
            bz = has ? __fmaf_rn(c1, cv1.g[r].z, bz) : __fmul_rn(c1, cv1.g[r].z);
            has = true;
          }
        }
        const float fx = g.force_in[3 * row], fy = g.force_in[3 * row + 1], fz = g.force_in[3 * row + 2];
        g.force_out[3 * row] = bx == 0.f ? fx : __fsub_rn(fx, bx);
        g.force_out[3 * row + 1] = by == 0.f ? fy : __fsub_rn(fy, by);
        g.force_out[3 * row + 2] = bz == 0.f ? fz : __fsub_rn(fz, bz);
      }
      if (t == 0) {
        g.cv_out[2 * (size_t)b] = work ? cv0.s : 0.f;
        g.cv_out[2 * (size_t)b + 1] = work ? cv1.s : 0.f;
        g.bias_out[2 * (size_t)b] = work ? sum.v : 0.f;
        g.bias_out[2 * (size_t)b + 1] = u;
        g.status_out[b] = bad ? NNHIP_BIAS_STATUS_INVALID : (cv0.degenerate ? 1 : 0) | (cv1.degenerate ? 2 : 0);
        if (work && g.deposit) {
          const float height = __fmul_rn(par[2], expf(-__fmul_rn(sum.v, par[3])));
          float4* out = reinterpret_cast<float4*>(g.hills) + (size_t)grp * (size_t)g.capacity + (size_t)n_hills + (size_t)j;
          *out = make_float4(cv0.s, cv1.s, height, 0.f);
        }
      }
    }
    __syncthreads();                                       // s_red belongs to the next molecule from here
  }
}

struct EvalArgs {
  const float* rows;
  const float* par;
  const float* points;
  float* v_out;
  float p0, p1;
  int n_hills, n_points;
};

__global__ void __launch_bounds__(BIAS_THREADS)
bias_eval_kernel(EvalArgs g) {
  __shared__ float s_red[3][BIAS_WAVES];
  for (int m = blockIdx.x; m < g.n_points; m += gridDim.x) {
    const HillSum sum = block_hill_sum(reinterpret_cast<const float4*>(g.rows), g.n_hills, g.points[2 * (size_t)m],
                                       g.points[2 * (size_t)m + 1], g.par[0], g.par[1], g.p0, g.p1, s_red);
    if (threadIdx.x == 0) g.v_out[m] = sum.v;
    __syncthreads();
  }
}

}  // namespace

extern "C" int nnhip_bias_step(const float* pos, const float* force_in, const int32_t* mol_ptr, const int32_t* mol_ptr_host,
                               const int32_t* group_ptr, const int32_t* group_ptr_host, const int32_t* cv_def, const float* restraint,
                               const float* hill_par, float* hills, int32_t capacity, int32_t n_deposits, int32_t flags,
                               int32_t n_groups, int32_t n_mol, int32_t n_atoms, float* force_out, float* cv_out, float* bias_out,
                               int32_t* status_out, void* stream) {
  if (n_groups < 0 || n_mol < 0 || n_atoms < 0 || capacity < 0) {
    nnhip_set_error("nnhip_bias_step: bad arguments (n_groups %d, n_mol %d, n_atoms %d, capacity %d)", n_groups, n_mol, n_atoms,
                    capacity);
    return NNHIP_E_INVALID;
  }
  if (n_deposits < 0) {
    nnhip_set_error("nnhip_bias_step: n_deposits %d (>= 0 expected)", n_deposits);
    return NNHIP_E_INVALID;
  }
  if (flags & ~NNHIP_BIAS_DEPOSIT) {
    nnhip_set_error("nnhip_bias_step: unknown flag bits %d (NNHIP_BIAS_DEPOSIT = %d is the only one)", flags, NNHIP_BIAS_DEPOSIT);
    return NNHIP_E_INVALID;
  }
  if (n_mol == 0 && n_groups == 0) return NNHIP_OK;
  if (!pos || !force_in || !mol_ptr || !mol_ptr_host || !group_ptr || !group_ptr_host || !cv_def || !restraint || !hill_par || !hills ||
      !force_out || !cv_out || !bias_out || !status_out) {
    nnhip_set_error("nnhip_bias_step: null pointer (every pointer but stream is mandatory)");
    return NNHIP_E_INVALID;
  }
  const size_t n3 = 3 * (size_t)n_atoms;
  if (overlap(force_out, force_in, n3) || overlap(force_out, pos, n3)) {
    nnhip_set_error("nnhip_bias_step: force_out may not overlap force_in or pos");
    return NNHIP_E_INVALID;
  }
  if ((uintptr_t)hills % 16 != 0) {
    nnhip_set_error("nnhip_bias_step: hills must be 16-byte aligned");
    return NNHIP_E_INVALID;
  }
  if (group_ptr_host[0] != 0 || group_ptr_host[n_groups] != n_mol) {
    nnhip_set_error("nnhip_bias_step: group_ptr must run from 0 to n_mol = %d (got %d .. %d)", n_mol, group_ptr_host[0],
                    group_ptr_host[n_groups]);
    return NNHIP_E_INVALID;
  }
  if (mol_ptr_host[0] != 0 || mol_ptr_host[n_mol] != n_atoms) {
    nnhip_set_error("nnhip_bias_step: mol_ptr must run from 0 to n_atoms = %d (got %d .. %d)", n_atoms, mol_ptr_host[0],
                    mol_ptr_host[n_mol]);
    return NNHIP_E_INVALID;
  }
  const int deposit = (flags & NNHIP_BIAS_DEPOSIT) ? 1 : 0;
  for (int l = 0; l < n_groups; ++l) {
    const int m0 = group_ptr_host[l];
    const long W = (long)group_ptr_host[l + 1] - m0;
    if (W < 1 || m0 < 0 || m0 + W > n_mol) {
      nnhip_set_error("nnhip_bias_step: group_ptr must run from 0 to n_mol in groups of >= 1 walkers (group %d: molecules %d .. %ld "
                      "of %d)", l, m0, m0 + W - 1, n_mol);
      return NNHIP_E_INVALID;
    }
    const long n = (long)mol_ptr_host[m0 + 1] - mol_ptr_host[m0];
    for (int s = 0; s < W; ++s) {
      const long ns = (long)mol_ptr_host[m0 + s + 1] - mol_ptr_host[m0 + s];
      if (ns != n || ns < 0) {
        nnhip_set_error("nnhip_bias_step: group %d: walker %d has %ld atoms, walker 0 has %ld (equal counts >= 0 expected)", l, s, ns,
                        n);
        return NNHIP_E_INVALID;
      }
    }
    if (((long)n_deposits + deposit) * W > (long)capacity) {
      nnhip_set_error("nnhip_bias_step: group %d: %d deposits%s of %ld walkers leave the capacity of %d hills", l, n_deposits,
                      deposit ? " and this one" : "", W, capacity);
      return NNHIP_E_INVALID;
    }
  }
  BiasArgs g;
  g.pos = pos;
  g.force_in = force_in;
  g.mol_ptr = mol_ptr;
  g.group_ptr = group_ptr;
  g.cv_def = cv_def;
  g.restraint = restraint;
  g.hill_par = hill_par;
  g.hills = hills;
  g.force_out = force_out;
  g.cv_out = cv_out;
  g.bias_out = bias_out;
  g.status_out = status_out;
  g.capacity = capacity;
  g.n_deposits = n_deposits;
  g.deposit = deposit;
  g.n_groups = n_groups;
  g.n_mol = n_mol;
  g.n_atoms = n_atoms;
  const int blocks = n_mol > BIAS_MAX_BLOCKS ? BIAS_MAX_BLOCKS : n_mol;
  bias_step_kernel<<<blocks, BIAS_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}

extern "C" int nnhip_bias_eval(const float* hills, const float* hill_par, const float* points, float period0, float period1,
                               int32_t group, int32_t capacity, int32_t n_hills, int32_t n_points, int32_t n_groups, float* v_out,
                               void* stream) {
  if (n_groups < 0 || capacity < 0 || n_hills < 0 || n_points < 0 || group < 0 || group >= n_groups || n_hills > capacity) {
    nnhip_set_error("nnhip_bias_eval: bad arguments (group %d of %d, n_hills %d of capacity %d, n_points %d)", group, n_groups,
                    n_hills, capacity, n_points);
    return NNHIP_E_INVALID;
  }
  if (!(period0 >= 0.f && period0 < 3.0e38f) || !(period1 >= 0.f && period1 < 3.0e38f)) {
    nnhip_set_error("nnhip_bias_eval: periods must be finite and >= 0 (0 = not periodic)");
    return NNHIP_E_INVALID;
  }
  if (!hills || !hill_par || !points || !v_out) {
    nnhip_set_error("nnhip_bias_eval: null pointer (hills, hill_par, points and v_out are mandatory)");
    return NNHIP_E_INVALID;
  }
  if ((uintptr_t)hills % 16 != 0) {
    nnhip_set_error("nnhip_bias_eval: hills must be 16-byte aligned");
    return NNHIP_E_INVALID;
  }
  if (n_points == 0) return NNHIP_OK;
  EvalArgs g;
  g.rows = hills + 4 * (size_t)group * (size_t)capacity;
  g.par = hill_par + 4 * (size_t)group;
  g.points = points;
  g.v_out = v_out;
  g.p0 = period0;
  g.p1 = period1;
  g.n_hills = n_hills;
  g.n_points = n_points;
  const int blocks = n_points > BIAS_MAX_BLOCKS ? BIAS_MAX_BLOCKS : n_points;
  bias_eval_kernel<<<blocks, BIAS_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
