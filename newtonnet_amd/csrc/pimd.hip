// Path-integral molecular dynamics on the device (gfx950, fp32): one launch per step advances every ring polymer of a batch in
// its normal-mode coordinates.
//
// A system g is a run of P consecutive molecules of equal atom count n, its SLOTS (the layout of csrc/remd.hip).  In the force and
// position buffers the model sees, slot s holds bead s; in the state arrays u (mode positions) and w (mode velocities) slot k holds
// ring-polymer normal mode k.  The scheme is BAOAB with the A step exact for the free ring polymer (Ceriotti et al. 2010), the O
// step the PILE thermostat; a step of the driver (newtonnet_amd/pimd.py) is  model(beads) -> pimd_step(finish | begin).  Per atom i,
// mode k and coordinate, every operation in fp32 with one explicit rounding (tests/pimd_ref.py restates it in fp64 with one 2^-24
// per operation):
//   f_k = C[k][0] F_0;  f_k = fma(C[k][s], F_s, f_k)  s = 1 .. P-1 ascending              the mode force, once per launch
//   finish:  w = fma(hk, f_k, w)
//            est[row] = (md_chain::kinetic(w, m),               (m half_w2) fma(uz,uz,fma(uy,uy,ux ux)),
//                        k > 0 ? fma(uz,fz,fma(uy,fy,ux fx)) : 0,  0)                     only when est_out != NULL
//   begin:   w = fma(hk, f_k, w)
//            A:  u' = fma(b, w, a u);  w' = fma(d, u, a w)                                 both from the old u, w
//            O:  w = fma(sigma, xi, c1 w)                                                  skipped entirely when noise == NULL
//            A again;  store u, w
//            x_s = C[0][s] u_0;  x_s = fma(C[k][s], u_k, x_s)  k = 1 .. P-1 ascending      -> pos_out, bead s
// With P = 1 (C = [1], a = 1, b = dth, d = 0) this is md_step_kernel's chain.  The kernel evaluates no transcendental: C and the
// per-mode table (a, b, d, c1, half_w2) are formed in fp64 on the host and rounded once.
//
// One workgroup of 256 threads per (system, tile of atoms); a tile holds NNHIP_PIMD_THREADS / P atoms (rounded down), so that every
// (slot, atom) of it has a thread.  LDS holds C (rows padded to an odd stride: the forward sums read a column of it across the
// wave), the tile's force rows and afterwards its updated u rows.  Thread (k, atom) does the forward sums and the mode update;
// after a barrier thread (s, atom) does the back-transform.  Every barrier is reached by all threads: a system or a tile that is
// skipped skips the work, never the barrier.  No float atomics, no communication between workgroups: a system's outputs depend on
// nothing else in the batch.
#include "md_chain.h"

namespace {

constexpr int PIMD_THREADS = NNHIP_PIMD_THREADS;
constexpr int PIMD_MAX_TILE_BLOCKS = 4096;       // gridDim.y; more tiles per system by a stride loop

struct PimdArgs {
  float* u;
  float* w;
  const float* force;
  const float* ctab;
  const float* mode_tab;
  const float* hk;
  const float* mass;
  const float* sigma;
  const float* noise;
  const int32_t* mol_ptr;
  float* pos_out;
  float* est_out;
  int flags, n_beads, n_systems, n_atoms;
};

__global__ void __launch_bounds__(PIMD_THREADS)
pimd_step_kernel(PimdArgs g) {
  __shared__ float s_c[NNHIP_PIMD_MAX_BEADS * (NNHIP_PIMD_MAX_BEADS + 1)];
  __shared__ float s_f[PIMD_THREADS * 3];
  __shared__ float s_u[PIMD_THREADS * 3];
  const int P = g.n_beads, ld = P | 1, cap = PIMD_THREADS / P;
  const int t = threadIdx.x;
  const int k = t / cap, a = t - k * cap;           // this thread's slot (a mode, then a bead) and atom of the tile
  const bool finish = g.flags & NNHIP_PIMD_FINISH, begin = g.flags & NNHIP_PIMD_BEGIN;
  for (int j = t; j < P * P; j += PIMD_THREADS) s_c[(j / P) * ld + (j % P)] = g.ctab[j];
  __syncthreads();
  for (int sys = blockIdx.x; sys < g.n_systems; sys += gridDim.x) {              // (uniform over the workgroup)
    const long base = g.mol_ptr[(size_t)sys * P];
    const long n = g.mol_ptr[(size_t)sys * P + 1] - base;
    // a system whose device offsets leave the arrays is not touched
    const bool inside = base >= 0 && n >= 0 && base + (long)P * n <= (long)g.n_atoms;
    const long n_tiles = inside ? (n + cap - 1) / cap : 0;
    for (long tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {            // (uniform over the workgroup)
      const long i = tile * cap + a;                                             // atom of the system
      const bool active = k < P && i < n;
      const size_t row = (size_t)(base + (long)k * n + i);                       // only used when active
      const size_t o = 3 * row;
      if (active) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s_f[(k * cap + a) * 3 + c] = g.force[o + c];
      }
      __syncthreads();
      if (active) {
        const float* crow = s_c + k * ld;
        float f[3], uu[3], ww[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = __fmul_rn(crow[0], s_f[a * 3 + c]);
        for (int s = 1; s < P; ++s) {
          const float cks = crow[s];
#pragma unroll
          for (int c = 0; c < 3; ++c) f[c] = __fmaf_rn(cks, s_f[(s * cap + a) * 3 + c], f[c]);
        }
        const float hk = g.hk[row];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          uu[c] = g.u[o + c];
          ww[c] = g.w[o + c];
        }
        const float* mt = g.mode_tab + 5 * ((size_t)sys * P + k);
        if (finish) {
#pragma unroll
          for (int c = 0; c < 3; ++c) ww[c] = __fmaf_rn(hk, f[c], ww[c]);
          if (g.est_out) {
            const float m = g.mass[row];
            const float spr = __fmaf_rn(uu[2], uu[2], __fmaf_rn(uu[1], uu[1], __fmul_rn(uu[0], uu[0])));
            const float vir = k > 0 ? __fmaf_rn(uu[2], f[2], __fmaf_rn(uu[1], f[1], __fmul_rn(uu[0], f[0]))) : 0.f;
            float* e = g.est_out + 4 * row;
            e[0] = md_chain::kinetic(ww, m);
            e[1] = __fmul_rn(__fmul_rn(m, mt[4]), spr);
            e[2] = vir;
            e[3] = 0.f;
          }
        }
        if (begin) {
          const float ca = mt[0], cb = mt[1], cd = mt[2], c1 = mt[3];
          const float sigma = g.noise ? g.sigma[row] : 0.f;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float wv = __fmaf_rn(hk, f[c], ww[c]);
            float uv = uu[c];
            float un = __fmaf_rn(cb, wv, __fmul_rn(ca, uv));
            float wn = __fmaf_rn(cd, uv, __fmul_rn(ca, wv));
            if (g.noise) wn = __fmaf_rn(sigma, g.noise[o + c], __fmul_rn(c1, wn));
            uv = __fmaf_rn(cb, wn, __fmul_rn(ca, un));
            wv = __fmaf_rn(cd, un, __fmul_rn(ca, wn));
            uu[c] = uv;
            ww[c] = wv;
            g.u[o + c] = uv;
            s_u[(k * cap + a) * 3 + c] = uv;
          }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) g.w[o + c] = ww[c];
      }
      __syncthreads();
      if (active && begin) {                           // this thread as bead s = k of atom a
        float x[3];
        const float c0 = s_c[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = __fmul_rn(c0, s_u[a * 3 + c]);
        for (int q = 1; q < P; ++q) {
          const float cqs = s_c[q * ld + k];
#pragma unroll
          for (int c = 0; c < 3; ++c) x[c] = __fmaf_rn(cqs, s_u[(q * cap + a) * 3 + c], x[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) g.pos_out[o + c] = x[c];
      }
      __syncthreads();                                 // s_f / s_u belong to the next tile from here
    }
  }
}

}  // namespace

extern "C" int nnhip_pimd_step(float* u, float* w, const float* force, const float* ctab, const float* mode_tab, const float* hk,
                               const float* mass, const float* sigma, const float* noise, const int32_t* mol_ptr,
                               const int32_t* mol_ptr_host, const float* pos_pending, int32_t flags, int32_t n_beads, int32_t n_mol,
                               int32_t n_atoms, float* pos_out, float* est_out, void* stream) {
  if (n_atoms < 0 || n_mol < 0 || flags < 1 || flags > (NNHIP_PIMD_FINISH | NNHIP_PIMD_BEGIN)) {
    nnhip_set_error("nnhip_pimd_step: bad arguments (n_mol %d, n_atoms %d, flags %d: bit 0 = finish, bit 1 = begin)", n_mol, n_atoms,
                    flags);
    return NNHIP_E_INVALID;
  }
  if (n_beads < 1 || n_beads > NNHIP_PIMD_MAX_BEADS || n_mol % n_beads != 0) {
    nnhip_set_error("nnhip_pimd_step: n_beads %d (1 .. %d expected, dividing n_mol = %d)", n_beads, NNHIP_PIMD_MAX_BEADS, n_mol);
    return NNHIP_E_INVALID;
  }
  if ((sigma == nullptr) != (noise == nullptr)) {
    nnhip_set_error("nnhip_pimd_step: sigma and noise come together (both given or both null)");
    return NNHIP_E_INVALID;
  }
  const bool begin = flags & NNHIP_PIMD_BEGIN;
  if (est_out && !(flags & NNHIP_PIMD_FINISH)) {
    nnhip_set_error("nnhip_pimd_step: est_out needs finish");
    return NNHIP_E_INVALID;
  }
  if (!mol_ptr || !mol_ptr_host) {
    nnhip_set_error("nnhip_pimd_step: null pointer (mol_ptr and mol_ptr_host are mandatory)");
    return NNHIP_E_INVALID;
  }
  if (mol_ptr_host[0] != 0 || mol_ptr_host[n_mol] != n_atoms) {
    nnhip_set_error("nnhip_pimd_step: mol_ptr must run from 0 to n_atoms = %d (got %d .. %d)", n_atoms, mol_ptr_host[0],
                    mol_ptr_host[n_mol]);
    return NNHIP_E_INVALID;
  }
  const int n_systems = n_mol / n_beads;
  long max_n = 0;
  for (int s = 0; s < n_systems; ++s) {
    const int m0 = s * n_beads;
    const long n = (long)mol_ptr_host[m0 + 1] - mol_ptr_host[m0];
    for (int k = 0; k < n_beads; ++k) {
      const long nk = (long)mol_ptr_host[m0 + k + 1] - mol_ptr_host[m0 + k];
      if (nk != n || nk < 0) {
        nnhip_set_error("nnhip_pimd_step: system %d: slot %d has %ld atoms, slot 0 has %ld (equal counts >= 0 expected)", s, k, nk, n);
        return NNHIP_E_INVALID;
      }
    }
    max_n = n > max_n ? n : max_n;
  }
  if (n_atoms == 0) return NNHIP_OK;
  if (!u || !w || !force || !ctab || !mode_tab || !hk || (begin && !pos_out) || (est_out && !mass)) {
    nnhip_set_error("nnhip_pimd_step: null pointer (u, w, force, ctab, mode_tab and hk always; pos_out with begin; est_out needs "
                    "mass)");
    return NNHIP_E_INVALID;
  }
  const size_t n3 = 3 * (size_t)n_atoms;
  if (begin && pos_pending && overlap(pos_pending, pos_out, n3)) {
    nnhip_set_error("nnhip_pimd_step: pos_out may not alias pos_pending (a forward call that has to be repeated reads it again)");
    return NNHIP_E_INVALID;
  }
  PimdArgs g;
  g.u = u;
  g.w = w;
  g.force = force;
  g.ctab = ctab;
  g.mode_tab = mode_tab;
  g.hk = hk;
  g.mass = mass;
  g.sigma = sigma;
  g.noise = noise;
  g.mol_ptr = mol_ptr;
  g.pos_out = pos_out;
  g.est_out = est_out;
  g.flags = flags;
  g.n_beads = n_beads;
  g.n_systems = n_systems;
  g.n_atoms = n_atoms;
  const int cap = PIMD_THREADS / n_beads;
  long tiles = (max_n + cap - 1) / cap;
  tiles = tiles > PIMD_MAX_TILE_BLOCKS ? PIMD_MAX_TILE_BLOCKS : tiles;
  // (a grid of at most 2^20 workgroups: more systems, or more tiles, by the kernel's stride loops)
  long gx = (1L << 20) / tiles;
  gx = gx < 1 ? 1 : gx > n_systems ? n_systems : gx;
  pimd_step_kernel<<<dim3((unsigned)gx, (unsigned)tiles), PIMD_THREADS, 0, (hipStream_t)stream>>>(g);
  LAUNCH_CHECK();
  return NNHIP_OK;
}
