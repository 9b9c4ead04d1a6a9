// What the two normal-mode sampling kernels share (sample.hip: the mode matrix in LDS; sample_large.hip: streamed from HBM): the
// tile sizes, the physical constants and the rule that turns an eigenvalue into the standard deviation of its mode's amplitude.
// One definition, so a molecule both kernels can serve gets the same bits from either.
#pragma once
#include <cmath>

#include "common.h"

#define SMP_THREADS 256
#define SMP_TILE 32            // samples per workgroup
#define SMP_MAX_TILES 65535    // grid.y

// k_B T in eV: k_B = 8.617333262e-5 eV / K (CODATA 2018, exact in the SI of 2019)
inline float smp_kT(double temperature) { return (float)(8.617333262e-5 * temperature); }
// hbar sqrt(e / (1e-20 amu)) / e: eps in eV of a mode with lambda = 1 eV / (A^2 amu) -- EV_PER_WAVENUMBER x WAVENUMBER_PER_SQRT_EIGENVALUE
// of newtonnet_amd/vibrations.py (0.064654 eV)
inline float smp_hbar_unit() {
  return (float)(6.62607015e-34 / (2.0 * 3.14159265358979323846 * 1.602176634e-19) *
                 std::sqrt(1.602176634e-19 / (1e-20 * 1.66053906660e-27)));
}

// Mode with eigenvalue l of a molecule with zero threshold thr:
//   live iff l > thr                                    (projected, zero and imaginary modes: sigma = 0, by rule)
//   classical  sigma^2 = kT / l
//   quantum    sigma^2 = (eps / 2 l) coth(eps / 2 kT),  eps = hbar_unit sqrt(l),  coth(x / 2) = 1 + 2 / expm1(x), x = eps / kT
//              (expm1 -> inf gives coth = 1, the ground state, as does T = 0)
// sig = sigma, lam = l if live else 0 (the weight of q^2 / 2 in the harmonic energy); returns 1 for an imaginary mode (l < -thr).
__device__ __forceinline__ int smp_mode_rule(float l, float thr, float kT, float hbar_unit, int quantum, float* sig, float* lam) {
  const bool live = l > thr;
  float var = 0.f;
  if (live) {
    if (quantum) {
      const float eps = hbar_unit * sqrtf(l);
      const float coth = kT > 0.f ? 1.f + 2.f / expm1f(eps / kT) : 1.f;
      var = eps / (2.f * l) * coth;
    } else {
      var = kT / l;
    }
  }
  *sig = sqrtf(var);
  *lam = live ? l : 0.f;
  return l < -thr ? 1 : 0;
}
