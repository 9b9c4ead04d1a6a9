// Worst error, in ulps, of the fp32 library calls csrc/bias.hip relies on, against fp64 on the host: expf over the exponents of a
// Gaussian hill, atan2f over the plane (angles and torsions), and -- as a check of the compiler's defaults -- __fsqrt_rn, __fdiv_rn
// and rintf, which must come out correctly rounded (0.5, 0.5) and exact (0).  tests/bias_ref.py takes TWICE the printed expf and
// atan2f figures as its ulp counts.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probes/math_ulp_probe.hip -o tools/probes/math_ulp_probe && tools/probes/math_ulp_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define TRY(e)                                                                   \
  do {                                                                           \
    hipError_t _e = (e);                                                         \
    if (_e != hipSuccess) {                                                      \
      std::printf("%s -> %s\n", #e, hipGetErrorString(_e));                      \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

__global__ void probe(const float* a, const float* b, float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = expf(a[i]);
  out[n + i] = atan2f(a[i], b[i]);
  out[2 * n + i] = __fsqrt_rn(fabsf(b[i]));
  out[3 * n + i] = __fdiv_rn(a[i], b[i]);
  out[4 * n + i] = rintf(b[i]);
  out[5 * n + i] = atan2f(fabsf(b[i]), a[i]);
}

static double ulps(float got, double exact) {
  if (exact == 0.0) return got == 0.f ? 0.0 : INFINITY;
  int e;
  std::frexp(exact, &e);                                   // |exact| in [2^(e-1), 2^e)
  const double ulp = std::ldexp(1.0, (e - 1 < -126 ? -126 : e - 1) - 23);
  return std::fabs((double)got - exact) / ulp;
}

int main() {
  const int n = 1 << 22;
  std::vector<float> a(n), b(n), out(6 * (size_t)n);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);                 // [0, 1)
  };
  for (int i = 0; i < n; ++i) {
    a[i] = (float)(-60.0 * next());                                         // the exponent of a hill; the y of atan2f(y, x)
    b[i] = (float)((next() < 0.5 ? -1.0 : 1.0) * std::exp(12.0 * next() - 8.0));      // 3e-4 .. 55, either sign
    if (i & 1) a[i] = (float)((next() < 0.5 ? -1.0 : 1.0) * std::exp(12.0 * next() - 8.0));
  }
  float *da, *db, *dout;
  TRY(hipMalloc(&da, n * sizeof(float)));
  TRY(hipMalloc(&db, n * sizeof(float)));
  TRY(hipMalloc(&dout, 6 * (size_t)n * sizeof(float)));
  TRY(hipMemcpy(da, a.data(), n * sizeof(float), hipMemcpyHostToDevice));
  TRY(hipMemcpy(db, b.data(), n * sizeof(float), hipMemcpyHostToDevice));
  probe<<<(n + 255) / 256, 256>>>(da, db, dout, n);
  TRY(hipGetLastError());
  TRY(hipMemcpy(out.data(), dout, 6 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  double worst[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const double x = a[i], y = b[i];
    const double want[6] = {std::exp(x), std::atan2(x, y), std::sqrt(std::fabs(y)), x / y, std::nearbyint(y), std::atan2(std::fabs(y), x)};
    for (int k = 0; k < 6; ++k) {
      if (k == 0 && x > 0.0) continue;                                      // expf: the hills' range only
      const double u = ulps(out[(size_t)k * n + i], want[k]);
      if (u > worst[k]) worst[k] = u;
    }
  }
  std::printf("{\"n\": %d, \"expf_ulp\": %.4f, \"atan2f_ulp\": %.4f, \"fsqrt_rn_ulp\": %.4f, \"fdiv_rn_ulp\": %.4f, \"rintf_ulp\": %.4f, "
              "\"atan2f_upper_half_ulp\": %.4f}\n", n, worst[0], worst[1], worst[2], worst[3], worst[4], worst[5]);
  TRY(hipFree(da));
  TRY(hipFree(db));
  TRY(hipFree(dout));
  return 0;
}
