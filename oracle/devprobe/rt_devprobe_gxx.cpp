// rt_devprobe_gxx.cpp -- test infrastructure: csrc/rt_detmath.h as g++ compiles it for the oracle (the flags of
// oracle/Makefile), over arrays of bit patterns.  The third compiler beside rt_devprobe.hip's two passes.
#include <stddef.h>
#include <stdint.h>

#include "rt_devprobe_fns.h"

#define DP_API extern "C" __attribute__((visibility("default")))

DP_API int devprobe_unary_gxx(int fn, const uint32_t* x, uint32_t* y, size_t n) {
  if (fn < dp::FN_SIN || fn > dp::FN_ACOS) return 1;
  for (size_t i = 0; i < n; ++i) y[i] = dp::det_unary(fn, x[i]);
  return 0;
}
DP_API int devprobe_binary_gxx(const uint32_t* y, const uint32_t* x, uint32_t* out, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = dp::det_atan2(y[i], x[i]);
  return 0;
}
DP_API int devprobe_checker_gxx(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = dp::det_checker(a[i], b[i], c[i]);
  return 0;
}
DP_API int devprobe_sin_neg_gxx(const uint32_t* x, uint32_t* out, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = dp::det_sin_neg(x[i]);
  return 0;
}
// The double value before det_*f's final cast, for the accuracy tests' margin (tests/test_devprobe_cpu.py):
// the header's own double-precision helpers, called as det_sinf .. det_acosf call them.
// det_logf and det_acosf have no such helper: their bodies are restated here up to the cast, for positive
// finite x and |x| <= 1 (scripts/measure_detmath_margin.py checks that the cast of each gives det_*f's bits).
static double log_before_cast(float x) {
  const uint32_t u = rtm::f2u(x);
  int e;
  double m;
  if ((u & 0x7f800000u) == 0) {
    const double sx = (double)x * 4294967296.0;
    uint64_t b;
    memcpy(&b, &sx, 8);
    e = (int)((b >> 52) & 0x7ff) - 1023 - 32;
    b = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    memcpy(&m, &b, 8);
  } else {
    e = (int)((u >> 23) & 0xff) - 127;
    m = (double)rtm::u2f((u & 0x007fffffu) | 0x3f800000u);
  }
  if (m > 1.41421356237309504880) {
    m = m * 0.5;
    e += 1;
  }
  const double s = (m - 1.0) / (m + 1.0);
  const double z = s * s;
  double p = 1.0 / 23.0;
  for (int k = 21; k >= 1; k -= 2) p = 1.0 / (double)k + z * p;
  return (double)e * 6.93147180559945286227e-01 + 2.0 * s * p;
}
static double acos_before_cast(float x) {
  const double d = (double)x;
  const double w = (1.0 - d) * (1.0 + d);
  double s = 0.0;
  if (w > 0.0) {
    s = (double)__builtin_sqrtf((float)w);
    if (s > 0.0) s = 0.5 * (s + w / s);
  }
  return rtm::atan2_d(s, d);
}
DP_API int devprobe_unary_double_gxx(int fn, const uint32_t* x, double* y, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const float f = rtm::u2f(x[i]);
    const double d = (double)f;
    bool ok;
    switch (fn) {
      case dp::FN_SIN: y[i] = rtm::sin_d(d, ok); break;
      case dp::FN_COS: y[i] = rtm::cos_d(d); break;
      case dp::FN_TAN: y[i] = rtm::sin_d(d, ok) / rtm::cos_d(d); break;
      case dp::FN_LOG: y[i] = log_before_cast(f); break;
      case dp::FN_POW5: y[i] = (d * d) * (d * d) * d; break;
      case dp::FN_ACOS: y[i] = acos_before_cast(f); break;
      default: return 1;
    }
  }
  return 0;
}
DP_API int devprobe_atan2_double_gxx(const uint32_t* y, const uint32_t* x, double* out, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = rtm::atan2_d((double)rtm::u2f(y[i]), (double)rtm::u2f(x[i]));
  return 0;
}
