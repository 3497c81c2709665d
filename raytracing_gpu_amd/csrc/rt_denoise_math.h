// rt_denoise_math.h -- internal: the arithmetic of the variance-guided NL-means denoiser (include/rt_hip.h,
// "denoiser"), stated once for the device kernels of rt_denoise.hip and the host twin of rt_denoise_blob.cpp.
// Every float operation below is one correctly rounded IEEE operation (-ffp-contract=off, correctly rounded
// divide); every sum across pixels is an integer sum.  The byte identity of rt_denoise_monitor and
// rt_denoise_monitor_blob (and the adaptive pair) rests on both compiling these functions.
#ifndef RT_DENOISE_MATH_H
#define RT_DENOISE_MATH_H

#include <stdint.h>

#include "../../include/rt_hip.h"

#ifdef __HIPCC__
#define RT_DN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RT_DN_HD inline
#endif

namespace rtdn {

constexpr int kMaxSearch = 10;  // search_radius 0..10
constexpr int kMaxPatch = 3;    // patch_radius 0..3

// k > 0, alpha >= 0, eps > 0 (a NaN fails each comparison), radii in range.
RT_DN_HD bool params_ok(const rt_denoise_params* p) {
  return p->search_radius >= 0 && p->search_radius <= kMaxSearch && p->patch_radius >= 0 && p->patch_radius <= kMaxPatch &&
         p->k > 0.0f && p->alpha >= 0.0f && p->eps > 0.0f;
}

// One value after n >= 2 frame buffers, from its moments: Q = mean of c^2 with 8 fractional bits (< 2^24),
// M = Q / 256 (exact), V = variance of that mean in c^2 units.
RT_DN_HD void prepare(uint32_t s1, uint64_t s2, int32_t n, float* M, float* V) {
  const uint64_t un = (uint64_t)n;
  const uint64_t Q = (256u * (uint64_t)s1 + un / 2) / un;
  const uint64_t D = un * s2 - (uint64_t)s1 * s1;
  const double dn = (double)n;
  *M = (float)Q / 256.0f;
  *V = (float)((double)D / (dn * dn * (double)(n - 1)));
}
RT_DN_HD uint32_t q_of(float M) { return (uint32_t)(M * 256.0f); }  // exact: M = Q / 256, Q < 2^24

// The distance term of the pair (a, b) for one channel; kk = k * k.  t is clamped to [-64, 64] with a NaN
// (k * k = inf against V = 0) taken to -64, so the cast is always defined.
RT_DN_HD int32_t term(float Ma, float Va, float Mb, float Vb, float alpha, float kk, float eps) {
  const float d = Ma - Mb;
  const float vmin = Va < Vb ? Va : Vb;  // fminf: V is never NaN
  const float num = d * d - alpha * (Va + vmin);
  const float den = eps + kk * (Va + Vb);
  float t = num / den;
  if (!(t > -64.0f)) t = -64.0f;
  if (t > 64.0f) t = 64.0f;
  return (int32_t)(t * 256.0f);
}

// The weight of a search offset from its patch sum P over cnt terms: (1 - x / 8)^8 in 16 fractional bits.
RT_DN_HD uint32_t weight(int32_t P, int32_t cnt) {
  float x = (float)P / (float)(256 * cnt);
  if (x < 0.0f) x = 0.0f;
  float s = 1.0f - x * 0.125f;
  if (s < 0.0f) s = 0.0f;
  const float s2 = s * s, s4 = s2 * s2, s8 = s4 * s4;
  return (uint32_t)(s8 * 65536.0f);
}

// Patch offsets u, |u| <= f, along one axis for which p + u and p + o + u are inside [0, size).
RT_DN_HD int32_t patch_span(int32_t p, int32_t o, int32_t f, int32_t size) {
  const int32_t low = o < 0 ? p + o : p, high = o < 0 ? p : p + o;
  const int32_t u0 = -f > -low ? -f : -low, u1 = f < size - 1 - high ? f : size - 1 - high;
  return u1 - u0 + 1;
}

RT_DN_HD float linear(uint64_t Num, uint64_t Den) { return (float)((double)Num / ((double)Den * 256.0 * 65025.0)); }
RT_DN_HD float gain(uint64_t Den) { return (float)((double)Den / 65536.0); }

}  // namespace rtdn

#endif  // RT_DENOISE_MATH_H
