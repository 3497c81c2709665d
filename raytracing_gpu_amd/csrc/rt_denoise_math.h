// rt_denoise_math.h -- internal: the arithmetic of the variance-guided NL-means denoiser (include/rt_hip.h,
// "denoiser"), stated once for the device kernels of rt_denoise.hip and the host twin of rt_denoise_blob.cpp.
// Every float operation below is one correctly rounded IEEE operation (-ffp-contract=off, correctly rounded
// divide); every sum across pixels is an integer sum.  The byte identity of rt_denoise_monitor and
// rt_denoise_monitor_blob (and the adaptive pair) rests on both compiling these functions.
#ifndef RT_DENOISE_MATH_H
#define RT_DENOISE_MATH_H

#include <stddef.h>
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

// The guided denoise (include/rt_hip.h, "guided denoise"): gains >= 0, a NaN fails.
RT_DN_HD bool guide_params_ok(const rt_guide_params* g) {
  return g->normal_gain >= 0.0f && g->albedo_gain >= 0.0f && g->depth_gain >= 0.0f;
}
// The feature planes of rows x width pixels (device memory for the kernels, host memory for the twin) with the
// gains, checked by the caller.
struct GuideView {
  const float* normal;  // [rows][width][3]
  const float* albedo;  // [rows][width][3]
  const float* depth;   // [rows][width]
  rt_guide_params gains;
};
// One pixel's features: normal, albedo, depth (0 = a miss).
struct Feature {
  float n[3], a[3], z;
};
// xf of the pair (p, q), q = p + o for an offset o other than the centre.
RT_DN_HD float feature_x(const Feature& p, const Feature& q, const rt_guide_params& g) {
  const bool mp = p.z == 0.0f, mq = q.z == 0.0f;
  if (mp != mq) return 64.0f;
  if (mp) return 0.0f;
  const float n0 = p.n[0] - q.n[0], n1 = p.n[1] - q.n[1], n2 = p.n[2] - q.n[2];
  const float a0 = p.a[0] - q.a[0], a1 = p.a[1] - q.a[1], a2 = p.a[2] - q.a[2];
  const float fn = n0 * n0 + n1 * n1 + n2 * n2;
  const float fa = a0 * a0 + a1 * a1 + a2 * a2;
  const float r = (p.z - q.z) / (p.z + q.z);
  const float fz = r * r;
  const float xf = fn * g.normal_gain + fa * g.albedo_gain + fz * g.depth_gain;
  return xf == xf ? xf : 64.0f;
}
// weight() with the feature term: x = fmaxf(x, xf) after the clamp at 0 (xf is never a NaN).
RT_DN_HD uint32_t weight(int32_t P, int32_t cnt, float xf) {
  float x = (float)P / (float)(256 * cnt);
  if (x < 0.0f) x = 0.0f;
  if (xf > x) x = xf;
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

// The host twin's two entry points with optional planes (rt_denoise_blob.cpp): what rt_denoise_*_blob and
// rt_guide_denoise_*_blob (rt_guide_host.cpp) both call.  guide = null: the unguided filter.
__attribute__((visibility("hidden"))) int monitor_blob(const void* blob, size_t n, const rt_denoise_params* prm, const GuideView* guide, int32_t plane_width,
                 int32_t plane_height, uint8_t* out, float* gain);
__attribute__((visibility("hidden"))) int adaptive_blob(const void* blob, size_t n, const rt_denoise_params* prm, const GuideView* guide, int32_t plane_width,
                  int32_t plane_height, uint8_t* out, float* gain);

}  // namespace rtdn

#endif  // RT_DENOISE_MATH_H
