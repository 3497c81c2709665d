// rt_aov.h -- internal: feature planes averaged over pixel-footprint, lens and shutter samples (include/rt_hip.h,
// "averaged feature planes"), stated once for aov_render_kernel of rt_guide.hip and the host twin of
// rt_guide_host.cpp.  The sample pattern is one table for the whole image, computed on the host (pattern());
// a pixel's rays, their casts through rtfh::cast and the sums in sample order are pixel().  No HIP header.
#ifndef RT_AOV_H
#define RT_AOV_H

#include <stdint.h>

#include "../../include/rt_hip.h"
#include "rt_first_hit.h"

namespace rtaov {

constexpr int kMaxSamples = 256;
constexpr int kEntry = 5;  // floats per sample: du, dv, lx, ly, f

inline bool valid(const rt_aov_params& p) {
  return p.samples >= 1 && p.samples <= kMaxSamples && (p.lens == 0 || p.lens == 1) && (p.footprint == 0 || p.footprint == 1) &&
         (p.shutter == 0 || p.shutter == 1);
}

// k's lowest `digits` digits in `base`, reversed.
inline uint32_t reversed(uint32_t k, uint32_t base, int digits) {
  uint32_t r = 0;
  for (int d = 0; d < digits; ++d) r = r * base + k % base, k /= base;
  return r;
}

// The table of a valid p: out[samples][kEntry].  Host only.
inline void pattern(const rt_aov_params& p, float* out) {
  const uint32_t S = (uint32_t)p.samples;
  uint32_t P = 1;
  int bits = 0;
  while (P < S) P *= 2, ++bits;
  uint32_t k = 0;  // the lens walk's candidate
  for (uint32_t s = 0; s < S; ++s) {
    float* e = out + kEntry * s;
    e[0] = p.footprint ? (float)(2 * s + 1) / (float)(2 * S) : 0.5f;
    e[1] = p.footprint ? (float)(2 * reversed(s, 2, bits) + 1) / (float)(2 * P) : 0.5f;
    e[2] = e[3] = 0.0f;
    if (p.lens) {
      double x, y;
      do {
        ++k;
        x = 2.0 * ((double)reversed(k, 3, 10) / 59049.0) - 1.0;
        y = 2.0 * ((double)reversed(k, 5, 7) / 78125.0) - 1.0;
      } while (!(x * x + y * y <= 1.0));
      e[2] = (float)x, e[3] = (float)y;
    }
    e[4] = p.shutter ? (float)((double)reversed(s, 7, 5) / 16807.0) : 0.5f;
  }
}

// The ray of pixel (i, j) of a W x H image for the table entry q: camera.h get_ray at
// s = (i + du) / W, t = (j + dv) / H with the lens point (lx, ly) and the time time0 + f (time1 - time0);
// without the lens, rtfh::centre_ray's expression from the camera's own origin.
RT_HD void sample_ray(const rt_camera& c, int i, int j, int W, int H, const float* q, int lens, float* e) {
  using rtfh::V3;
  using rtfh::v3;
  const float su = ((float)i + q[0]) / (float)W, sv = ((float)j + q[1]) / (float)H;
  V3 o = v3(c.origin);
  V3 d = v3(c.lower_left) + su * v3(c.horizontal) + sv * v3(c.vertical) - v3(c.origin);
  if (lens) {
    const float rx = c.lens_radius * q[2], ry = c.lens_radius * q[3];
    const V3 offset = rx * v3(c.u) + ry * v3(c.v);
    o = o + offset;
    d = d - offset;
  }
  e[0] = o.x, e[1] = o.y, e[2] = o.z;
  e[3] = d.x, e[4] = d.y, e[5] = d.z;
  e[6] = c.time0 + q[4] * (c.time1 - c.time0);
  e[7] = 0.0f;
}

struct Pixel {
  float n[3], albedo[3];
  float depth, coverage;
  int32_t prim;
};

// The averages of one pixel over the S entries of table.  The sums start as sample 0's values (the sign of a zero
// survives) and take the others in order; a miss adds cast's n = 0 and the background.
RT_HD void pixel(const rt_scene_soa& sc, const float* table, int S, int lens, int i, int j, int W, int H, Pixel& out) {
  float sn[3] = {0.0f, 0.0f, 0.0f}, sa[3] = {0.0f, 0.0f, 0.0f}, st = 0.0f;
  int32_t hits = 0, first = -1;
  for (int s = 0; s < S; ++s) {
    float e[8];
    rt_guide_hit h;
    sample_ray(sc.camera, i, j, W, H, table + kEntry * s, lens, e);
    rtfh::cast(sc, e, &h);
    for (int c = 0; c < 3; ++c) {
      sn[c] = s ? sn[c] + h.n[c] : h.n[c];
      sa[c] = s ? sa[c] + h.albedo[c] : h.albedo[c];
    }
    if (h.prim >= 0) {
      st = hits ? st + h.t : h.t;
      if (!hits) first = h.prim;
      ++hits;
    }
  }
  const float fs = (float)S;
  for (int c = 0; c < 3; ++c) out.n[c] = sn[c] / fs, out.albedo[c] = sa[c] / fs;
  out.depth = hits ? st / (float)hits : 0.0f;
  out.coverage = (float)hits / fs;
  out.prim = first;
}

}  // namespace rtaov

#endif  // RT_AOV_H
