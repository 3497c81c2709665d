// rt_spec.h -- internal: ray casts and feature planes that follow mirrors and glass (include/rt_hip.h, "casts and
// planes through specular surfaces"), stated once for spec_cast_kernel and spec_render_kernel of rt_guide.hip and
// the host twin of rt_guide_host.cpp.  A chain is a sequence of rtfh::cast calls: begin(), then advance() after
// every cast until it returns false, then finish().  The caller owns the loop, so that it has one call site of
// rtfh::cast for the primary and the continuation rays.  pixel() is rtaov::pixel with a chain per sample.  Float
// arithmetic, one rounded operation per operator (-ffp-contract=off on both sides).  No HIP header.
#ifndef RT_SPEC_H
#define RT_SPEC_H

#include <stdint.h>

#include "../../include/rt_hip.h"
#include "rt_aov.h"
#include "rt_first_hit.h"

namespace rtspec {

using rtfh::dot;
using rtfh::V3;
using rtfh::v3;

constexpr int kMaxBounces = 16;

inline bool valid(const rt_spec_params& p) {
  return p.max_bounces >= 0 && p.max_bounces <= kMaxBounces && p.max_fuzz >= 0.0f && p.max_fuzz <= 1.0f &&
         (p.glass == 0 || p.glass == 1) && p.reserved == 0;
}

RT_HD V3 reflect(V3 v, V3 n) { return v - (2.0f * dot(v, n)) * n; }  // vec3.h:148-150
RT_HD V3 refract(V3 uv, V3 n, float eta) {                           // vec3.h:152-158, its double island included
  const float c = __builtin_fminf(dot(-uv, n), 1.0f);
  const V3 perp = eta * (uv + c * n);
  const float par = -__builtin_sqrtf(__builtin_fabsf((float)(1.0 - (double)dot(perp, perp))));
  return perp + par * n;
}

struct Chain {
  rt_guide_hit hit;  // the last cast that hit; the primary cast when that missed
  float thr[3];
  float t0, len0, sum;  // the primary hit's t, |d_0|, the continuation segments' t_k |d_k| in order
  int32_t k, terms, status, first_prim, first_material;
};

RT_HD void begin(Chain& c) {
  c.thr[0] = c.thr[1] = c.thr[2] = 1.0f;
  c.t0 = 0.0f, c.len0 = 1.0f, c.sum = 0.0f;
  c.k = 0, c.terms = 0, c.status = RT_SPEC_MISS, c.first_prim = -1, c.first_material = -1;
}

// h is the cast of ray e (segment c.k).  true: e has become the next segment's ray; false: the chain has ended
// with c.status.
RT_HD bool advance(const rt_scene_soa& sc, const rt_spec_params& P, Chain& c, float* e, const rt_guide_hit& h) {
  const V3 d = v3(e + 3);
  const float len = __builtin_sqrtf(dot(d, d));
  if (c.k == 0) {
    c.hit = h;
    c.t0 = h.t, c.len0 = len;
    c.first_prim = h.prim, c.first_material = h.material;
    if (h.prim < 0) {
      c.status = RT_SPEC_MISS;
      return false;
    }
  } else {
    if (h.prim < 0) {
      c.status = RT_SPEC_ESCAPED;
      return false;
    }
    c.hit = h;
    const float term = h.t * len;
    c.sum = c.terms ? c.sum + term : term;
    ++c.terms;
  }
  const rt_material& m = sc.materials[h.material];
  const bool metal = m.type == RT_MAT_METAL && m.param <= P.max_fuzz;
  const bool glass = m.type == RT_MAT_DIELECTRIC && P.glass != 0;
  if (!metal && !glass) {
    c.status = RT_SPEC_SURFACE;
    return false;
  }
  if (c.k == P.max_bounces) {
    c.status = RT_SPEC_LIMIT;
    return false;
  }
  const V3 ud = d / len, n = v3(h.n);
  V3 dir;
  if (metal) {  // material.h:46-54 with the fuzz term at its mean
    dir = reflect(ud, n);
    if (!(dot(dir, n) > 0.0f)) {
      c.status = RT_SPEC_ABSORBED;
      return false;
    }
    for (int a = 0; a < 3; ++a) c.thr[a] = c.thr[a] * h.albedo[a];
  } else {  // material.h:67-90 without Schlick's choice
    const float ratio = h.front ? 1.0f / m.param : m.param;
    const float ct = __builtin_fminf(dot(-ud, n), 1.0f);
    const float st = __builtin_sqrtf(1.0f - ct * ct);
    dir = ratio * st > 1.0f ? reflect(ud, n) : refract(ud, n, ratio);
  }
  e[0] = h.p[0], e[1] = h.p[1], e[2] = h.p[2];
  e[3] = dir.x, e[4] = dir.y, e[5] = dir.z;
  ++c.k;
  return true;
}

// Length along the chain in the primary ray's parameter units.
RT_HD float depth(const Chain& c) { return c.terms ? c.t0 + c.sum / c.len0 : c.t0; }

RT_HD void finish(const Chain& c, rt_spec_path* p) {
  p->bounces = c.k, p->status = c.status, p->first_prim = c.first_prim, p->first_material = c.first_material;
  for (int a = 0; a < 3; ++a) p->throughput[a] = c.thr[a];
  p->depth = depth(c);
}

// One ray's chain, for the host twin and the cast kernel.  hit and path may each be null.
RT_HD void trace(const rt_scene_soa& sc, const rt_spec_params& P, const float* ray, rt_guide_hit* hit, rt_spec_path* path) {
  float e[8];
  for (int a = 0; a < 8; ++a) e[a] = ray[a];
  Chain c;
  begin(c);
  rt_guide_hit h;
  do rtfh::cast(sc, e, &h);
  while (advance(sc, P, c, e, h));
  if (hit) *hit = c.hit;
  if (path) finish(c, path);
}

// rtaov::pixel with a chain per sample: the sums, their order and the divisions are that function's; what a sample
// adds is the chain's last normal, thr * (its last albedo, or the background once it has left the scene) and the
// chain's depth, while the hit count, prim and coverage stay the primary ray's.
RT_HD void pixel(const rt_scene_soa& sc, const float* table, int S, int lens, const rt_spec_params& P, int i, int j, int W, int H,
                 rtaov::Pixel& out) {
  float sn[3] = {0.0f, 0.0f, 0.0f}, sa[3] = {0.0f, 0.0f, 0.0f}, st = 0.0f;
  int32_t hits = 0, first = -1;
  for (int s = 0; s < S; ++s) {
    float e[8];
    rtaov::sample_ray(sc.camera, i, j, W, H, table + rtaov::kEntry * s, lens, e);
    Chain c;
    begin(c);
    rt_guide_hit h;
    do rtfh::cast(sc, e, &h);
    while (advance(sc, P, c, e, h));
    const bool sky = c.status == RT_SPEC_MISS || c.status == RT_SPEC_ESCAPED;
    for (int a = 0; a < 3; ++a) {
      const float al = c.thr[a] * (sky ? sc.background[a] : c.hit.albedo[a]);
      sn[a] = s ? sn[a] + c.hit.n[a] : c.hit.n[a];
      sa[a] = s ? sa[a] + al : al;
    }
    if (c.first_prim >= 0) {
      const float dp = depth(c);
      st = hits ? st + dp : dp;
      if (!hits) first = c.first_prim;
      ++hits;
    }
  }
  const float fs = (float)S;
  for (int a = 0; a < 3; ++a) out.n[a] = sn[a] / fs, out.albedo[a] = sa[a] / fs;
  out.depth = hits ? st / (float)hits : 0.0f;
  out.coverage = (float)hits / fs;
  out.prim = first;
}

}  // namespace rtspec

#endif  // RT_SPEC_H
