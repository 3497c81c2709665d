// rt_guide_host.cpp -- the host-only twin of the guide (rt_guide_cast_host, rt_guide_render_host, the
// rt_guide_denoise_*_blob calls and the host-only rt_aov_* and rt_spec_* calls of include/rt_hip.h): ray casts, feature planes,
// planes averaged over a sample pattern and the guided denoise of a checkpoint without a context or a GPU.  Plain C++ with no HIP include; a stand-alone program links this file
// with rt_validate.cpp and the rt_*_blob.cpp files.
//
// The first hit is rt_first_hit.h's, which the device kernels (rt_guide.hip) compile too, and the guided weight
// is rt_denoise_math.h's through the twin of rt_denoise_blob.cpp, so each pair agrees bit for bit.
#include "rt_aov.h"
#include "rt_denoise_math.h"
#include "rt_first_hit.h"
#include "rt_spec.h"

namespace {

int scene_check(const rt_scene_soa* scene) {
  if (!scene) return RT_ERR_ARG;
  const int rc = rt_scene_validate(scene, nullptr, 0);
  if (rc) return rc;
  return rtfh::scene_fits(scene) ? RT_OK : RT_ERR_SCENE;
}

template <class Blob>
int denoise_blob(Blob fn, const void* blob, size_t n, const rt_denoise_params* params, const rt_guide_params* gparams,
                 const float* normal, const float* albedo, const float* depth, int32_t plane_width, int32_t plane_height,
                 uint8_t* out, float* gain) {
  rtdn::GuideView g;
  g.normal = normal, g.albedo = albedo, g.depth = depth;
  if (gparams) g.gains = *gparams;
  else rt_guide_params_default(&g.gains);
  return fn(blob, n, params, &g, plane_width, plane_height, out, gain);
}

}  // namespace

extern "C" {

// The shipped gains (DESIGN.md 3.8 has the measurements behind them).
void rt_guide_params_default(rt_guide_params* p) {
  if (!p) return;
  p->normal_gain = 0.0f;
  p->albedo_gain = 0.25f;
  p->depth_gain = 64.0f;
  p->pad = 0;
}

int rt_guide_cast_host(const rt_scene_soa* scene, const float* rays, long long n, rt_guide_hit* out) {
  if (n < 0 || (n > 0 && (!rays || !out))) return RT_ERR_ARG;
  const int rc = scene_check(scene);
  if (rc) return rc;
  for (long long k = 0; k < n; ++k) rtfh::cast(*scene, rays + 8 * k, out + k);
  return RT_OK;
}

int rt_guide_render_host(const rt_scene_soa* scene, int32_t width, int32_t height, float* normal, float* albedo, float* depth,
                         int32_t* prim) {
  if (width < 1 || height < 1) return RT_ERR_ARG;
  const int rc = scene_check(scene);
  if (rc) return rc;
  for (int32_t j = 0; j < height; ++j)
    for (int32_t i = 0; i < width; ++i) {
      float e[8];
      rt_guide_hit h;
      rtfh::centre_ray(scene->camera, i, j, width, height, e);
      rtfh::cast(*scene, e, &h);
      const size_t p = (size_t)j * (size_t)width + (size_t)i;
      for (int c = 0; c < 3; ++c) {
        if (normal) normal[3 * p + c] = h.n[c];
        if (albedo) albedo[3 * p + c] = h.albedo[c];
      }
      if (depth) depth[p] = h.t;
      if (prim) prim[p] = h.prim;
    }
  return RT_OK;
}

void rt_aov_params_default(rt_aov_params* p) {
  if (!p) return;
  p->samples = 16;
  p->lens = p->footprint = p->shutter = 1;
}

int rt_aov_pattern(const rt_aov_params* params, float* out) {
  rt_aov_params p;
  if (params) p = *params;
  else rt_aov_params_default(&p);
  if (!out || !rtaov::valid(p)) return RT_ERR_ARG;
  rtaov::pattern(p, out);
  return RT_OK;
}

int rt_aov_render_host(const rt_scene_soa* scene, int32_t width, int32_t height, const rt_aov_params* params, float* normal,
                       float* albedo, float* depth, int32_t* prim, float* coverage) {
  rt_aov_params p;
  if (params) p = *params;
  else rt_aov_params_default(&p);
  if (width < 1 || height < 1 || !rtaov::valid(p)) return RT_ERR_ARG;
  const int rc = scene_check(scene);
  if (rc) return rc;
  float table[rtaov::kMaxSamples * rtaov::kEntry];
  rtaov::pattern(p, table);
  for (int32_t j = 0; j < height; ++j)
    for (int32_t i = 0; i < width; ++i) {
      rtaov::Pixel px;
      rtaov::pixel(*scene, table, p.samples, p.lens, i, j, width, height, px);
      const size_t k = (size_t)j * (size_t)width + (size_t)i;
      for (int c = 0; c < 3; ++c) {
        if (normal) normal[3 * k + c] = px.n[c];
        if (albedo) albedo[3 * k + c] = px.albedo[c];
      }
      if (depth) depth[k] = px.depth;
      if (prim) prim[k] = px.prim;
      if (coverage) coverage[k] = px.coverage;
    }
  return RT_OK;
}

// max_fuzz: DESIGN.md 3.10.
void rt_spec_params_default(rt_spec_params* p) {
  if (!p) return;
  p->max_bounces = 4;
  p->max_fuzz = 0.1f;
  p->glass = 1;
  p->reserved = 0;
}

int rt_spec_cast_host(const rt_scene_soa* scene, const float* rays, long long n, const rt_spec_params* params, rt_guide_hit* hits,
                      rt_spec_path* paths) {
  rt_spec_params p;
  if (params) p = *params;
  else rt_spec_params_default(&p);
  if (n < 0 || (n > 0 && !rays) || !rtspec::valid(p)) return RT_ERR_ARG;
  const int rc = scene_check(scene);
  if (rc) return rc;
  for (long long k = 0; k < n; ++k) rtspec::trace(*scene, p, rays + 8 * k, hits ? hits + k : nullptr, paths ? paths + k : nullptr);
  return RT_OK;
}

int rt_spec_render_host(const rt_scene_soa* scene, int32_t width, int32_t height, const rt_aov_params* aov,
                        const rt_spec_params* spec, float* normal, float* albedo, float* depth, int32_t* prim, float* coverage) {
  rt_aov_params p = {1, 0, 0, 0};  // the centre ray
  if (aov) p = *aov;
  rt_spec_params sp;
  if (spec) sp = *spec;
  else rt_spec_params_default(&sp);
  if (width < 1 || height < 1 || !rtaov::valid(p) || !rtspec::valid(sp)) return RT_ERR_ARG;
  const int rc = scene_check(scene);
  if (rc) return rc;
  float table[rtaov::kMaxSamples * rtaov::kEntry];
  rtaov::pattern(p, table);
  for (int32_t j = 0; j < height; ++j)
    for (int32_t i = 0; i < width; ++i) {
      rtaov::Pixel px;
      rtspec::pixel(*scene, table, p.samples, p.lens, sp, i, j, width, height, px);
      const size_t k = (size_t)j * (size_t)width + (size_t)i;
      for (int c = 0; c < 3; ++c) {
        if (normal) normal[3 * k + c] = px.n[c];
        if (albedo) albedo[3 * k + c] = px.albedo[c];
      }
      if (depth) depth[k] = px.depth;
      if (prim) prim[k] = px.prim;
      if (coverage) coverage[k] = px.coverage;
    }
  return RT_OK;
}

int rt_guide_denoise_monitor_blob(const void* blob, size_t n, const rt_denoise_params* params, const rt_guide_params* gparams,
                                  const float* normal, const float* albedo, const float* depth, int32_t plane_width,
                                  int32_t plane_height, uint8_t* out, float* gain) {
  return denoise_blob(rtdn::monitor_blob, blob, n, params, gparams, normal, albedo, depth, plane_width, plane_height, out, gain);
}

int rt_guide_denoise_adaptive_blob(const void* blob, size_t n, const rt_denoise_params* params, const rt_guide_params* gparams,
                                   const float* normal, const float* albedo, const float* depth, int32_t plane_width,
                                   int32_t plane_height, uint8_t* out, float* gain) {
  return denoise_blob(rtdn::adaptive_blob, blob, n, params, gparams, normal, albedo, depth, plane_width, plane_height, out, gain);
}

}  // extern "C"
