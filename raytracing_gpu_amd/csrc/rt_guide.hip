// rt_guide.hip -- the device half of the guide (include/rt_hip.h, "ray casts and feature buffers"): a validated
// copy of the scene in device memory, the cast kernel (one lane per ray), the centre-ray pass into the feature
// planes, the pass that averages them over a sample pattern (rt_aov.h), the casts and the pass that follow mirrors
// and glass (rt_spec.h) and the planes' 8-bit pictures.  The first hit is rt_first_hit.h's, which the host twin
// (rt_guide_host.cpp) compiles too.  Nothing here touches a context or the render kernels; rt_progressive.hip reads the planes
// through rt_guide.h for the guided denoise.
//
// The scene stays in global memory; the rt_scene_soa of device pointers is a kernel argument, so its fields and
// every wave-uniform record reached through them (the world list, an entry's rt_object) are scalar loads.  The
// BVH walk keeps no stack (rt_first_hit.h, next_node).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <new>

#include "../../include/rt_hip.h"
#include "rt_accum_blob.h"
#include "rt_aov.h"
#include "rt_devbuf.h"
#include "rt_first_hit.h"
#include "rt_guide.h"
#include "rt_quant.h"
#include "rt_spec.h"

using rtctx::DevBuf;
using rtctx::Staged;

namespace {

__global__ __launch_bounds__(kBlock) void guide_cast_kernel(const rt_scene_soa sc, const float* __restrict__ rays, long long n,
                                                           rt_guide_hit* __restrict__ out) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  float e[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) e[c] = rays[8 * k + c];
  rtfh::cast(sc, e, out + k);
}

// One lane per pixel, 16 x 16 pixels per workgroup (a wave holds 4 rows of 16: neighbouring rays).
__global__ __launch_bounds__(256) void guide_render_kernel(const rt_scene_soa sc, int width, int height, float* __restrict__ normal,
                                                          float* __restrict__ albedo, float* __restrict__ depth,
                                                          int32_t* __restrict__ prim) {
  const int i = blockIdx.x * 16 + (threadIdx.x & 15), j = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= width || j >= height) return;
  float e[8];
  rt_guide_hit h;
  rtfh::centre_ray(sc.camera, i, j, width, height, e);
  rtfh::cast(sc, e, &h);
  const long long p = (long long)j * width + i;
#pragma unroll
  for (int c = 0; c < 3; ++c) normal[3 * p + c] = h.n[c], albedo[3 * p + c] = h.albedo[c];
  depth[p] = h.t;
  prim[p] = h.prim;
}

// The same lanes, each looping over the pattern's samples (rtaov::pixel).  Every lane of a wave is on the same
// sample at the same time: the table is read through the loop counter alone (scalar loads), and the lens offset
// and the time are wave-uniform, so a wave's rays stay as coherent as the centre pass's.
// Four waves per SIMD, the centre pass's occupancy: the sums and the loop take the kernel from 127 to 152 VGPRs
// (three waves) left alone; held to 128 it spills 80 bytes of scratch and is the faster one.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void aov_render_kernel(
    const rt_scene_soa sc, int width, int height, int samples, int lens, const float* __restrict__ table,
    float* __restrict__ normal, float* __restrict__ albedo, float* __restrict__ depth, int32_t* __restrict__ prim,
    float* __restrict__ coverage) {
  const int i = blockIdx.x * 16 + (threadIdx.x & 15), j = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= width || j >= height) return;
  rtaov::Pixel px;
  rtaov::pixel(sc, table, samples, lens, i, j, width, height, px);
  const long long p = (long long)j * width + i;
#pragma unroll
  for (int c = 0; c < 3; ++c) normal[3 * p + c] = px.n[c], albedo[3 * p + c] = px.albedo[c];
  depth[p] = px.depth;
  prim[p] = px.prim;
  coverage[p] = px.coverage;
}

// One lane per ray; a lane whose chain has ended waits for the wave's longest (rtspec::trace's do-while holds the
// one call site of rtfh::cast).
__global__ __launch_bounds__(kBlock) void spec_cast_kernel(const rt_scene_soa sc, const rt_spec_params sp, const float* __restrict__ rays,
                                                          long long n, rt_guide_hit* __restrict__ hits,
                                                          rt_spec_path* __restrict__ paths) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  rtspec::trace(sc, sp, rays + 8 * k, hits ? hits + k : nullptr, paths ? paths + k : nullptr);
}

// aov_render_kernel's lanes, loop and wave-uniform table loads, with a chain per sample (rtspec::pixel): inside a
// sample a do-while over the chain's segments, so that the world query is inlined once for primary and
// continuation rays; the lanes of a wave whose chains have ended wait for its longest before the next sample.
// Four waves per SIMD, as the averaged pass: left alone the kernel takes 177 VGPRs (two waves) and is slower on
// every scene measured; held to 128 it spills 59 VGPRs into 184 bytes of scratch.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void spec_render_kernel(
    const rt_scene_soa sc, const rt_spec_params sp, int width, int height, int samples, int lens, const float* __restrict__ table,
    float* __restrict__ normal, float* __restrict__ albedo, float* __restrict__ depth, int32_t* __restrict__ prim,
    float* __restrict__ coverage) {
  const int i = blockIdx.x * 16 + (threadIdx.x & 15), j = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= width || j >= height) return;
  rtaov::Pixel px;
  rtspec::pixel(sc, table, samples, lens, sp, i, j, width, height, px);
  const long long p = (long long)j * width + i;
#pragma unroll
  for (int c = 0; c < 3; ++c) normal[3 * p + c] = px.n[c], albedo[3 * p + c] = px.albedo[c];
  depth[p] = px.depth;
  prim[p] = px.prim;
  coverage[p] = px.coverage;
}

__global__ __launch_bounds__(kBlock) void guide_image_kernel(const float* __restrict__ plane, int normal, long long n_values,
                                                            uint8_t* __restrict__ out) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n_values) return;
  const float v = plane[k];
  out[k] = (uint8_t)quant(normal ? (v + 1.0f) / 2.0f : v);
}

// [rows][width x per] elements with the rows reversed.
template <class T>
void flip_rows(T* dst, const T* src, size_t rows, size_t row_elems) {
  for (size_t j = 0; j < rows; ++j) memcpy(dst + (rows - 1 - j) * row_elems, src + j * row_elems, row_elems * sizeof(T));
}

}  // namespace

struct RT_INTERNAL rt_guide {
  int device = 0;
  uint64_t scene_fp = 0;
  rt_scene_soa dev{};  // the scene with device pointers
  DevBuf<int32_t> world;
  DevBuf<rt_object> objects;
  DevBuf<rt_prim> prims;
  DevBuf<rt_triangle> triangles;
  DevBuf<rt_bvh_node> nodes;
  DevBuf<rt_material> materials;
  DevBuf<rt_texture> textures;
  DevBuf<rt_perlin> perlins;
  DevBuf<rt_image> images;
  DevBuf<uint8_t> texels;
  int32_t width = 0, height = 0;  // of the planes; 0 before the first render
  DevBuf<float> normal, albedo, depth;
  DevBuf<int32_t> prim;
  DevBuf<float> coverage, table;  // rt_aov_render's and rt_spec_render's: hits / samples per pixel, the pattern
  bool averaged = false;          // the planes came from one of them
  hipEvent_t ev[2] = {nullptr, nullptr}, aov_ev[2] = {nullptr, nullptr}, spec_ev[2] = {nullptr, nullptr};
  bool timed = false, aov_timed = false, spec_timed = false;
  ~rt_guide() {
    for (hipEvent_t e : spec_ev)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : aov_ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace rtguide {
View view(const rt_guide* g) {
  return View{g->device, g->scene_fp, g->width, g->height, g->normal.get(), g->albedo.get(), g->depth.get()};
}
}  // namespace rtguide

namespace {

// n elements of src in device memory owned by buf; *dst = the device pointer (null for n = 0).
template <class T>
int upload(const T* src, size_t n, DevBuf<T>& buf, const T** dst) {
  *dst = nullptr;
  if (!n) return RT_OK;
  if (!buf.alloc(n)) return RT_ERR_NOMEM;
  if (hipMemcpy(buf.get(), src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return RT_ERR_HIP;
  *dst = buf.get();
  return RT_OK;
}

// A caller's output of n elements: written on the device (p itself or a staging buffer), then copied out.
template <class T>
int copy_out(const Staged<T>& s, T* p, size_t n) {
  if (s.host() && hipMemcpy(p, s.dev(), n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return RT_ERR_HIP;
  return RT_OK;
}

// One plane of the last render into a caller's pointer (device: a copy; host: a copy, rows reversed for png_order).
template <class T>
int plane_out(const rt_guide* g, const T* plane, int per, T* out, int32_t png_order) {
  if (!out) return RT_OK;
  const size_t rows = (size_t)g->height, row_elems = (size_t)g->width * per, n = rows * row_elems;
  if (rtctx::device_ptr(out)) {
    if (png_order) return RT_ERR_ARG;
    return hipMemcpy(out, plane, n * sizeof(T), hipMemcpyDeviceToDevice) == hipSuccess ? RT_OK : RT_ERR_HIP;
  }
  if (!png_order) return hipMemcpy(out, plane, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess ? RT_OK : RT_ERR_HIP;
  std::unique_ptr<T[]> tmp(new (std::nothrow) T[n]);
  if (!tmp) return RT_ERR_NOMEM;
  if (hipMemcpy(tmp.get(), plane, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return RT_ERR_HIP;
  flip_rows(out, tmp.get(), rows, row_elems);
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_guide_create(const rt_scene_soa* scene, int hip_device, rt_guide** out) {
  if (!out) return RT_ERR_ARG;
  *out = nullptr;
  if (!scene) return RT_ERR_ARG;
  int rc = rt_scene_validate(scene, nullptr, 0);
  if (rc) return rc;
  if (!rtfh::scene_fits(scene)) return RT_ERR_SCENE;
  if (hipSetDevice(hip_device) != hipSuccess) return RT_ERR_HIP;
  std::unique_ptr<rt_guide> g(new (std::nothrow) rt_guide);
  if (!g) return RT_ERR_NOMEM;
  g->device = hip_device;
  g->scene_fp = rtacc::scene_fingerprint(scene);
  g->dev = *scene;
  if ((rc = upload(scene->world, (size_t)scene->n_world, g->world, &g->dev.world)) ||
      (rc = upload(scene->objects, (size_t)scene->n_objects, g->objects, &g->dev.objects)) ||
      (rc = upload(scene->prims, (size_t)scene->n_prims, g->prims, &g->dev.prims)) ||
      (rc = upload(scene->triangles, (size_t)scene->n_triangles, g->triangles, &g->dev.triangles)) ||
      (rc = upload(scene->nodes, (size_t)scene->n_nodes, g->nodes, &g->dev.nodes)) ||
      (rc = upload(scene->materials, (size_t)scene->n_materials, g->materials, &g->dev.materials)) ||
      (rc = upload(scene->textures, (size_t)scene->n_textures, g->textures, &g->dev.textures)) ||
      (rc = upload(scene->perlins, (size_t)scene->n_perlins, g->perlins, &g->dev.perlins)) ||
      (rc = upload(scene->images, (size_t)scene->n_images, g->images, &g->dev.images)) ||
      (rc = upload(scene->texels, (size_t)scene->n_texels, g->texels, &g->dev.texels)))
    return rc;
  if (hipEventCreate(&g->ev[0]) != hipSuccess || hipEventCreate(&g->ev[1]) != hipSuccess ||
      hipEventCreate(&g->aov_ev[0]) != hipSuccess || hipEventCreate(&g->aov_ev[1]) != hipSuccess ||
      hipEventCreate(&g->spec_ev[0]) != hipSuccess || hipEventCreate(&g->spec_ev[1]) != hipSuccess)
    return RT_ERR_HIP;
  *out = g.release();
  return RT_OK;
}

int rt_guide_destroy(rt_guide* g) {
  if (!g) return RT_ERR_ARG;
  const hipError_t e = hipSetDevice(g->device);
  delete g;
  return e == hipSuccess ? RT_OK : RT_ERR_HIP;
}

int rt_guide_cast(rt_guide* g, const float* rays, long long n, rt_guide_hit* out) {
  if (!g || n < 0 || n > (1LL << 31)) return RT_ERR_ARG;
  if (n == 0) return RT_OK;
  if (!rays || !out) return RT_ERR_ARG;
  if (hipSetDevice(g->device) != hipSuccess) return RT_ERR_HIP;
  const Staged<float> in(rays, (size_t)n * 8);
  const Staged<rt_guide_hit> res(out, (size_t)n);
  if (!in.ok() || !res.ok()) return RT_ERR_NOMEM;
  if (in.host() && hipMemcpy(in.dev(), rays, in.bytes(), hipMemcpyHostToDevice) != hipSuccess) return RT_ERR_HIP;
  if (hipEventRecord(g->ev[0], nullptr) != hipSuccess) return RT_ERR_HIP;
  hipLaunchKernelGGL(guide_cast_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, g->dev, in.dev(), n,
                     res.dev());
  if (hipGetLastError() != hipSuccess || hipEventRecord(g->ev[1], nullptr) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess)
    return RT_ERR_HIP;
  g->timed = true;
  return copy_out(res, out, (size_t)n);
}

int rt_guide_render(rt_guide* g, int32_t width, int32_t height) {
  if (!g || width < 1 || height < 1 || (long long)width * height > (1LL << 30) || (height + 15) / 16 > 65535) return RT_ERR_ARG;
  if (hipSetDevice(g->device) != hipSuccess) return RT_ERR_HIP;
  const size_t px = (size_t)width * (size_t)height;
  g->width = g->height = 0;
  g->averaged = false;
  if (g->normal.reserve(3 * px) == DevBuf<float>::failed || g->albedo.reserve(3 * px) == DevBuf<float>::failed ||
      g->depth.reserve(px) == DevBuf<float>::failed || g->prim.reserve(px) == DevBuf<int32_t>::failed)
    return RT_ERR_NOMEM;
  if (hipEventRecord(g->ev[0], nullptr) != hipSuccess) return RT_ERR_HIP;
  hipLaunchKernelGGL(guide_render_kernel, dim3((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16)), dim3(256), 0, nullptr,
                     g->dev, width, height, g->normal.get(), g->albedo.get(), g->depth.get(), g->prim.get());
  if (hipGetLastError() != hipSuccess || hipEventRecord(g->ev[1], nullptr) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess)
    return RT_ERR_HIP;
  g->timed = true;
  g->width = width, g->height = height;
  return RT_OK;
}

int rt_guide_planes(rt_guide* g, float* normal, float* albedo, float* depth, int32_t* prim, int32_t png_order) {
  if (!g || (png_order != 0 && png_order != 1)) return RT_ERR_ARG;
  if (!g->width) return RT_ERR_STATE;
  if (hipSetDevice(g->device) != hipSuccess) return RT_ERR_HIP;
  if (png_order && ((normal && rtctx::device_ptr(normal)) || (albedo && rtctx::device_ptr(albedo)) ||
                    (depth && rtctx::device_ptr(depth)) || (prim && rtctx::device_ptr(prim))))
    return RT_ERR_ARG;  // before anything is written
  int rc;
  if ((rc = plane_out(g, g->normal.get(), 3, normal, png_order)) || (rc = plane_out(g, g->albedo.get(), 3, albedo, png_order)) ||
      (rc = plane_out(g, g->depth.get(), 1, depth, png_order)) || (rc = plane_out(g, g->prim.get(), 1, prim, png_order)))
    return rc;
  return RT_OK;
}

int rt_guide_image(rt_guide* g, int32_t which, uint8_t* out, int32_t png_order) {
  if (!g || !out || (which != RT_GUIDE_NORMAL && which != RT_GUIDE_ALBEDO) || (png_order != 0 && png_order != 1)) return RT_ERR_ARG;
  if (!g->width) return RT_ERR_STATE;
  if (hipSetDevice(g->device) != hipSuccess) return RT_ERR_HIP;
  const size_t n = (size_t)g->width * (size_t)g->height * 3;
  const Staged<uint8_t> img(out, n);
  if (!img.ok()) return RT_ERR_NOMEM;
  if (png_order && !img.host()) return RT_ERR_ARG;
  hipLaunchKernelGGL(guide_image_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                     which == RT_GUIDE_NORMAL ? g->normal.get() : g->albedo.get(), which == RT_GUIDE_NORMAL ? 1 : 0, (long long)n,
                     img.dev());
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) return RT_ERR_HIP;
  if (!img.host()) return RT_OK;
  if (!png_order) return copy_out(img, out, n);
  std::unique_ptr<uint8_t[]> tmp(new (std::nothrow) uint8_t[n]);
  if (!tmp) return RT_ERR_NOMEM;
  if (hipMemcpy(tmp.get(), img.dev(), n, hipMemcpyDeviceToHost) != hipSuccess) return RT_ERR_HIP;
  flip_rows(out, tmp.get(), (size_t)g->height, (size_t)g->width * 3);
  return RT_OK;
}

int rt_aov_render(rt_guide* g, int32_t width, int32_t height, const rt_aov_params* params) {
  if (!g || width < 1 || height < 1 || (long long)width * height > (1LL << 30) || (height + 15) / 16 > 65535) return RT_ERR_ARG;
  rt_aov_params p;
  if (params) p = *params;
  else rt_aov_params_default(&p);
  if (!rtaov::valid(p)) return RT_ERR_ARG;
  if (hipSetDevice(g->device) != hipSuccess) return RT_ERR_HIP;
  const size_t px = (size_t)width * (size_t)height;
  g->width = g->height = 0;
  g->averaged = false;
  if (g->normal.reserve(3 * px) == DevBuf<float>::failed || g->albedo.reserve(3 * px) == DevBuf<float>::failed ||
      g->depth.reserve(px) == DevBuf<float>::failed || g->prim.reserve(px) == DevBuf<int32_t>::failed ||
      g->coverage.reserve(px) == DevBuf<float>::failed ||
      g->table.reserve((size_t)rtaov::kMaxSamples * rtaov::kEntry) == DevBuf<float>::failed)
    return RT_ERR_NOMEM;
  float table[rtaov::kMaxSamples * rtaov::kEntry];
  rtaov::pattern(p, table);
  if (hipMemcpy(g->table.get(), table, (size_t)p.samples * rtaov::kEntry * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
    return RT_ERR_HIP;
  if (hipEventRecord(g->aov_ev[0], nullptr) != hipSuccess) return RT_ERR_HIP;
  hipLaunchKernelGGL(aov_render_kernel, dim3((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16)), dim3(256), 0, nullptr,
                     g->dev, width, height, p.samples, p.lens, g->table.get(), g->normal.get(), g->albedo.get(), g->depth.get(),
                     g->prim.get(), g->coverage.get());
  if (hipGetLastError() != hipSuccess || hipEventRecord(g->aov_ev[1], nullptr) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess)
    return RT_ERR_HIP;
  g->aov_timed = true;
  g->width = width, g->height = height;
  g->averaged = true;
  return RT_OK;
}

int rt_aov_coverage(rt_guide* g, float* out, int32_t png_order) {
  if (!g || (png_order != 0 && png_order != 1)) return RT_ERR_ARG;
  if (!g->width || !g->averaged) return RT_ERR_STATE;
  if (hipSetDevice(g->device) != hipSuccess) return RT_ERR_HIP;
  if (png_order && out && rtctx::device_ptr(out)) return RT_ERR_ARG;
  return plane_out(g, g->coverage.get(), 1, out, png_order);
}

float rt_aov_last_ms(const rt_guide* g) {
  float ms = 0.0f;
  if (!g || !g->aov_timed || hipEventElapsedTime(&ms, g->aov_ev[0], g->aov_ev[1]) != hipSuccess) return 0.0f;
  return ms;
}

int rt_spec_cast(rt_guide* g, const float* rays, long long n, const rt_spec_params* params, rt_guide_hit* hits, rt_spec_path* paths) {
  if (!g || n < 0 || n > (1LL << 31)) return RT_ERR_ARG;
  rt_spec_params p;
  if (params) p = *params;
  else rt_spec_params_default(&p);
  if (!rtspec::valid(p)) return RT_ERR_ARG;
  if (n == 0) return RT_OK;
  if (!rays) return RT_ERR_ARG;
  if (hipSetDevice(g->device) != hipSuccess) return RT_ERR_HIP;
  const Staged<float> in(rays, (size_t)n * 8);
  // an output the caller does not want is staged as one element that the kernel never sees
  const Staged<rt_guide_hit> res(hits, hits ? (size_t)n : 1);
  const Staged<rt_spec_path> pres(paths, paths ? (size_t)n : 1);
  if (!in.ok() || !res.ok() || !pres.ok()) return RT_ERR_NOMEM;
  if (in.host() && hipMemcpy(in.dev(), rays, in.bytes(), hipMemcpyHostToDevice) != hipSuccess) return RT_ERR_HIP;
  if (hipEventRecord(g->spec_ev[0], nullptr) != hipSuccess) return RT_ERR_HIP;
  hipLaunchKernelGGL(spec_cast_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, g->dev, p, in.dev(), n,
                     hits ? res.dev() : nullptr, paths ? pres.dev() : nullptr);
  if (hipGetLastError() != hipSuccess || hipEventRecord(g->spec_ev[1], nullptr) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess)
    return RT_ERR_HIP;
  g->spec_timed = true;
  int rc = RT_OK;
  if (hits) rc = copy_out(res, hits, (size_t)n);
  if (!rc && paths) rc = copy_out(pres, paths, (size_t)n);
  return rc;
}

int rt_spec_render(rt_guide* g, int32_t width, int32_t height, const rt_aov_params* aov, const rt_spec_params* spec) {
  if (!g || width < 1 || height < 1 || (long long)width * height > (1LL << 30) || (height + 15) / 16 > 65535) return RT_ERR_ARG;
  rt_aov_params p = {1, 0, 0, 0};  // the centre ray
  if (aov) p = *aov;
  rt_spec_params sp;
  if (spec) sp = *spec;
  else rt_spec_params_default(&sp);
  if (!rtaov::valid(p) || !rtspec::valid(sp)) return RT_ERR_ARG;
  if (hipSetDevice(g->device) != hipSuccess) return RT_ERR_HIP;
  const size_t px = (size_t)width * (size_t)height;
  g->width = g->height = 0;
  g->averaged = false;
  if (g->normal.reserve(3 * px) == DevBuf<float>::failed || g->albedo.reserve(3 * px) == DevBuf<float>::failed ||
      g->depth.reserve(px) == DevBuf<float>::failed || g->prim.reserve(px) == DevBuf<int32_t>::failed ||
      g->coverage.reserve(px) == DevBuf<float>::failed ||
      g->table.reserve((size_t)rtaov::kMaxSamples * rtaov::kEntry) == DevBuf<float>::failed)
    return RT_ERR_NOMEM;
  float table[rtaov::kMaxSamples * rtaov::kEntry];
  rtaov::pattern(p, table);
  if (hipMemcpy(g->table.get(), table, (size_t)p.samples * rtaov::kEntry * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
    return RT_ERR_HIP;
  if (hipEventRecord(g->spec_ev[0], nullptr) != hipSuccess) return RT_ERR_HIP;
  hipLaunchKernelGGL(spec_render_kernel, dim3((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16)), dim3(256), 0, nullptr,
                     g->dev, sp, width, height, p.samples, p.lens, g->table.get(), g->normal.get(), g->albedo.get(), g->depth.get(),
                     g->prim.get(), g->coverage.get());
  if (hipGetLastError() != hipSuccess || hipEventRecord(g->spec_ev[1], nullptr) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess)
    return RT_ERR_HIP;
  g->spec_timed = true;
  g->width = width, g->height = height;
  g->averaged = true;
  return RT_OK;
}

float rt_spec_last_ms(const rt_guide* g) {
  float ms = 0.0f;
  if (!g || !g->spec_timed || hipEventElapsedTime(&ms, g->spec_ev[0], g->spec_ev[1]) != hipSuccess) return 0.0f;
  return ms;
}

float rt_guide_last_ms(const rt_guide* g) {
  float ms = 0.0f;
  if (!g || !g->timed || hipEventElapsedTime(&ms, g->ev[0], g->ev[1]) != hipSuccess) return 0.0f;
  return ms;
}

}  // extern "C"
