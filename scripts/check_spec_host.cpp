// check_spec_host.cpp -- the host-only twin of the casts and planes that follow mirrors and glass (rt_spec_cast_host
// and rt_spec_render_host of csrc/rt_guide_host.cpp, over csrc/rt_spec.h) in a stand-alone program, the one a
// sanitizer build runs: a hall of two facing mirrors with a lambertian sphere, a glass sphere, a metal triangle of
// short normal and open sky; one ray for every status, max_bounces 0 and 16, planes on images smaller than a tile
// from the centre ray and from 1 and 5 samples, the plain cast and the plain planes as the degenerate case, every
// refusal.
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Iinclude -Iraytracing_gpu_amd/csrc \
//       scripts/check_spec_host.cpp raytracing_gpu_amd/csrc/rt_guide_host.cpp raytracing_gpu_amd/csrc/rt_validate.cpp \
//       raytracing_gpu_amd/csrc/rt_{accum,noise,adapt,denoise}_blob.cpp -o check_spec_host && ./check_spec_host
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_hip.h"

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      printf("check_spec_host: line %d: %s\n", __LINE__, #x); \
      return 1;                                               \
    }                                                         \
  } while (0)

namespace {

rt_prim prim(int type, int material, std::initializer_list<float> p) {
  rt_prim q = {};
  int k = 0;
  for (float v : p) q.p[k++] = v;
  q.type = type, q.material = material;
  return q;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

struct RayRow {
  float e[8];
  int status, bounces;  // with max_bounces = 16
};

}  // namespace

int main() {
  // a camera at (0, 0, -5) looking down +z through a 4 x 4 window at z = 0, with a lens and an open shutter
  rt_scene_soa sc = {};
  const float cam[21] = {0, 0, -5, -2, -2, 0, 4, 0, 0, 0, 4, 0, 1, 0, 0, 0, 1, 0, 0, 0, -1};
  memcpy(&sc.camera, cam, sizeof(cam));
  sc.camera.lens_radius = 0.25f, sc.camera.time0 = 0.0f, sc.camera.time1 = 1.0f;
  sc.background[0] = 0.7f, sc.background[1] = 0.8f, sc.background[2] = 1.0f;
  sc.aspect = 1.0f;
  rt_texture tex[2] = {};
  tex[0].color[0] = 0.25f, tex[0].color[1] = 0.5f, tex[0].color[2] = 0.75f;
  tex[1].color[0] = 0.9f, tex[1].color[1] = 0.8f, tex[1].color[2] = 0.5f;
  rt_material mat[4] = {};
  mat[0].type = RT_MAT_LAMBERTIAN, mat[0].texture = 0;
  mat[1].type = RT_MAT_METAL, mat[1].texture = 1, mat[1].param = 0.0f;
  mat[2].type = RT_MAT_DIELECTRIC, mat[2].texture = -1, mat[2].param = 1.5f;
  mat[3].type = RT_MAT_METAL, mat[3].texture = 1, mat[3].param = 0.5f;
  rt_triangle tri = {};  // cross(e1, e0) = (0, 0, -0.36): a shading normal of squared length 0.13
  tri.v0[0] = -0.3f, tri.v0[1] = -1.5f, tri.v0[2] = 3.0f;
  tri.e0[0] = 0.6f, tri.e1[1] = 0.6f;
  for (int c = 0; c < 3; ++c) tri.v1[c] = tri.v0[c] + tri.e0[c], tri.v2[c] = tri.v0[c] + tri.e1[c];
  tri.d00 = 0.36f, tri.d01 = 0.0f, tri.d11 = 0.36f, tri.inv_denom = 1.0f / (0.36f * 0.36f);
  tri.uv[2] = 1.0f, tri.uv[5] = 1.0f;
  std::vector<rt_prim> prims = {prim(RT_PRIM_RECT_YZ, 1, {-2, 2, -1, 6, -1.5f, 4, 7}),  // the mirrors x = -1.5 and x = 1.5
                                prim(RT_PRIM_RECT_YZ, 1, {-2, 2, -1, 6, 1.5f, 4, 7}),
                                prim(RT_PRIM_SPHERE, 0, {-0.5f, -0.5f, 2, 0.6f}),
                                prim(RT_PRIM_SPHERE, 2, {0.6f, 0.6f, 1, 0.5f}),
                                prim(RT_PRIM_TRIANGLE, 1, {0}),
                                prim(RT_PRIM_RECT_XY, 0, {-1.5f, 1.5f, -2, 0, 6, 3, 2}),  // the lower half of the far end: sky above
                                prim(RT_PRIM_MOVING_SPHERE, 3, {0.9f, -1.2f, 2.5f, 0.4f, 0, 0.5f, 0, 0, 1})};
  rt_object objects[2] = {};
  objects[0].kind = RT_OBJ_LIST, objects[0].a = 0, objects[0].b = 5;
  objects[1].kind = RT_OBJ_LIST, objects[1].a = 5, objects[1].b = 2;
  int32_t world[2] = {0, 1};
  sc.world = world, sc.n_world = 2;
  sc.objects = objects, sc.n_objects = 2;
  sc.prims = prims.data(), sc.n_prims = (int32_t)prims.size();
  sc.triangles = &tri, sc.n_triangles = 1;
  sc.materials = mat, sc.n_materials = 4;
  sc.textures = tex, sc.n_textures = 2;
  char msg[128];
  if (rt_scene_validate(&sc, msg, sizeof msg) != RT_OK) {
    printf("check_spec_host: scene: %s\n", msg);
    return 1;
  }

  rt_spec_params d = {};
  rt_spec_params_default(&d);
  CHECK(d.max_bounces == 4 && d.glass == 1 && d.reserved == 0 && d.max_fuzz == 0.1f);
  CHECK(sizeof(rt_spec_params) == 16 && sizeof(rt_spec_path) == 32 && sizeof(rt_guide_hit) == 64);
  rt_spec_params_default(nullptr);

  // one ray for every status
  const RayRow rows[] = {
      {{0, 1, -5, 0, 1, 0, 0.5f, 0}, RT_SPEC_MISS, 0},                  // straight up between the mirrors
      {{-0.5f, -0.5f, -5, 0, 0, 1, 0.5f, 0}, RT_SPEC_SURFACE, 0},       // the lambertian sphere
      {{0, 0, 0, 1, 1, 0.1f, 0.5f, 0}, RT_SPEC_ESCAPED, 1},             // off the right mirror, over the left one
      {{0, 0, 0, 1, 0, 0.001f, 0.5f, 0}, RT_SPEC_LIMIT, 16},            // to and fro between the mirrors
      {{-0.1f, -1.3f, -5, 0, 0, 1, 0.5f, 0}, RT_SPEC_ABSORBED, 0},      // the triangle of short normal
      {{0.6f, 0.6f, -5, 0, 0, 2, 0.5f, 0}, RT_SPEC_ESCAPED, 1},         // through the glass sphere's front, into the sky
      {{0, -1.8f, 0, 1, 0.001f, 0.5f, 0.5f, 0}, RT_SPEC_SURFACE, -1},  // along the hall onto the far wall, after some bounces
      {{0.9f, -1.0f, -5, 0, 0, 1, 0.5f, 0}, RT_SPEC_SURFACE, 0},        // the metal of fuzz 0.5 under max_fuzz 0.25
  };
  const int n = (int)(sizeof(rows) / sizeof(rows[0]));
  std::vector<float> rays;
  for (const RayRow& r : rows) rays.insert(rays.end(), r.e, r.e + 8);
  for (int mb : {0, 1, 16}) {
    rt_spec_params p = {mb, 0.25f, 1, 0};
    std::vector<rt_guide_hit> hits(n), plain(n), hits2(n);
    std::vector<rt_spec_path> paths(n), paths2(n);
    CHECK(rt_spec_cast_host(&sc, rays.data(), n, &p, hits.data(), paths.data()) == RT_OK);
    CHECK(rt_spec_cast_host(&sc, rays.data(), n, &p, hits2.data(), nullptr) == RT_OK && same(hits, hits2));
    CHECK(rt_spec_cast_host(&sc, rays.data(), n, &p, nullptr, paths2.data()) == RT_OK);
    CHECK(memcmp(paths.data(), paths2.data(), n * sizeof(rt_spec_path)) == 0);
    CHECK(rt_guide_cast_host(&sc, rays.data(), n, plain.data()) == RT_OK);
    if (mb == 0) CHECK(same(hits, plain));
    for (int k = 0; k < n; ++k) {
      const rt_spec_path& q = paths[k];
      CHECK(q.bounces >= 0 && q.bounces <= mb && q.status >= RT_SPEC_MISS && q.status <= RT_SPEC_ABSORBED);
      CHECK(q.first_prim == plain[k].prim && q.first_material == plain[k].material);
      CHECK((q.status == RT_SPEC_MISS) == (plain[k].prim < 0) && q.depth >= plain[k].t);
      if (q.bounces == 0) CHECK(q.depth == plain[k].t && q.throughput[0] == 1.0f && q.throughput[2] == 1.0f);
      if (q.status == RT_SPEC_LIMIT) CHECK(q.bounces == mb);
      if (mb == 16) {
        CHECK(q.status == rows[k].status);
        if (rows[k].bounces >= 0) CHECK(q.bounces == rows[k].bounces);
        else CHECK(q.bounces >= 2 && hits[k].prim == 5 && q.throughput[0] < 0.9f * 0.9f + 1e-6f);
      }
    }
    if (mb == 16) {  // the mirrors' tint, 16 times; the glass leaves the throughput alone
      CHECK(std::fabs(paths[3].throughput[0] - std::pow(0.9f, 16.0f)) < 1e-5f && paths[5].throughput[1] == 1.0f);
      CHECK(paths[3].depth > 16 * 2.9f && paths[3].depth < 16 * 3.1f + 1.5f);  // |d| is about 1: sixteen crossings of 3
    }
  }
  // a metal of fuzz 0.5 is a mirror under max_fuzz 0.5, glass is a surface with glass = 0
  {
    rt_spec_params p = {4, 0.5f, 0, 0};
    std::vector<rt_spec_path> paths(n);
    CHECK(rt_spec_cast_host(&sc, rays.data(), n, &p, nullptr, paths.data()) == RT_OK);
    CHECK(paths[7].bounces >= 1 && paths[5].bounces == 0 && paths[5].status == RT_SPEC_SURFACE);
  }

  // planes on images smaller than a tile
  const int sizes[][2] = {{1, 1}, {3, 2}, {5, 7}};
  bool deeper = false, partial = false;
  for (int S : {0, 1, 5})
    for (int mb : {0, 16})
      for (const auto& z : sizes) {
        const int W = z[0], H = z[1];
        const size_t px = (size_t)W * H;
        rt_aov_params ap = {S ? S : 1, S ? 1 : 0, S ? 1 : 0, S ? 1 : 0};
        const rt_aov_params* aov = S ? &ap : nullptr;
        rt_spec_params p = {mb, 0.25f, 1, 0};
        std::vector<float> nrm(3 * px, -9), alb(3 * px, -9), dep(px, -9), cov(px, -9), dep2(px, -9);
        std::vector<float> n0(3 * px, -9), a0(3 * px, -9), d0(px, -9), c0(px, -9);
        std::vector<int32_t> prm(px, -9), p0(px, -9);
        CHECK(rt_spec_render_host(&sc, W, H, aov, &p, nrm.data(), alb.data(), dep.data(), prm.data(), cov.data()) == RT_OK);
        CHECK(rt_spec_render_host(&sc, W, H, aov, &p, nullptr, nullptr, dep2.data(), nullptr, nullptr) == RT_OK && same(dep, dep2));
        CHECK(rt_aov_render_host(&sc, W, H, &ap, n0.data(), a0.data(), d0.data(), p0.data(), c0.data()) == RT_OK);
        CHECK(same(prm, p0) && same(cov, c0));  // the silhouette is the first surface's
        if (mb == 0) CHECK(same(nrm, n0) && same(alb, a0) && same(dep, d0));
        if (!S) {
          CHECK(rt_guide_render_host(&sc, W, H, n0.data(), a0.data(), d0.data(), p0.data()) == RT_OK && same(prm, p0));
          if (mb == 0) CHECK(same(nrm, n0) && same(alb, a0) && same(dep, d0));
        }
        for (size_t k = 0; k < px; ++k) {
          CHECK(prm[k] >= -1 && prm[k] < sc.n_prims && cov[k] >= 0.0f && cov[k] <= 1.0f && dep[k] >= d0[k]);
          CHECK((prm[k] < 0) == (cov[k] == 0.0f) && (prm[k] < 0) == (dep[k] == 0.0f));
          for (int c = 0; c < 3; ++c) CHECK(alb[3 * k + c] >= 0.0f && alb[3 * k + c] <= 1.0f && std::fabs(nrm[3 * k + c]) <= 1.0001f);
          deeper = deeper || dep[k] > d0[k];
          partial = partial || (cov[k] > 0.0f && cov[k] < 1.0f);
        }
      }
  CHECK(deeper && partial);
  // NULL parameters are the defaults
  {
    std::vector<float> a(6), b(6);
    CHECK(rt_spec_render_host(&sc, 3, 2, nullptr, nullptr, nullptr, nullptr, a.data(), nullptr, nullptr) == RT_OK);
    CHECK(rt_spec_render_host(&sc, 3, 2, nullptr, &d, nullptr, nullptr, b.data(), nullptr, nullptr) == RT_OK && same(a, b));
    std::vector<rt_spec_path> p1(n), p2(n);
    CHECK(rt_spec_cast_host(&sc, rays.data(), n, nullptr, nullptr, p1.data()) == RT_OK);
    CHECK(rt_spec_cast_host(&sc, rays.data(), n, &d, nullptr, p2.data()) == RT_OK);
    CHECK(memcmp(p1.data(), p2.data(), n * sizeof(rt_spec_path)) == 0);
    CHECK(rt_spec_cast_host(&sc, nullptr, 0, nullptr, nullptr, nullptr) == RT_OK);
    CHECK(rt_spec_cast_host(&sc, rays.data(), n, nullptr, nullptr, nullptr) == RT_OK);
  }
  // every refusal, with the outputs untouched
  std::vector<float> keep(64, 7.0f);
  std::vector<rt_guide_hit> nohit(n);
  memset(nohit.data(), 0x5a, n * sizeof(rt_guide_hit));
  const float nan = std::nanf("");
  const rt_spec_params bad[] = {{-1, 0.25f, 1, 0}, {17, 0.25f, 1, 0}, {4, -0.1f, 1, 0}, {4, 1.5f, 1, 0},
                                {4, nan, 1, 0},    {4, 0.25f, 2, 0},  {4, 0.25f, -1, 0}, {4, 0.25f, 1, 1}};
  const rt_aov_params ok_aov = {2, 1, 1, 1}, bad_aov = {0, 1, 1, 1};
  for (const rt_spec_params& p : bad) {
    CHECK(rt_spec_cast_host(&sc, rays.data(), n, &p, nohit.data(), nullptr) == RT_ERR_ARG);
    CHECK(rt_spec_render_host(&sc, 3, 2, &ok_aov, &p, keep.data(), keep.data(), keep.data(), nullptr, keep.data()) == RT_ERR_ARG);
    CHECK(rt_spec_render_host(&sc, 3, 2, nullptr, &p, keep.data(), keep.data(), keep.data(), nullptr, keep.data()) == RT_ERR_ARG);
  }
  CHECK(rt_spec_render_host(&sc, 3, 2, &bad_aov, &d, keep.data(), nullptr, nullptr, nullptr, nullptr) == RT_ERR_ARG);
  CHECK(rt_spec_render_host(&sc, 0, 2, nullptr, &d, keep.data(), nullptr, nullptr, nullptr, nullptr) == RT_ERR_ARG);
  CHECK(rt_spec_render_host(&sc, 3, -1, nullptr, &d, keep.data(), nullptr, nullptr, nullptr, nullptr) == RT_ERR_ARG);
  CHECK(rt_spec_render_host(nullptr, 3, 2, nullptr, &d, keep.data(), nullptr, nullptr, nullptr, nullptr) == RT_ERR_ARG);
  CHECK(rt_spec_cast_host(nullptr, rays.data(), n, &d, nohit.data(), nullptr) == RT_ERR_ARG);
  CHECK(rt_spec_cast_host(&sc, nullptr, n, &d, nohit.data(), nullptr) == RT_ERR_ARG);
  CHECK(rt_spec_cast_host(&sc, rays.data(), -1, &d, nohit.data(), nullptr) == RT_ERR_ARG);
  world[1] = 9;  // no such object
  CHECK(rt_spec_cast_host(&sc, rays.data(), n, &d, nohit.data(), nullptr) == RT_ERR_SCENE);
  CHECK(rt_spec_render_host(&sc, 3, 2, nullptr, &d, keep.data(), nullptr, nullptr, nullptr, nullptr) == RT_ERR_SCENE);
  world[1] = 1;
  for (float v : keep) CHECK(v == 7.0f);
  for (size_t k = 0; k < n * sizeof(rt_guide_hit); ++k) CHECK(((const unsigned char*)nohit.data())[k] == 0x5a);
  printf("check_spec_host ok\n");
  return 0;
}
