// check_aov_host.cpp -- the host-only twin of the averaged feature planes (rt_aov_pattern and rt_aov_render_host of
// csrc/rt_guide_host.cpp, over csrc/rt_aov.h) in a stand-alone program, the one a sanitizer build runs: the
// pattern and the planes for 1, 2, 5 and 256 samples with every combination of the three switches, on images
// smaller than a tile, on a scene with a lens, a moving sphere, a BVH, a rect and open sky; the centre pass as the
// degenerate case; every refusal.
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Iinclude -Iraytracing_gpu_amd/csrc \
//       scripts/check_aov_host.cpp raytracing_gpu_amd/csrc/rt_guide_host.cpp raytracing_gpu_amd/csrc/rt_validate.cpp \
//       raytracing_gpu_amd/csrc/rt_{accum,noise,adapt,denoise}_blob.cpp -o check_aov_host && ./check_aov_host
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_hip.h"

#define CHECK(x)                                             \
  do {                                                       \
    if (!(x)) {                                              \
      printf("check_aov_host: line %d: %s\n", __LINE__, #x); \
      return 1;                                              \
    }                                                        \
  } while (0)

namespace {

rt_prim prim(int type, int material, std::initializer_list<float> p) {
  rt_prim q = {};
  int k = 0;
  for (float v : p) q.p[k++] = v;
  q.type = type, q.material = material;
  return q;
}

rt_bvh_node node(float x0, float y0, float z0, float x1, float y1, float z1, int a, int b) {
  rt_bvh_node n = {};
  n.lo[0] = x0, n.lo[1] = y0, n.lo[2] = z0, n.hi[0] = x1, n.hi[1] = y1, n.hi[2] = z1;
  n.leaf_a = a, n.leaf_b = b;
  return n;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

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
  tex[1].color[0] = 0.9f, tex[1].color[1] = 0.1f, tex[1].color[2] = 0.2f;
  rt_material mat[3] = {};
  mat[0].type = RT_MAT_LAMBERTIAN, mat[0].texture = 0;
  mat[1].type = RT_MAT_METAL, mat[1].texture = 1;
  mat[2].type = RT_MAT_DIELECTRIC, mat[2].texture = -1, mat[2].param = 1.5f;
  std::vector<rt_prim> prims = {prim(RT_PRIM_SPHERE, 0, {-0.6f, 0.2f, 0, 0.5f}),
                                prim(RT_PRIM_MOVING_SPHERE, 1, {0.9f, -0.6f, 0.5f, 0.4f, 0, 0.8f, 0, 0, 1}),
                                prim(RT_PRIM_SPHERE, 2, {0.3f, 0.9f, -1, 0.3f}),
                                prim(RT_PRIM_RECT_XY, 0, {-2, 0.5f, -2, 0, 3, 2.5f, 2})};  // the lower left: sky elsewhere
  rt_bvh_node nodes[3] = {node(-1.2f, -1.1f, -1.4f, 1.4f, 1.3f, 1, 0, -1), node(-1.2f, -1.1f, -0.5f, 1.4f, 0.7f, 1, 0, 1),
                          node(0, 0.6f, -1.3f, 0.6f, 1.2f, -0.7f, 2, -1)};
  rt_object objects[2] = {};
  objects[0].kind = RT_OBJ_BVH, objects[0].a = 0, objects[0].b = 2;
  objects[1].kind = RT_OBJ_PRIM, objects[1].a = 3;
  int32_t world[2] = {0, 1};
  sc.world = world, sc.n_world = 2;
  sc.objects = objects, sc.n_objects = 2;
  sc.prims = prims.data(), sc.n_prims = (int32_t)prims.size();
  sc.nodes = nodes, sc.n_nodes = 3;
  sc.materials = mat, sc.n_materials = 3;
  sc.textures = tex, sc.n_textures = 2;
  char msg[128];
  if (rt_scene_validate(&sc, msg, sizeof msg) != RT_OK) {
    printf("check_aov_host: scene: %s\n", msg);
    return 1;
  }

  rt_aov_params d = {};
  rt_aov_params_default(&d);
  CHECK(d.samples == 16 && d.lens == 1 && d.footprint == 1 && d.shutter == 1 && sizeof(rt_aov_params) == 16);
  rt_aov_params_default(nullptr);

  const int counts[] = {1, 2, 5, 256};
  const int sizes[][2] = {{1, 1}, {3, 2}, {5, 7}};
  bool partial = false, moved = false;
  for (int S : counts)
    for (int sw = 0; sw < 8; ++sw) {
      rt_aov_params p = {S, sw & 1, (sw >> 1) & 1, (sw >> 2) & 1};
      std::vector<float> tab((size_t)S * 5, -9.0f);
      CHECK(rt_aov_pattern(&p, tab.data()) == RT_OK);
      for (int s = 0; s < S; ++s) {
        const float* e = &tab[(size_t)5 * s];
        CHECK(e[0] > 0.0f && e[0] < 1.0f && e[1] > 0.0f && e[1] < 1.0f && e[4] >= 0.0f && e[4] < 1.0f);
        CHECK((double)e[2] * e[2] + (double)e[3] * e[3] <= 1.0 + 1e-6);
        if (s) CHECK(p.footprint ? e[0] > e[-5] : e[0] == 0.5f);
        if (!p.footprint) CHECK(e[0] == 0.5f && e[1] == 0.5f);
        if (!p.lens) CHECK(e[2] == 0.0f && e[3] == 0.0f);
        if (!p.shutter) CHECK(e[4] == 0.5f);
      }
      CHECK(tab[0] == (p.footprint ? 1.0f / (2.0f * S) : 0.5f) && (S > 1 || (tab[0] == 0.5f && tab[1] == 0.5f)));
      for (const auto& z : sizes) {
        const int W = z[0], H = z[1];
        const size_t px = (size_t)W * H;
        std::vector<float> nrm(3 * px, -9), alb(3 * px, -9), dep(px, -9), cov(px, -9), dep2(px, -9);
        std::vector<int32_t> prm(px, -9);
        CHECK(rt_aov_render_host(&sc, W, H, &p, nrm.data(), alb.data(), dep.data(), prm.data(), cov.data()) == RT_OK);
        CHECK(rt_aov_render_host(&sc, W, H, &p, nullptr, nullptr, dep2.data(), nullptr, nullptr) == RT_OK);
        CHECK(same(dep, dep2));
        for (size_t k = 0; k < px; ++k) {
          CHECK(prm[k] >= -1 && prm[k] < sc.n_prims && cov[k] >= 0.0f && cov[k] <= 1.0f);
          CHECK((prm[k] < 0) == (cov[k] == 0.0f) && (prm[k] < 0) == (dep[k] == 0.0f));
          CHECK(std::fabs(cov[k] * (float)S - std::nearbyint(cov[k] * (float)S)) < 1e-3f);
          for (int c = 0; c < 3; ++c) CHECK(alb[3 * k + c] >= 0.0f && alb[3 * k + c] <= 1.0f && std::fabs(nrm[3 * k + c]) <= 1.0001f);
          partial = partial || (cov[k] > 0.0f && cov[k] < 1.0f);
        }
        if (S == 1 && !p.lens && !p.shutter) {  // the centre pass, whatever footprint says
          std::vector<float> n0(3 * px), a0(3 * px), d0(px);
          std::vector<int32_t> p0(px);
          CHECK(rt_guide_render_host(&sc, W, H, n0.data(), a0.data(), d0.data(), p0.data()) == RT_OK);
          CHECK(same(nrm, n0) && same(alb, a0) && same(dep, d0) && same(prm, p0));
        }
        if (S == 5 && W == 5 && sw == 4) {  // the shutter alone moves the moving sphere's depth
          rt_aov_params still = {S, 0, 0, 0};
          CHECK(rt_aov_render_host(&sc, W, H, &still, nullptr, nullptr, dep2.data(), nullptr, nullptr) == RT_OK);
          moved = !same(dep, dep2);
        }
      }
    }
  CHECK(partial && moved);
  // NULL parameters are the defaults
  {
    std::vector<float> a((size_t)16 * 5), b((size_t)16 * 5), c1(6), c2(6);
    CHECK(rt_aov_pattern(nullptr, a.data()) == RT_OK && rt_aov_pattern(&d, b.data()) == RT_OK && same(a, b));
    CHECK(rt_aov_render_host(&sc, 3, 2, nullptr, nullptr, nullptr, nullptr, nullptr, c1.data()) == RT_OK);
    CHECK(rt_aov_render_host(&sc, 3, 2, &d, nullptr, nullptr, nullptr, nullptr, c2.data()) == RT_OK && same(c1, c2));
  }
  // every refusal, with the outputs untouched
  std::vector<float> keep((size_t)256 * 5, 7.0f);
  const rt_aov_params bad[] = {{0, 1, 1, 1}, {-1, 1, 1, 1}, {257, 1, 1, 1}, {4, 2, 1, 1}, {4, -1, 1, 1},
                               {4, 1, 2, 1}, {4, 1, -1, 1}, {4, 1, 1, 2}, {4, 1, 1, -1}};
  for (const rt_aov_params& p : bad) {
    CHECK(rt_aov_pattern(&p, keep.data()) == RT_ERR_ARG);
    CHECK(rt_aov_render_host(&sc, 3, 2, &p, keep.data(), keep.data(), keep.data(), nullptr, keep.data()) == RT_ERR_ARG);
  }
  CHECK(rt_aov_pattern(&d, nullptr) == RT_ERR_ARG);
  CHECK(rt_aov_render_host(&sc, 0, 2, &d, nullptr, nullptr, keep.data(), nullptr, nullptr) == RT_ERR_ARG);
  CHECK(rt_aov_render_host(&sc, 3, -1, &d, nullptr, nullptr, keep.data(), nullptr, nullptr) == RT_ERR_ARG);
  CHECK(rt_aov_render_host(nullptr, 3, 2, &d, nullptr, nullptr, keep.data(), nullptr, nullptr) == RT_ERR_ARG);
  objects[0].b = 1;  // rows below what the format allows
  CHECK(rt_aov_render_host(&sc, 3, 2, &d, nullptr, nullptr, keep.data(), nullptr, nullptr) == RT_ERR_SCENE);
  objects[0].b = 2;
  for (float v : keep) CHECK(v == 7.0f);
  printf("check_aov_host ok\n");
  return 0;
}
