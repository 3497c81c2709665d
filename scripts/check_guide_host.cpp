// check_guide_host.cpp -- the guide's host-only twin (csrc/rt_guide_host.cpp) in a stand-alone program, the one a
// sanitizer build runs: the smallest scene of every object kind (a primitive, a list, a BVH of two rows with a
// one-primitive leaf, a transform, a medium; every primitive type; every texture type), rays that hit, miss, graze
// and carry zeros and NaNs, planes smaller than a tile, and the guided denoise on images smaller than its window.
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Iinclude -Iraytracing_gpu_amd/csrc \
//       scripts/check_guide_host.cpp raytracing_gpu_amd/csrc/rt_guide_host.cpp raytracing_gpu_amd/csrc/rt_validate.cpp \
//       raytracing_gpu_amd/csrc/rt_{accum,noise,adapt,denoise}_blob.cpp -o check_guide_host && ./check_guide_host
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_hip.h"

#define CHECK(x)                                               \
  do {                                                         \
    if (!(x)) {                                                \
      printf("check_guide_host: line %d: %s\n", __LINE__, #x); \
      return 1;                                                \
    }                                                          \
  } while (0)

namespace {

struct Scene {
  std::vector<int32_t> world;
  std::vector<rt_object> objects;
  std::vector<rt_prim> prims;
  std::vector<rt_triangle> tris;
  std::vector<rt_bvh_node> nodes;
  std::vector<rt_material> mats;
  std::vector<rt_texture> texs;
  std::vector<rt_perlin> perlins;
  std::vector<rt_image> images;
  std::vector<uint8_t> texels;
  rt_scene_soa soa{};

  int tex(int type, int a = 0, int b = 0, float scale = 1.0f) {
    rt_texture t = {};
    t.type = type, t.a = a, t.b = b, t.scale = scale;
    t.color[0] = 0.25f, t.color[1] = 0.5f, t.color[2] = 0.75f;
    texs.push_back(t);
    return (int)texs.size() - 1;
  }
  int mat(int type, int texture) {
    rt_material m = {};
    m.type = type, m.texture = texture, m.param = 1.5f;
    mats.push_back(m);
    return (int)mats.size() - 1;
  }
  int prim(int type, int material, std::initializer_list<float> p) {
    rt_prim q = {};
    int k = 0;
    for (float v : p) q.p[k++] = v;
    q.type = type, q.material = material;
    prims.push_back(q);
    return (int)prims.size() - 1;
  }
  int obj(int kind, int a, int b = 0, std::initializer_list<float> f = {}) {
    rt_object o = {};
    o.kind = kind, o.a = a, o.b = b;
    int k = 0;
    for (float v : f) o.f[k++] = v;
    objects.push_back(o);
    return (int)objects.size() - 1;
  }
  const rt_scene_soa* view() {
    rt_camera& c = soa.camera;  // at (0, 0, -5) looking down +z, a 4 x 4 window at z = 0
    const float cam[21] = {0, 0, -5, -2, -2, 0, 4, 0, 0, 0, 4, 0, 1, 0, 0, 0, 1, 0, 0, 0, -1};
    memcpy(&c, cam, sizeof(cam));
    c.lens_radius = 0.0f, c.time0 = 0.0f, c.time1 = 1.0f;
    soa.background[0] = 0.7f, soa.background[1] = 0.8f, soa.background[2] = 1.0f;
    soa.aspect = 1.0f;
    soa.world = world.data(), soa.n_world = (int32_t)world.size();
    soa.objects = objects.data(), soa.n_objects = (int32_t)objects.size();
    soa.prims = prims.data(), soa.n_prims = (int32_t)prims.size();
    soa.triangles = tris.data(), soa.n_triangles = (int32_t)tris.size();
    soa.nodes = nodes.data(), soa.n_nodes = (int32_t)nodes.size();
    soa.materials = mats.data(), soa.n_materials = (int32_t)mats.size();
    soa.textures = texs.data(), soa.n_textures = (int32_t)texs.size();
    soa.perlins = perlins.data(), soa.n_perlins = (int32_t)perlins.size();
    soa.images = images.data(), soa.n_images = (int32_t)images.size();
    soa.texels = texels.data(), soa.n_texels = (int64_t)texels.size();
    return &soa;
  }
};

rt_bvh_node node(float x0, float y0, float z0, float x1, float y1, float z1, int a, int b) {
  rt_bvh_node n = {};
  n.lo[0] = x0, n.lo[1] = y0, n.lo[2] = z0, n.hi[0] = x1, n.hi[1] = y1, n.hi[2] = z1;
  n.leaf_a = a, n.leaf_b = b;
  return n;
}

}  // namespace

int main() {
  Scene s;
  // textures of every type; materials of every type
  rt_perlin pn = {};
  for (int i = 0; i < 256; ++i) {
    pn.ranvec[i][0] = 0.6f, pn.ranvec[i][1] = (i & 1) ? 0.8f : -0.8f, pn.ranvec[i][2] = 0.0f;
    pn.perm_x[i] = i, pn.perm_y[i] = 255 - i, pn.perm_z[i] = (i * 7) & 255;
  }
  s.perlins.push_back(pn);
  s.images.push_back(rt_image{2, 2, 3, 0});
  s.images.push_back(rt_image{0, 0, 0, 0});   // no data: cyan
  s.images.push_back(rt_image{3, 1, 1, 12});  // one byte per pixel reads two bytes past its last texel
  for (int k = 0; k < 12 + 3 + 2; ++k) s.texels.push_back((uint8_t)(40 + 13 * k));
  const int solid = s.tex(RT_TEX_SOLID), noise = s.tex(RT_TEX_NOISE, 0, 0, 4.0f), turb = s.tex(RT_TEX_TURBULENT, 0, 7, 2.0f);
  const int marble = s.tex(RT_TEX_MARBLE, 0, 7, 3.0f), image = s.tex(RT_TEX_IMAGE, 0), cyan = s.tex(RT_TEX_IMAGE, 1);
  const int grey = s.tex(RT_TEX_IMAGE, 2), checker = s.tex(RT_TEX_CHECKER, noise, image);
  const int m_solid = s.mat(RT_MAT_LAMBERTIAN, solid), m_noise = s.mat(RT_MAT_METAL, noise), m_turb = s.mat(RT_MAT_LAMBERTIAN, turb);
  const int m_marble = s.mat(RT_MAT_DIFFUSE_LIGHT, marble), m_image = s.mat(RT_MAT_LAMBERTIAN, image);
  const int m_cyan = s.mat(RT_MAT_LAMBERTIAN, cyan), m_grey = s.mat(RT_MAT_LAMBERTIAN, grey), m_check = s.mat(RT_MAT_LAMBERTIAN, checker);
  const int m_glass = s.mat(RT_MAT_DIELECTRIC, -1), m_fog = s.mat(RT_MAT_ISOTROPIC, solid);
  // primitives of every type
  rt_triangle t = {};
  const float tv[15] = {-1.8f, 0.2f, 1, -1.0f, 0.2f, 1, -1.4f, 1.0f, 1, 0.8f, 0, 0, 0.4f, 0.8f, 0};
  memcpy(&t, tv, sizeof(tv));
  t.d00 = 0.64f, t.d01 = 0.32f, t.d11 = 0.8f, t.inv_denom = 1.0f / (0.64f * 0.8f - 0.32f * 0.32f);
  const float uv[6] = {0, 0, 1, 0, 0.5f, 1};
  memcpy(t.uv, uv, sizeof(uv));
  s.tris.push_back(t);
  t.vertex_normals = 1;
  t.n0[2] = t.n1[2] = t.n2[2] = -1.0f, t.n1[0] = 0.3f;
  for (int k = 0; k < 9; ++k) (&t.v0[0])[k] += k % 3 == 1 ? -1.2f : 0.0f;  // a second one, lower
  s.tris.push_back(t);
  const int sphere = s.prim(RT_PRIM_SPHERE, m_image, {0, 0, 0, 0.5f});
  const int mover = s.prim(RT_PRIM_MOVING_SPHERE, m_noise, {1.2f, 1.2f, 0, 0.4f, 0, 0.3f, 0, 0, 1});
  const int rxy = s.prim(RT_PRIM_RECT_XY, m_check, {-2, 2, -2, 2, 3, 4, 4});
  const int rxz = s.prim(RT_PRIM_RECT_XZ, m_turb, {-2, 2, -1, 3, -1.9f, 4, 4});
  const int ryz = s.prim(RT_PRIM_RECT_YZ, m_marble, {-2, 2, -1, 3, 1.9f, 4, 4});
  const int tri0 = s.prim(RT_PRIM_TRIANGLE, m_cyan, {0}), tri1 = s.prim(RT_PRIM_TRIANGLE, m_grey, {1});
  const int box = s.prim(RT_PRIM_BOX, m_glass, {-0.3f, -0.3f, -0.3f, 0.3f, 0.3f, 0.3f});
  const int fogbox = s.prim(RT_PRIM_BOX, m_solid, {-0.4f, -0.4f, -0.4f, 0.4f, 0.4f, 0.4f});
  const int zero = s.prim(RT_PRIM_SPHERE, m_image, {-1.5f, -1.5f, 0, 0.0f});  // radius 0: NaN normals, never an image index
  // objects of every kind: a BVH of two rows (three primitives, one leaf alone), a list, a transform, a medium
  s.nodes.push_back(node(-2, -2, -1, 2, 2, 3.1f, 0, -1));
  s.nodes.push_back(node(-1, -1, -1, 2, 2, 1, sphere, mover));
  s.nodes.push_back(node(-2, -2, 2.9f, 2, 2, 3.1f, rxy, -1));
  const int o_bvh = s.obj(RT_OBJ_BVH, 0, 2), o_list = s.obj(RT_OBJ_LIST, rxz, 2), o_tri0 = s.obj(RT_OBJ_PRIM, tri0);
  const int o_tri1 = s.obj(RT_OBJ_PRIM, tri1), o_box = s.obj(RT_OBJ_PRIM, box), o_fogbox = s.obj(RT_OBJ_PRIM, fogbox);
  const int o_x = s.obj(RT_OBJ_XFORM, o_box, 3, {1.2f, -1.2f, 0.2f, 0.5f, 0.8660254f});
  const int o_xf = s.obj(RT_OBJ_XFORM, o_fogbox, 1, {0.0f, 1.3f, 0});
  const int o_fog = s.obj(RT_OBJ_MEDIUM, o_xf, m_fog, {-1.0f / 0.5f}), o_zero = s.obj(RT_OBJ_PRIM, zero);
  (void)ryz;
  s.world = {o_bvh, o_list, o_tri0, o_tri1, o_x, o_fog, o_zero};
  const rt_scene_soa* sc = s.view();
  char msg[128];
  if (rt_scene_validate(sc, msg, sizeof msg) != RT_OK) {
    printf("check_guide_host: scene: %s\n", msg);
    return 1;
  }

  // planes smaller than a tile, and one larger; the centre ray hits the sphere
  const int sizes[][2] = {{1, 1}, {3, 2}, {5, 7}, {37, 29}};
  for (const auto& z : sizes) {
    const int W = z[0], H = z[1];
    const size_t px = (size_t)W * H;
    std::vector<float> nrm(3 * px, -9), alb(3 * px, -9), dep(px, -9);
    std::vector<int32_t> prim(px, -9);
    CHECK(rt_guide_render_host(sc, W, H, nrm.data(), alb.data(), dep.data(), prim.data()) == RT_OK);
    CHECK(rt_guide_render_host(sc, W, H, nullptr, nullptr, dep.data(), nullptr) == RT_OK);
    for (size_t p = 0; p < px; ++p) CHECK(prim[p] >= -1 && prim[p] < sc->n_prims && (prim[p] < 0) == (dep[p] == 0.0f));
    if (W == 1) CHECK(prim[0] == sphere && std::fabs(dep[0] - 0.9f) < 1e-5f && nrm[2] < -0.99f);
    if (W == 37) {
      std::vector<char> seen((size_t)sc->n_prims, 0);
      for (size_t p = 0; p < px; ++p)
        if (prim[p] >= 0) seen[(size_t)prim[p]] = 1;
      for (int k : {sphere, mover, rxy, rxz, ryz, tri0, tri1, box, fogbox}) CHECK(seen[(size_t)k]);
    }
  }
  // rays: a hit, a miss, zero and NaN directions, an origin on a rect's plane, a direction along a box face
  const float rays[][8] = {{0, 0, -5, 0, 0, 1, 0.5f, 0},   {0, 9, -5, 0, 0, -1, 0, 0},         {0, 0, -5, 0, 0, 0, 0, 0},
                           {0, 0, -5, NAN, NAN, NAN, 0, 0}, {0, 0, 3, 0.1f, 0.2f, 1, 0, 0},      {-0.3f, 0, -5, 0, 0, 1, 0, 0},
                           {0, 0, 3, 0, 0, -1, 0, 0},       {1.9f, 0, -5, 0, 0, 1, NAN, 0},      {-1.5f, -1.5f, -5, 0, 0, 1, 0, 0}};
  const long long n = (long long)(sizeof rays / sizeof rays[0]);
  std::vector<rt_guide_hit> hits((size_t)n);
  CHECK(rt_guide_cast_host(sc, &rays[0][0], n, hits.data()) == RT_OK);
  CHECK(hits[0].prim == sphere && hits[0].front == 1 && hits[0].material == m_image);
  CHECK(hits[1].prim == -1 && hits[1].t == 0.0f && hits[1].albedo[2] == 1.0f);
  for (const rt_guide_hit& h : hits) CHECK(h.prim >= -1 && h.prim < sc->n_prims);  // degenerate rays: the reference's NaN hits, in range
  CHECK(hits[4].prim == -1);       // from the xy rect's own plane: t = 0 is below 0.001
  CHECK(hits[6].prim == sphere);   // from that plane back towards the camera: the far side of the sphere first
  CHECK(rt_guide_cast_host(sc, nullptr, 0, nullptr) == RT_OK);
  CHECK(rt_guide_cast_host(nullptr, &rays[0][0], 1, hits.data()) == RT_ERR_ARG);
  CHECK(rt_guide_cast_host(sc, &rays[0][0], -1, hits.data()) == RT_ERR_ARG);
  CHECK(rt_guide_render_host(sc, 0, 3, nullptr, nullptr, nullptr, nullptr) == RT_ERR_ARG);
  s.objects[(size_t)o_bvh].b = 1;  // rows below what the format allows
  CHECK(rt_guide_cast_host(sc, &rays[0][0], 1, hits.data()) == RT_ERR_SCENE);
  s.objects[(size_t)o_bvh].b = 2;

  // the guided denoise on images smaller than a window, a patch and a noise tile, with the scene's own planes
  const int cases[][4] = {{5, 3, 10, 3}, {1, 1, 10, 3}, {7, 2, 10, 0}, {2, 9, 4, 2}, {19, 17, 0, 3}, {23, 19, 3, 1}};
  unsigned seed = 2026;
  auto next = [&]() { return (seed = seed * 1664525u + 1013904223u) >> 24; };  // 0..255
  for (const auto& z : cases) {
    const int W = z[0], H = z[1];
    const size_t px = (size_t)W * H, nv = 3 * px;
    std::vector<float> nrm(nv), alb(nv), dep(px);
    CHECK(rt_guide_render_host(sc, W, H, nrm.data(), alb.data(), dep.data(), nullptr) == RT_OK);
    rt_accum_info info = {};
    info.args.width = W, info.args.height = H, info.args.spp = 1, info.args.fb_count = 5, info.args.max_depth = 50;
    info.args.band_rows = H, info.args.band_stride = 1;
    info.n_values = (int64_t)nv;
    std::vector<uint32_t> s1(nv);
    std::vector<uint64_t> s2(nv);
    for (size_t k = 0; k < nv; ++k) {
      uint64_t a = 0, b = 0;
      for (int f = 0; f < 5; ++f) {
        const uint64_t c = k % 7 == 0 ? 255 : next();
        a += c * c, b += c * c * c * c;
      }
      s1[k] = (uint32_t)a, s2[k] = b;
    }
    size_t need = 0;
    CHECK(rt_noise_blob_pack(&info, nullptr, nullptr, nullptr, 0, &need) == RT_OK);
    std::vector<unsigned char> blob(need);
    CHECK(rt_noise_blob_pack(&info, s1.data(), s2.data(), blob.data(), need, nullptr) == RT_OK);
    rt_denoise_params p;
    rt_denoise_params_default(&p);
    p.search_radius = z[2], p.patch_radius = z[3];
    rt_guide_params g;
    rt_guide_params_default(&g);
    std::vector<uint8_t> out(nv, 0xAB), plain(nv), again(nv);
    std::vector<float> gain(px, -1.0f), gain0(px);
    CHECK(rt_guide_denoise_monitor_blob(blob.data(), need, &p, &g, nrm.data(), alb.data(), dep.data(), W, H, out.data(), gain.data()) == RT_OK);
    CHECK(rt_guide_denoise_monitor_blob(blob.data(), need, &p, nullptr, nrm.data(), alb.data(), dep.data(), W, H, again.data(), nullptr) == RT_OK);
    CHECK(again == out);
    CHECK(rt_denoise_monitor_blob(blob.data(), need, &p, plain.data(), gain0.data()) == RT_OK);
    for (size_t k = 0; k < px; ++k) CHECK(gain[k] >= 1.0f && gain[k] <= gain0[k]);
    // refusals leave the outputs alone
    std::vector<uint8_t> keep(nv, 0xCD);
    g.depth_gain = -1.0f;
    CHECK(rt_guide_denoise_monitor_blob(blob.data(), need, &p, &g, nrm.data(), alb.data(), dep.data(), W, H, keep.data(), nullptr) == RT_ERR_ARG);
    g.depth_gain = 1.0f;
    CHECK(rt_guide_denoise_monitor_blob(blob.data(), need, &p, &g, nrm.data(), alb.data(), dep.data(), W + 1, H, keep.data(), nullptr) == RT_ERR_ARG);
    CHECK(rt_guide_denoise_monitor_blob(blob.data(), need, &p, &g, nrm.data(), nullptr, dep.data(), W, H, keep.data(), nullptr) == RT_ERR_ARG);
    CHECK(rt_guide_denoise_adaptive_blob(blob.data(), need, &p, &g, nrm.data(), alb.data(), dep.data(), W, H, keep.data(), nullptr) == RT_ERR_ARG);
    for (uint8_t v : keep) CHECK(v == 0xCD);
  }
  printf("check_guide_host ok\n");
  return 0;
}
