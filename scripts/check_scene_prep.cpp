// check_scene_prep.cpp -- scene preparation (csrc/rt_scene_prep.cpp) in a stand-alone program, the one a
// sanitizer build runs.  Cases: the eleven asset-free built-in scenes, and earth, door and final over synthetic
// assets (a 9x5 RGB image, no multiple of the 8x8 texel tile, and a mesh of 12 triangles whose last four repeat
// the first four bit for bit).  Each case runs under the default options and under every single upload-time option
// that changes its output.  Per run: (a) one digest line on stdout (tests/golden/prep_digests.txt pins them) --
// byte count and FNV-1a-64 of every array rt_scene_upload copies, in its order, then its scalars; (b) the
// invariants of check_run() below; exit status 1 when one fails.  _Float16 needs clang++:
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Iinclude -Iraytracing_gpu_amd/csrc \
//       scripts/check_scene_prep.cpp raytracing_gpu_amd/csrc/rt_scene_prep.cpp raytracing_gpu_amd/csrc/rt_scene.cpp \
//       raytracing_gpu_amd/csrc/rt_obj.cpp raytracing_gpu_amd/csrc/rt_image.cpp raytracing_gpu_amd/csrc/rt_validate.cpp \
//       -o check_scene_prep && ./check_scene_prep
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "rt_hip.h"
#include "rt_host_geom.h"
#include "rt_scene_prep.h"

#define CHECK(x)                                                                     \
  do {                                                                               \
    if (!(x)) {                                                                      \
      printf("check_scene_prep: %s: line %d: %s\n", g_run.c_str(), __LINE__, #x);    \
      return false;                                                                  \
    }                                                                                \
  } while (0)

namespace {

std::string g_run;  // "case/option" of the run being checked

// ------------------------------------------------------------------ synthetic assets
struct Assets {
  std::vector<uint8_t> texels;
  std::vector<float> mesh;
  rt_image_asset image;
  rt_mesh_asset mesh_asset;
  rt_scene_assets all;
  Assets() {
    const int W = 9, H = 5;
    for (int i = 0; i < W * H * 3; ++i) texels.push_back((uint8_t)(i * 37 + 11));
    image = rt_image_asset{W, H, 3, 0, texels.data()};
    for (int k = 0; k < 12; ++k) {  // triangles 8..11 repeat 0..3
      const float t = (float)(k < 8 ? k : k - 8);
      const float v[9] = {0.25f * t - 1.0f, 0.125f * t,        0.5f * t - 2.0f,  0.25f * t - 0.5f, 0.125f * t + 0.25f,
                          0.5f * t - 1.75f, 0.25f * t - 0.75f, 0.125f * t + 1.0f, 0.5f * t - 2.0f};
      const float n[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1}, uv[6] = {0, 0, 1, 0, 0.5f, 1};
      mesh.insert(mesh.end(), v, v + 9);
      mesh.insert(mesh.end(), n, n + 9);
      mesh.insert(mesh.end(), uv, uv + 6);
    }
    mesh_asset = rt_mesh_asset{12, 1, 0, 0, mesh.data()};
    all = rt_scene_assets{1, 1, &image, &mesh_asset};
  }
};

// ------------------------------------------------------------------ digest
uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 0x100000001b3ull;
  return h;
}

template <class T>
void put(std::string& line, const T* p, size_t n) {  // as upload(): an empty array is no buffer
  if (n == 0) return;
  char buf[64];
  snprintf(buf, sizeof(buf), " %zu:%016llx", n * sizeof(T), (unsigned long long)fnv1a(p, n * sizeof(T)));
  line += buf;
}

std::string digest(const rt_scene_soa* s, const rtprep::Prepared& P) {
  std::string line;
  put(line, s->world, (size_t)s->n_world);
  put(line, P.objects.data(), P.objects.size());
  put(line, P.prims.data(), P.prims.size());
  put(line, s->triangles, (size_t)s->n_triangles);
  put(line, P.nodes.data(), P.nodes.size());
  put(line, s->materials, (size_t)s->n_materials);
  put(line, P.pmargin.data(), P.pmargin.size());
  put(line, P.pvalid.data(), P.pvalid.size());
  put(line, s->textures, (size_t)s->n_textures);
  put(line, s->perlins, (size_t)s->n_perlins);
  put(line, P.images.data(), P.images.size());
  put(line, P.texels.data(), P.texels.size());
  put(line, P.wleaf.data(), P.wleaf.size());
  put(line, P.wxf.data(), P.wxf.size());
  put(line, P.worder.data(), P.worder.size());
  put(line, P.qnodes.data(), P.qnodes.size());
  put(line, P.bin_sph.data(), P.bin_sph.size());
  put(line, P.bin_ids.data(), P.bin_ids.size());
  char buf[256];
  snprintf(buf, sizeof(buf),
           " wt_fb=%d w_media=%d w_inert=%d merge_ok=%d q_pairs=%d q_ebias=%d features=%d world_bvh=%d world_step=%d"
           " world_tree=%d bin_n=%d plane_fb=%d plane_pairs=%d",
           P.wt_fb, P.w_media, P.w_inert, P.merge_ok, P.q_pairs, P.q_ebias, P.features, (int)P.world_bvh,
           (int)P.world_step, (int)P.world_tree, P.bin_n, P.plane_fb, P.plane_pairs);
  return line + buf;
}

// ------------------------------------------------------------------ invariants
int32_t bits(float f) {
  int32_t i;
  memcpy(&i, &f, 4);
  return i;
}

// The box that bounds primitive id over the ordered shutter (an xz_rect's reference box spans z1 only).
rth::Box geom_box(const rt_scene_soa* s, int id) {
  const float a = s->camera.time0, b = s->camera.time1;
  const rt_prim& q = s->prims[id];
  rth::Box box = rth::prim_box(q, s->triangles, a < b ? a : b, a < b ? b : a);
  if ((q.type & 0xff) == RT_PRIM_RECT_XZ) box.lo[2] = std::fmin(q.p[2], q.p[3]), box.hi[2] = std::fmax(q.p[2], q.p[3]);
  return box;
}

const rth::Box kEmpty = {{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};  // join's identity

bool inside(const rth::Box& in, const float* lo, const float* hi) {
  for (int a = 0; a < 3; ++a)
    if (!(lo[a] <= in.lo[a] && hi[a] >= in.hi[a])) return false;
  return true;
}

// Walks the traversal tree of `records` pair records at nodes[fb]: every record reached once, every stored child
// box around the boxes of the leaves below it.  leaf(child word) -> the leaf's box; seen counts the leaves.
struct TreeWalk {
  const std::vector<rt_bvh_node>& nodes;
  int fb, records;
  std::function<rth::Box(int)> leaf_box;
  std::map<int, int> leaves;  // leaf -> times reached
  std::vector<int> visits;
  bool ok = true;
  rth::Box walk(int rec) {
    if (rec < 0 || rec >= records || visits[(size_t)rec]++) {
      ok = false;
      return rth::Box{{0, 0, 0}, {0, 0, 0}};
    }
    const rt_bvh_node* r = &nodes[(size_t)fb + 2 * (size_t)rec];
    const int child[2] = {r[0].leaf_a, r[0].leaf_b};
    rth::Box out{};
    for (int c = 0; c < 2; ++c) {
      rth::Box b;
      if (child[c] < 0) {
        ++leaves[-child[c] - 1];
        b = leaf_box(-child[c] - 1);
        // A sphere of negative radius ("first": the hollow glass sphere) has the reference's own inverted box
        // (sphere.h:75-78, lo > hi), which bounds nothing and which no box contains: it counts as empty here.
        if (b.lo[0] > b.hi[0] || b.lo[1] > b.hi[1] || b.lo[2] > b.hi[2]) b = kEmpty;
      } else {
        b = walk(child[c]);
      }
      const float lo[3] = {c ? r[1].lo[0] : r[0].lo[0], c ? r[1].lo[1] : r[0].lo[1], c ? r[1].lo[2] : r[0].lo[2]};
      const float hi[3] = {c ? r[1].hi[0] : r[0].hi[0], c ? r[1].hi[1] : r[0].hi[1], c ? r[1].hi[2] : r[0].hi[2]};
      if (!inside(b, lo, hi)) ok = false;
      out = c ? rth::join(out, b) : b;
    }
    return out;
  }
  bool run() {
    if (records < 1 || (size_t)fb + 2 * (size_t)records > nodes.size()) return false;
    visits.assign((size_t)records, 0);
    walk(0);
    for (int v : visits) ok = ok && v == 1;
    return ok;
  }
};

// The reference's depth-first left-first order over the perfect tree of `rows` inner levels: calls f(primitive,
// slot) with slot counting every leaf slot of the last row, empty ones too.
void ref_dfs(const rt_scene_soa* s, int base, int rows, int k, int level, int& slot, const std::function<void(int, int)>& f) {
  if (level == rows - 1) {
    for (int id : {s->nodes[base + k].leaf_a, s->nodes[base + k].leaf_b}) {
      if (id >= 0) f(id, slot);
      ++slot;
    }
    return;
  }
  ref_dfs(s, base, rows, 2 * k + 1, level + 1, slot, f);
  ref_dfs(s, base, rows, 2 * k + 2, level + 1, slot, f);
}

// The camera-bin bounding spheres (P.bin_sph), in double.  A sphere contains a box when it contains its corners.
struct Pt {
  double x[3];
};
void corners(const rth::Box& b, std::vector<Pt>& out) {
  for (int q = 0; q < 8; ++q)
    out.push_back(Pt{{(q & 1) ? b.hi[0] : b.lo[0], (q & 2) ? b.hi[1] : b.lo[1], (q & 4) ? b.hi[2] : b.lo[2]}});
}
bool sphere_contains(const rtprep::Float4& sp, const std::vector<Pt>& pts) {
  if (sp.w == INFINITY) return true;
  for (const Pt& p : pts) {
    const double d[3] = {p.x[0] - sp.x, p.x[1] - sp.y, p.x[2] - sp.z};
    if (!(std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) <= (double)sp.w)) return false;
  }
  return true;
}
// Corner points, in world space, of what object oi holds over the shutter: a primitive's box, the boxes of a
// list's or a BVH's primitives, a medium's boundary, and for an instance the eight corners of its child's box
// through translate(rotate_y(.)) (hittable.h: world = (c x + s z, y, -s x + c z) + offset).  false: no box.
bool object_corners(const rt_scene_soa* s, int oi, std::vector<Pt>& out, int depth = 0) {
  if (oi < 0 || oi >= s->n_objects || depth > 8) return false;
  const rt_object& o = s->objects[oi];
  switch (o.kind) {
    case RT_OBJ_PRIM:
      corners(geom_box(s, o.a), out);
      return true;
    case RT_OBJ_LIST:
      for (int k = 0; k < o.b; ++k) corners(geom_box(s, o.a + k), out);
      return o.b > 0;
    case RT_OBJ_BVH: {
      int slot = 0, n = 0;
      ref_dfs(s, o.a, o.b, 0, 0, slot, [&](int id, int) {
        corners(geom_box(s, id), out);
        ++n;
      });
      return n > 0;
    }
    case RT_OBJ_MEDIUM:
      return object_corners(s, o.a, out, depth + 1);
    case RT_OBJ_XFORM: {
      std::vector<Pt> child;
      if (!object_corners(s, o.a, child, depth + 1)) return false;
      double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (const Pt& p : child)
        for (int a = 0; a < 3; ++a) lo[a] = std::fmin(lo[a], p.x[a]), hi[a] = std::fmax(hi[a], p.x[a]);
      const double sn = (o.b & 2) ? o.f[3] : 0.0, cs = (o.b & 2) ? o.f[4] : 1.0;
      for (int q = 0; q < 8; ++q) {
        const double x = (q & 1) ? hi[0] : lo[0], y = (q & 2) ? hi[1] : lo[1], z = (q & 4) ? hi[2] : lo[2];
        Pt w{{cs * x + sn * z, y, -sn * x + cs * z}};
        if (o.b & 1)
          for (int a = 0; a < 3; ++a) w.x[a] += o.f[a];
        out.push_back(w);
      }
      return true;
    }
  }
  return false;
}

bool check_run(const rt_scene_soa* s, const rtprep::Options& opt, const rtprep::Prepared& P) {
  CHECK((int)P.prims.size() == s->n_prims && (int)P.objects.size() == s->n_objects);
  // the first node of each tree built here, in the order they were appended: each ends where the next begins
  std::vector<int> starts;
  for (const rt_object& o : P.objects)
    if (o.kind == RT_OBJ_BVH) starts.push_back(o.c);
  if (P.world_tree) starts.push_back(P.wt_fb);
  starts.push_back((int)P.nodes.size());
  CHECK(starts[0] == s->n_nodes);
  std::vector<int32_t> rank_of((size_t)s->n_prims, -1);
  size_t tree = 0;
  for (int k = 0; k < s->n_objects; ++k) {
    const rt_object& o = s->objects[k];
    if (o.kind != RT_OBJ_BVH) continue;
    // leaf ranks are the reference's depth-first order; members in that order
    std::vector<int> members;
    int slot = 0;
    bool ranks_ok = true;
    ref_dfs(s, o.a, o.b, 0, 0, slot, [&](int id, int at) {
      members.push_back(id);
      rank_of[(size_t)id] = at;
      ranks_ok = ranks_ok && bits(P.prims[(size_t)id].p[9]) == at;
    });
    CHECK(ranks_ok && slot == 1 << o.b);
    // with de-duplication the first member (the lowest rank) of each group of coincident triangles stands for it
    std::vector<int> expect;
    std::map<std::string, int> first_of;
    for (int id : members) {
      if (opt.dedup_triangles && (s->prims[id].type & 0xff) == RT_PRIM_TRIANGLE) {
        const rt_triangle& t = s->triangles[(int)s->prims[id].p[0]];
        std::string key((const char*)t.v0, 12);
        key.append((const char*)t.e0, 12).append((const char*)t.e1, 12);
        const auto it = first_of.find(key);
        if (it != first_of.end()) {
          CHECK(rank_of[(size_t)it->second] < rank_of[(size_t)id]);
          continue;
        }
        first_of[key] = id;
      }
      expect.push_back(id);
    }
    if (expect.size() < 2) expect = members;
    // leaves - 1 records, every kept leaf reached exactly once, child boxes around the leaves below
    const int fb = P.objects[(size_t)k].c;
    CHECK(fb == starts[tree] && (starts[tree + 1] - fb) % 2 == 0);
    TreeWalk w{P.nodes, fb, (starts[tree + 1] - fb) / 2, [&](int id) { return geom_box(s, id); }, {}, {}};
    ++tree;
    CHECK(w.records == (int)expect.size() - 1);
    CHECK(w.run());
    CHECK(w.leaves.size() == expect.size());
    for (int id : expect) CHECK(w.leaves.count(id) == 1 && w.leaves[id] == 1);
  }
  for (int id = 0; id < s->n_prims; ++id) CHECK(bits(P.prims[(size_t)id].p[9]) == rank_of[(size_t)id]);

  if (P.world_tree) {  // tie keys (n_world - 1 - entry) << 20 | rank; a tree over every leaf
    const int n = (int)P.wleaf.size() / 4;
    CHECK(n >= 2 && P.wleaf.size() == 4 * (size_t)n && P.wt_fb == starts[tree]);
    for (int i = 0; i < n; ++i) {
      rt_prim q;
      int32_t d[4];  // instance, world entry, reference BVH object or -1, primitive
      memcpy(&q, &P.wleaf[4 * (size_t)i], sizeof(q));
      memcpy(d, &P.wleaf[4 * (size_t)i + 3], sizeof(d));
      CHECK(d[1] >= 0 && d[1] < s->n_world && d[3] >= 0 && d[3] < s->n_prims);
      const int rank = d[2] >= 0 ? rank_of[(size_t)d[3]] : 0;
      CHECK(bits(q.p[9]) == (((s->n_world - 1 - d[1]) << RT_WKEY_SHIFT) | rank));
      CHECK(((q.type & RT_PRIM_FLAG_XF) != 0) == (d[0] >= 0));
    }
    // (an instance's leaves have world-space boxes through its transform: not re-derived here, an empty box)
    TreeWalk w{P.nodes, P.wt_fb, ((int)P.nodes.size() - P.wt_fb) / 2, [&](int i) {
                 const int32_t xf = bits(P.wleaf[4 * (size_t)i + 3].x), prim = bits(P.wleaf[4 * (size_t)i + 3].w);
                 return xf < 0 ? geom_box(s, prim) : kEmpty;
               }, {}, {}};
    CHECK(w.records == n - 1);
    CHECK(w.run());
    CHECK((int)w.leaves.size() == n);
    for (int i = 0; i < n; ++i) CHECK(w.leaves[i] == 1);
  } else {
    CHECK(P.wleaf.empty());
  }

  if (P.q_pairs > 0) {  // every quantized child box, decoded, contains the float box; child words round-trip
    CHECK(P.world_step && P.qnodes.size() == 6 * (size_t)P.q_pairs);
    const int fb = P.objects[(size_t)s->world[0]].c;
    for (int i = 0; i < P.q_pairs; ++i) {
      const uint32_t* w = &P.qnodes[6 * (size_t)i];
      const rt_bvh_node* r = &P.nodes[(size_t)fb + 2 * (size_t)i];
      const uint16_t org[3] = {(uint16_t)w[0], (uint16_t)(w[0] >> 16), (uint16_t)w[1]};
      uint8_t b[12];
      memcpy(b, &w[2], 12);
      for (int a = 0; a < 3; ++a) {
        _Float16 h;
        memcpy(&h, &org[a], 2);
        const double o = (double)(float)h, sc = std::ldexp(1.0, (int)((w[1] >> (16 + 5 * a)) & 31u) + P.q_ebias);
        for (int ch = 0; ch < 2; ++ch)
          CHECK(o + b[6 * ch + a] * sc <= (double)r[ch].lo[a] && o + b[6 * ch + 3 + a] * sc >= (double)r[ch].hi[a]);
      }
      CHECK((int16_t)(w[5] & 0xffffu) == r[0].leaf_a && (int16_t)(w[5] >> 16) == r[0].leaf_b);
    }
  } else {
    CHECK(P.qnodes.empty());
  }

  {  // worder is a permutation of the world's entries
    std::vector<int> seen((size_t)s->n_world, 0);
    CHECK((int)P.worder.size() == s->n_world);
    for (int32_t w : P.worder) CHECK(w >= 0 && w < s->n_world && !seen[(size_t)w]++);
  }

  // Camera-bin bounding spheres: a sphere contains what it stands for (the camera tile lists and entry masks
  // drop whatever lies outside a tile's frustum by more than its sphere's radius).
  if (P.world_bvh) {  // one per leaf of the world BVH, in the reference's depth-first order
    const rt_object& o = s->objects[s->world[0]];
    std::vector<int> members;
    int slot = 0;
    ref_dfs(s, o.a, o.b, 0, 0, slot, [&](int id, int) { members.push_back(id); });
    CHECK(P.bin_n == (int)members.size() && P.bin_ids.size() == members.size() && P.bin_sph.size() == members.size());
    for (size_t q = 0; q < members.size(); ++q) {
      CHECK(P.bin_ids[q] == members[q]);
      const rtprep::Float4& sp = P.bin_sph[q];
      const rth::Box b = geom_box(s, members[q]);
      std::vector<Pt> pts;
      corners(b, pts);
      CHECK(sphere_contains(sp, pts));
      // ... and is no looser than box_sphere's 1e-6 terms allow, with a tenfold margin
      const double h[3] = {0.5 * ((double)b.hi[0] - b.lo[0]), 0.5 * ((double)b.hi[1] - b.lo[1]), 0.5 * ((double)b.hi[2] - b.lo[2])};
      const double half_diag = std::sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
      const double c1 = std::fabs((double)sp.x) + std::fabs((double)sp.y) + std::fabs((double)sp.z);
      CHECK((double)sp.w - half_diag <= 1e-5 * ((double)sp.w + c1));
    }
  } else {  // one per top-level entry (the first 32): around the entry's box, or unbounded
    CHECK(P.bin_ids.empty() && P.bin_n == -(int)P.bin_sph.size() && (int)P.bin_sph.size() == (s->n_world < 32 ? s->n_world : 32));
    for (size_t w = 0; w < P.bin_sph.size(); ++w) {
      std::vector<Pt> pts;
      if (object_corners(s, s->world[w], pts)) CHECK(sphere_contains(P.bin_sph[w], pts));
      else CHECK(P.bin_sph[w].w == INFINITY);
    }
  }

  if (P.plane_fb >= 0) {  // only the last tree of nodes, of at most kPlanePairs records
    CHECK(P.world_step && P.plane_fb == P.objects[(size_t)s->world[0]].c);
    CHECK(P.plane_pairs >= 1 && P.plane_pairs <= rtprep::kPlanePairs);
    CHECK(P.plane_fb + 2 * P.plane_pairs == (int)P.nodes.size());
  }

  CHECK((int)P.images.size() == s->n_images);
  for (int k = 0; k < s->n_images; ++k) {  // every tiled texel equals its source texel
    const rt_image &src = s->images[k], &im = P.images[(size_t)k];
    if (src.width <= 0) continue;
    CHECK(im.bytes_per_pixel >= 3 && im.width == src.width && im.height == src.height);
    const int tpr = (im.width + 7) >> 3;
    for (int j = 0; j < im.height; ++j)
      for (int i = 0; i < im.width; ++i) {
        const size_t at = (size_t)im.offset +
                          ((((size_t)(j >> 3) * tpr + (i >> 3)) << 6) + ((j & 7) << 3) + (i & 7)) * im.bytes_per_pixel;
        CHECK(at + 3 <= P.texels.size());
        CHECK(!memcmp(&P.texels[at], s->texels + src.offset + ((size_t)j * src.width + i) * src.bytes_per_pixel, 3));
      }
  }
  CHECK(P.pmargin.size() % 2 == 0 && P.pvalid.size() == 3 * (size_t)s->n_prims);
  return true;
}

}  // namespace

int main() {
  const char* cases[] = {"basic", "first", "big1", "two_spheres", "two_perlin", "cornell", "cornell_smoke",
                         "triangle", "triangles", "coincident", "coincident_step", "earth", "door", "final"};
  struct Variant {
    const char* name;
    rtprep::Options opt;  // dedup_triangles, world_tree, quantized_tree, merged_search, merge_order
  };
  const Variant variants[] = {
      {"default", {1, 0, 1, RT_MERGE_ON, RT_ORDER_DISTANCE}},
      {"world_tree=1", {1, 1, 1, RT_MERGE_ON, RT_ORDER_DISTANCE}},
      {"dedup_triangles=0", {0, 0, 1, RT_MERGE_ON, RT_ORDER_DISTANCE}},
      {"quantized_tree=0", {1, 0, 0, RT_MERGE_ON, RT_ORDER_DISTANCE}},
      {"merged_search=off", {1, 0, 1, RT_MERGE_OFF, RT_ORDER_DISTANCE}},
      {"merged_search=fallback_all", {1, 0, 1, RT_MERGE_FALLBACK_ALL, RT_ORDER_DISTANCE}},
      {"merge_order=list", {1, 0, 1, RT_MERGE_ON, RT_ORDER_LIST}},
      {"merge_order=reversed", {1, 0, 1, RT_MERGE_ON, RT_ORDER_REVERSED}},
  };
  const Assets assets;
  int failed = 0;
  for (const char* name : cases) {
    rt_scene_host* host = nullptr;
    char msg[160] = "";
    if (rt_scene_build_ex(name, &assets.all, &host) != RT_OK || !host) {
      printf("check_scene_prep: %s: build failed\n", name);
      return 1;
    }
    const rt_scene_soa* s = rt_scene_view(host);
    if (rt_scene_validate(s, msg, sizeof(msg)) != RT_OK) {
      printf("check_scene_prep: %s: %s\n", name, msg);
      return 1;
    }
    std::string base;
    for (const Variant& v : variants) {
      g_run = std::string(name) + "/" + v.name;
      rtprep::Prepared P;
      std::string why;
      const int rc = rtprep::prepare(s, v.opt, P, why);
      if (rc != RT_OK) {
        printf("check_scene_prep: %s: prepare: %d %s\n", g_run.c_str(), rc, why.c_str());
        return 1;
      }
      const std::string line = digest(s, P);
      if (&v == variants) base = line;
      else if (line == base) continue;  // the option changes nothing of this scene
      printf("%s:%s\n", g_run.c_str(), line.c_str());
      if (!check_run(s, v.opt, P)) ++failed;
    }
    rt_scene_free(host);
  }
  return failed ? 1 : 0;
}
