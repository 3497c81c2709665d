// rt_scene_prep.cpp -- host-only: what rt_scene_upload (rt_kernels.hip) computes before it copies a scene
// to the device.  The traversal trees of the reference BVHs with their chain margins and triangle
// de-duplication, the world tree, the quantized tree, object boxes, inert media, texel tiling,
// world_search's visiting order, the camera-bin spheres and the scene's feature mask.  No HIP header:
// scripts/check_scene_prep.cpp runs this file under a sanitizer and pins its output
// (tests/test_prep_cpu.py, tests/golden/prep_digests.txt).
#include "rt_scene_prep.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <set>

#include "rt_host_geom.h"

namespace rtprep {
namespace {

// The camera's shutter interval, ordered.
struct Shutter {
  float t0, t1;
};
Shutter shutter(const rt_scene_soa* s) {
  const float t0 = s->camera.time0, t1 = s->camera.time1;
  return Shutter{t0 < t1 ? t0 : t1, t0 < t1 ? t1 : t0};
}

// Calls f(primitive, rank) for every leaf of the reference BVH of `rows` inner levels at nodes[base]: the
// last row's nodes hold the leaves, and rank is a leaf's position in the reference's depth-first
// left-first order.
template <class F>
void for_each_leaf(const rt_scene_soa* s, int base, int rows, F f) {
  const int inner = (1 << rows) - 1, last0 = (1 << (rows - 1)) - 1;
  for (int k = last0; k < inner; ++k) {
    const int ids[2] = {s->nodes[base + k].leaf_a, s->nodes[base + k].leaf_b};
    for (int q = 0; q < 2; ++q)
      if (ids[q] >= 0) f(ids[q], 2 * (k - last0) + q);
  }
}

int scene_features(const rt_scene_soa* s) {
  int f = 0;
  for (int k = 0; k < s->n_prims; ++k) {
    const int t = s->prims[k].type;
    if (t == RT_PRIM_MOVING_SPHERE) f |= F_MOVING;
    if ((t >= RT_PRIM_RECT_XY && t <= RT_PRIM_RECT_YZ) || t == RT_PRIM_BOX) f |= F_RECT;
    if (t == RT_PRIM_TRIANGLE) f |= F_TRI;
  }
  for (int k = 0; k < s->n_objects; ++k) {
    const int t = s->objects[k].kind;
    if (t == RT_OBJ_LIST) f |= F_LIST;
    if (t == RT_OBJ_BVH) f |= F_BVH;
    if (t == RT_OBJ_XFORM) f |= F_XFORM;
    if (t == RT_OBJ_MEDIUM) f |= F_MEDIUM;
  }
  for (int k = 0; k < s->n_textures; ++k) {
    const int t = s->textures[k].type;
    if (t == RT_TEX_CHECKER) f |= F_CHECKER;
    if (t == RT_TEX_NOISE || t == RT_TEX_TURBULENT || t == RT_TEX_MARBLE) f |= F_NOISE;
    if (t == RT_TEX_IMAGE) f |= F_IMAGE;
  }
  return f;
}

bool tex_needs_uv(const rt_scene_soa* s, int ti) {
  if (ti < 0 || ti >= s->n_textures) return false;
  const rt_texture& t = s->textures[ti];
  if (t.type == RT_TEX_IMAGE) return true;
  if (t.type == RT_TEX_CHECKER) {
    for (int c : {t.a, t.b})
      if (c >= 0 && c < s->n_textures && s->textures[c].type == RT_TEX_IMAGE) return true;
  }
  return false;
}

// Traversal tree of a reference BVH (see bvh_closest): a binary SAH tree over the same
// primitives, one primitive per leaf, child boxes stored in the parent (padded by 2^-16 relative
// so a primitive hit is never outside its padded ancestors).  Record i = 2 rt_bvh_node slots at
// nodes[fb + 2i]: {lo0, child0}, {hi0, child1}, {lo1, -}, {hi1, -}; child >= 0 is a record,
// child < 0 the primitive -child-1.  Also writes each primitive's reference leaf rank (its
// position in the reference's depth-first left-first order) into prims[].p[9].
// Returns the first node index of the new tree in `nodes` (rt_scene_validate has checked the reference tree).
struct SahBuilder {
  const std::vector<rth::Box>& box;
  std::vector<rt_bvh_node>& nodes;
  int fb;
  static float area(const rth::Box& b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return dx < 0.0f ? 0.0f : 2.0f * (dx * dy + dy * dz + dz * dx);
  }
  static rth::Box pad(rth::Box b) {
    for (int a = 0; a < 3; ++a) {
      const float p = (std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a])) + (b.hi[a] - b.lo[a])) * (1.0f / 65536.0f);
      b.lo[a] -= p;
      b.hi[a] += p;
    }
    return b;
  }
  rth::Box bounds(const int* ids, int n) const {
    rth::Box b = box[ids[0]];
    for (int i = 1; i < n; ++i) b = rth::join(b, box[ids[i]]);
    return b;
  }
  // Builds the subtree over ids[0..n) (n >= 2) as record `me`; returns nothing.
  void build(int* ids, int n, int me) {
    float best = INFINITY;
    int bax = 0, bsplit = n / 2;
    std::vector<float> right(n + 1);
    for (int ax = 0; ax < 3; ++ax) {
      auto key = [&](int id) { return box[id].lo[ax] + box[id].hi[ax]; };
      std::stable_sort(ids, ids + n, [&](int x, int y) { return key(x) < key(y); });
      rth::Box acc = box[ids[n - 1]];
      for (int i = n - 1; i >= 1; --i) {
        if (i < n - 1) acc = rth::join(acc, box[ids[i]]);
        right[i] = area(acc) * (float)(n - i);
      }
      rth::Box lacc = box[ids[0]];
      for (int i = 1; i < n; ++i) {
        if (i > 1) lacc = rth::join(lacc, box[ids[i - 1]]);
        const float cost = area(lacc) * (float)i + right[i];
        if (cost < best) {
          best = cost;
          bax = ax;
          bsplit = i;
        }
      }
    }
    auto key = [&](int id) { return box[id].lo[bax] + box[id].hi[bax]; };
    std::stable_sort(ids, ids + n, [&](int x, int y) { return key(x) < key(y); });
    int child[2];
    rth::Box cb[2];
    const int part[2][2] = {{0, bsplit}, {bsplit, n}};
    for (int c = 0; c < 2; ++c) {
      const int* cid = ids + part[c][0];
      const int cn = part[c][1] - part[c][0];
      cb[c] = pad(bounds(cid, cn));
      if (cn == 1) {
        child[c] = -cid[0] - 1;
      } else {
        child[c] = (int)(nodes.size() - fb) / 2;
        nodes.resize(nodes.size() + 2);
      }
    }
    rt_bvh_node* r = &nodes[fb + 2 * me];
    for (int a = 0; a < 3; ++a) {
      r[0].lo[a] = cb[0].lo[a];
      r[0].hi[a] = cb[0].hi[a];
      r[1].lo[a] = cb[1].lo[a];
      r[1].hi[a] = cb[1].hi[a];
    }
    r[0].leaf_a = child[0];
    r[0].leaf_b = child[1];
    r[1].leaf_a = 0;
    r[1].leaf_b = 0;
    for (int c = 0; c < 2; ++c)
      if (child[c] >= 0) build(ids + part[c][0], part[c][1] - part[c][0], child[c]);
  }
};

// Geometric box of a primitive over the shutter: bounding_box() (rth::prim_box) except for the
// xz_rect, whose reference box spans z1 only (aarect.h:39, H4) and so does not bound the rect.
rth::Box geom_box(const rt_prim& q, const rt_triangle* tris, float t0, float t1) {
  rth::Box b = rth::prim_box(q, tris, t0, t1);
  if ((q.type & 0xff) == RT_PRIM_RECT_XZ) {
    b.lo[2] = std::fmin(q.p[2], q.p[3]);
    b.hi[2] = std::fmax(q.p[2], q.p[3]);
  }
  return b;
}

int build_traversal_tree(const rt_scene_soa* s, int base, int rows, std::vector<rt_prim>& prims,
                         std::vector<rt_bvh_node>& nodes, std::vector<Float2>& pmargin, std::vector<Float4>& pvalid,
                         int* n_pairs, bool dedup) {
  std::vector<int> members;
  for_each_leaf(s, base, rows, [&](int id, int32_t rank) {
    memcpy(&prims[id].p[9], &rank, 4);
    members.push_back(id);
  });
  const Shutter sh = shutter(s);
  std::vector<rth::Box> box(s->n_prims);
  // (the geometric box: the reference's xz_rect box spans z1 only, H4, and where the stored boxes are not
  // the reference's own a search tree built from it would miss the rect where the stored boxes show it)
  for (int id : members) box[id] = geom_box(prims[id], s->triangles, sh.t0, sh.t1);
  // Safety margins of each primitive's reference chain: margin of chain position j = smallest
  // distance from the primitive's box (over the camera shutter) to the faces of its j-th
  // reference ancestor (position 0 = its last-row node).  Stored as {bitmask of positions with
  // margin < 0.05 (always tested), smallest margin of the other positions}.
  for_each_leaf(s, base, rows, [&](int id, int rank) {
    const int k = (1 << (rows - 1)) - 1 + rank / 2;  // the leaf's last-row node
    uint32_t mask = 0;
    float safe = INFINITY;
    int pos = 0;
    for (int a = k;; a = (a - 1) >> 1, ++pos) {
      const rt_bvh_node& an = s->nodes[base + a];
      float mm = INFINITY;
      for (int q = 0; q < 3; ++q) mm = std::min(mm, std::min(box[id].lo[q] - an.lo[q], an.hi[q] - box[id].hi[q]));
      if (!(mm >= 0.05f)) mask |= 1u << pos;
      else safe = std::min(safe, mm);
      if (!(mm >= 0.0f)) prims[id].type |= RT_PRIM_FLAG_OUT;  // chain_ok's own-box shortcut does not apply
      if (a == 0) break;
    }
    float mbits;
    memcpy(&mbits, &mask, 4);
    pmargin[id] = Float2{mbits, safe};
    // chain_ok's one-fetch record: the lowest `must` position's box, the mask, `safe`, and the largest
    // |coordinate| over the `must` ancestors' boxes.  Only when every `must` ancestor contains the
    // lowest one's box (the reference's surrounding boxes always do); else safe = -inf turns it off.
    int low = k;  // node of the lowest must position
    for (int q = 0; mask != 0u && q < __builtin_ctz(mask); ++q) low = (low - 1) >> 1;
    const rt_bvh_node& ln = s->nodes[base + low];
    float rmax = 0.0f, vsafe = safe;
    pos = 0;
    for (int a = k;; a = (a - 1) >> 1, ++pos) {
      if ((mask >> pos) & 1u) {
        const rt_bvh_node& an = s->nodes[base + a];
        for (int q = 0; q < 3; ++q) {
          rmax = std::fmax(rmax, std::fmax(std::fabs(an.lo[q]), std::fabs(an.hi[q])));
          if (!(an.lo[q] <= ln.lo[q] && an.hi[q] >= ln.hi[q])) vsafe = -INFINITY;
        }
      }
      if (a == 0) break;
    }
    if (!(rmax < INFINITY)) vsafe = -INFINITY;
    pvalid[3 * (size_t)id] = Float4{ln.lo[0], ln.lo[1], ln.lo[2], mbits};
    pvalid[3 * (size_t)id + 1] = Float4{ln.hi[0], ln.hi[1], ln.hi[2], vsafe};
    pvalid[3 * (size_t)id + 2] = Float4{rmax, 0.0f, 0.0f, 0.0f};
  });
  // Coincident triangles (the reference's mesh import indexes the concatenated vertex array with
  // per-mesh local indices, H16: 1 828 of the door's 4 330 triangles repeat an earlier one's v0, e0,
  // e1 bit for bit) hit every ray at the same t, so among them the reference keeps the first it
  // visits in its depth-first left-first order: the lowest leaf rank whose chain passes.  The
  // candidate search only needs that member; members are in rank order, so the first of each group
  // stays in the tree.  The settle validates the kept member's chain; if it fails the query re-runs
  // on the exact visit set, where a later member may win (options.dedup_triangles = 0 keeps every member).
  std::vector<int> kept;
  if (dedup) {
    std::set<std::array<uint32_t, 9>> seen;
    for (int id : members) {
      if ((prims[id].type & 0xff) == RT_PRIM_TRIANGLE) {
        const int ti = (int)prims[id].p[0];
        const rt_triangle& t = s->triangles[ti];
        std::array<uint32_t, 9> key;
        memcpy(&key[0], t.v0, 12);
        memcpy(&key[3], t.e0, 12);
        memcpy(&key[6], t.e1, 12);
        if (!seen.insert(key).second) continue;
      }
      kept.push_back(id);
    }
  }
  std::vector<int>& leaves = kept.size() >= 2 ? kept : members;
  const int fb = (int)nodes.size();
  nodes.resize(fb + 2);  // record 0 = root
  SahBuilder sb{box, nodes, fb};
  sb.build(leaves.data(), (int)leaves.size(), 0);
  *n_pairs = (int)leaves.size() - 1;  // records of the tree (one per inner node): leaves - 1
  return fb;
}

// Bounding sphere (centre, radius) of a primitive box, rounded outward so that it contains the box.
Float4 box_sphere(const rth::Box& b) {
  const double cx = 0.5 * ((double)b.lo[0] + b.hi[0]), cy = 0.5 * ((double)b.lo[1] + b.hi[1]),
               cz = 0.5 * ((double)b.lo[2] + b.hi[2]);
  const double hx = 0.5 * ((double)b.hi[0] - b.lo[0]), hy = 0.5 * ((double)b.hi[1] - b.lo[1]),
               hz = 0.5 * ((double)b.hi[2] - b.lo[2]);
  const double rad = std::sqrt(hx * hx + hy * hy + hz * hz) * (1.0 + 1e-6) +
                     1e-6 * (std::fabs(cx) + std::fabs(cy) + std::fabs(cz)) + 1e-30;
  return Float4{(float)cx, (float)cy, (float)cz, (float)(rad * (1.0 + 1e-6))};
}
// World-space box of a child-frame box cb under instance o (translate(rotate_y(child))).
rth::Box xform_box(const rt_object& o, const rth::Box& cb) {
  // world = R^-1 (object) + offset, R^-1: x = c x' + s z', z = -s x' + c z' (hittable.h:112-143)
  const double sn = (o.b & 2) ? o.f[3] : 0.0, cs = (o.b & 2) ? o.f[4] : 1.0;
  const double off[3] = {(o.b & 1) ? o.f[0] : 0.0, (o.b & 1) ? o.f[1] : 0.0, (o.b & 1) ? o.f[2] : 0.0};
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int q = 0; q < 8; ++q) {
    const double x = (q & 1) ? cb.hi[0] : cb.lo[0], y = (q & 2) ? cb.hi[1] : cb.lo[1], z = (q & 4) ? cb.hi[2] : cb.lo[2];
    const double w[3] = {cs * x + sn * z + off[0], y + off[1], -sn * x + cs * z + off[2]};
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], w[k]);
      hi[k] = std::max(hi[k], w[k]);
    }
  }
  rth::Box out;
  for (int k = 0; k < 3; ++k) {  // widened for the float rounding of the instance transform
    const double pad = 1e-5 * (std::fabs(lo[k]) + std::fabs(hi[k]) + (hi[k] - lo[k])) + 1e-6;
    out.lo[k] = (float)(lo[k] - pad);
    out.hi[k] = (float)(hi[k] + pad);
  }
  return out;
}

// World-space box over the shutter [t0, t1] of object oi (an instance's child box through its
// rotate_y + translate, a medium's boundary); false when it cannot be bounded.
bool object_box(const rt_scene_soa* s, int oi, float t0, float t1, rth::Box& out, int depth = 0) {
  const rt_prim* prims = s->prims;  // the scene's records (the device copies hold triangle operands)
  if (oi < 0 || oi >= s->n_objects || depth > 8) return false;
  const rt_object& o = s->objects[oi];
  auto pbox = [&](int id) { return geom_box(prims[id], s->triangles, t0, t1); };
  switch (o.kind) {
    case RT_OBJ_PRIM:
      out = pbox(o.a);
      return true;
    case RT_OBJ_LIST:
      if (o.b <= 0) return false;
      out = pbox(o.a);
      for (int k = 1; k < o.b; ++k) out = rth::join(out, pbox(o.a + k));
      return true;
    case RT_OBJ_BVH: {
      bool any = false;
      for_each_leaf(s, o.a, o.b, [&](int id, int) {
        out = any ? rth::join(out, pbox(id)) : pbox(id);
        any = true;
      });
      return any;
    }
    case RT_OBJ_MEDIUM:
      return object_box(s, o.a, t0, t1, out, depth + 1);
    case RT_OBJ_XFORM: {
      rth::Box cb;
      if (!object_box(s, o.a, t0, t1, cb, depth + 1)) return false;
      out = xform_box(o, cb);
      return true;
    }
  }
  return false;
}

// World tree (F_WORLD): a list world (hittable_list.h:23-39) of primitives, BVHs and translate /
// rotate_y instances of them, followed by constant media, flattened into ONE traversal tree over
// every primitive of every non-medium entry (world-space boxes over the shutter; an instance's
// primitives through its transform, padded), so the whole world query is one candidate search in
// render_step_kernel instead of a loop over entries with a traversal per BVH.  Each leaf keeps its
// entry's semantics: it is tested in its instance's frame, its tie key orders exact ties as the list
// does (a later entry wins) and, inside a BVH entry, as bvh.h does (the lower reference leaf rank
// wins), and a BVH member's winner is validated on that BVH's reference chain (world_settle).
// Media must follow every tree entry in the list (they draw from the RNG with the closest hit so far
// as their t_max), except inert ones: a medium bounded by a sphere never reaches its draw (H1: the
// second boundary query returns nothing or t1 itself) unless its boundary root is NaN, which a
// sane ray (ray_sane) cannot produce.  Leaves: 4 float4 each (see DScene::wleaf).
// A constant medium that never reaches its RNG draw for a sane ray (ray_sane): its boundary is a
// sphere with coordinates and radius below 1e6, whose second boundary query repeats the first root
// (H1, sphere.h:51) -- see sphere_boundary_no_hit -- or a moving sphere whose centre c0 + (tm - t0) /
// dt * d stays within 1e6 of c0 for every sane ray time (|tm| < 1024): a tiny shutter span dt would
// let the centre run off to where the boundary root overflows to NaN, and NaN reaches the draw.
static bool medium_inert(const rt_scene_soa* s, const rt_object& o) {
  if (o.kind != RT_OBJ_MEDIUM || o.a < 0 || o.a >= s->n_objects) return false;
  const rt_object& bo = s->objects[o.a];
  if (bo.kind != RT_OBJ_PRIM) return false;
  const rt_prim& q = s->prims[bo.a];
  const int ty = q.type & 0xff;
  if (ty != RT_PRIM_SPHERE && ty != RT_PRIM_MOVING_SPHERE) return false;
  const int np = ty == RT_PRIM_SPHERE ? 4 : 9;
  for (int k = 0; k < np; ++k)
    if (!(std::fabs(q.p[k]) < 1e6f)) return false;
  if (ty == RT_PRIM_SPHERE) return true;
  const double dmax = std::max(std::fabs((double)q.p[4]), std::max(std::fabs((double)q.p[5]), std::fabs((double)q.p[6])));
  return q.p[8] != 0.0f && (1024.0 + std::fabs((double)q.p[7])) / std::fabs((double)q.p[8]) * dmax < 1e6;
}

static bool build_world_tree(const rt_scene_soa* s, const std::vector<rt_prim>& prims, std::vector<rt_bvh_node>& nodes,
                             std::vector<Float4>& wleaf, std::vector<Float4>& wxf, int& wt_fb, int& w_media,
                             int& w_inert) {
  const int NW = s->n_world;
  if (NW < 2 || NW >= (1 << (31 - RT_WKEY_SHIFT))) return false;
  auto obj = [&](int k) -> const rt_object& { return s->objects[k]; };
  int last_tree = -1;
  for (int w = 0; w < NW; ++w)
    if (obj(s->world[w]).kind != RT_OBJ_MEDIUM) last_tree = w;
  if (last_tree < 0) return false;
  w_inert = 0;
  for (int w = 0; w < NW; ++w) {
    const rt_object& o = obj(s->world[w]);
    if (o.kind == RT_OBJ_MEDIUM) {
      const rt_object& bo = obj(o.a);
      if (w < last_tree) {  // must be inert
        if (!medium_inert(s, o)) return false;
        w_inert = 1;
      } else if (!(bo.kind == RT_OBJ_PRIM || (bo.kind == RT_OBJ_XFORM && obj(bo.a).kind == RT_OBJ_PRIM))) {
        return false;  // active media: primitive boundaries (object_query's direct path)
      }
    } else if (o.kind == RT_OBJ_XFORM) {
      const int ck = obj(o.a).kind;
      if (ck != RT_OBJ_PRIM && ck != RT_OBJ_BVH) return false;
    } else if (o.kind != RT_OBJ_PRIM && o.kind != RT_OBJ_BVH) {
      return false;
    }
  }
  w_media = last_tree + 1;
  struct Leaf {
    int prim, xf, w, bobj, rank;
  };
  std::vector<Leaf> leaves;
  std::vector<rth::Box> box;
  std::vector<int> xf_of(s->n_objects, -1);
  const float t0 = std::fmin(s->camera.time0, s->camera.time1), t1 = std::fmax(s->camera.time0, s->camera.time1);
  for (int w = 0; w < w_media; ++w) {
    int oi = s->world[w];
    if (obj(oi).kind == RT_OBJ_MEDIUM) continue;  // inert
    int xf = -1, xo = -1;
    if (obj(oi).kind == RT_OBJ_XFORM) {
      xo = oi;
      if (xf_of[oi] < 0) {
        const rt_object& o = obj(oi);
        int32_t bits = o.b;
        float fb;
        memcpy(&fb, &bits, 4);
        xf_of[oi] = (int)wxf.size() / 2;
        wxf.push_back(Float4{o.f[0], o.f[1], o.f[2], fb});
        wxf.push_back(Float4{o.f[3], o.f[4], 0.0f, 0.0f});
      }
      xf = xf_of[oi];
      oi = obj(oi).a;
    }
    auto add = [&](int pid, int bobj, int rank) {
      rth::Box b = geom_box(s->prims[pid], s->triangles, t0, t1);
      if (xo >= 0) b = xform_box(obj(xo), b);
      leaves.push_back(Leaf{pid, xf, w, bobj, rank});
      box.push_back(b);
    };
    const rt_object& o = obj(oi);
    if (o.kind == RT_OBJ_PRIM) {
      add(o.a, -1, 0);
    } else {  // BVH: its reference leaves, with their ranks in the reference's depth-first order
      if (o.b > RT_WKEY_SHIFT) return false;
      for_each_leaf(s, o.a, o.b, [&](int id, int rank) { add(id, oi, rank); });
    }
  }
  const int n = (int)leaves.size();
  if (n < 2 || n >= (1 << 24)) return false;
  wleaf.resize(4 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    const Leaf& L = leaves[(size_t)i];
    rt_prim q = prims[(size_t)L.prim];  // the device record: flags, triangle operands
    const int32_t key = ((NW - 1 - L.w) << RT_WKEY_SHIFT) | L.rank;
    memcpy(&q.p[9], &key, 4);
    if (L.xf >= 0) q.type |= RT_PRIM_FLAG_XF;
    memcpy(&wleaf[4 * (size_t)i], &q, sizeof(q));
    const int32_t d[4] = {L.xf, L.w, L.bobj, L.prim};
    memcpy(&wleaf[4 * (size_t)i + 3], d, sizeof(d));
  }
  std::vector<int> ids(n);
  for (int i = 0; i < n; ++i) ids[(size_t)i] = i;
  wt_fb = (int)nodes.size();
  nodes.resize(wt_fb + 2);  // record 0 = root
  SahBuilder sb{box, nodes, wt_fb};
  sb.build(ids.data(), n, 0);
  return true;
}

// Quantized traversal tree (F_QLDS; qpair): the world BVH's traversal-tree pair records, `npairs` of
// them from rt_bvh_node index fb, as 24-byte records that fit LDS next to 16-bit stacks (C4's door:
// 4 329 pairs = 104 KB + 32 KB of stacks, instead of 277 KB in L2).  Per pair and axis: an origin
// rounded down to binary16 below both children, a power-of-two scale 2^E with 255 * 2^E covering the
// pair's extent, and each child's padded box as bytes rounded outward.  False when a value does
// not fit (binary16 range, scales spread over more than 32 octaves, child words beyond 16 bits).
static bool build_qtree(const std::vector<rt_bvh_node>& nodes, int fb, int npairs, std::vector<uint32_t>& out,
                        int& ebias) {
  auto half_down = [](double x, uint16_t& bits) {
    if (!(std::fabs(x) < 60000.0)) return false;
    _Float16 h = (_Float16)(float)x;
    memcpy(&bits, &h, 2);
    while ((double)(float)h > x) {  // step down one binary16 ulp
      bits = (bits & 0x8000u) ? (uint16_t)(bits + 1) : (bits == 0 ? (uint16_t)0x8001u : (uint16_t)(bits - 1));
      memcpy(&h, &bits, 2);
    }
    return true;
  };
  std::vector<int> E((size_t)npairs * 3);
  std::vector<uint16_t> org((size_t)npairs * 3);
  int emax = -1000;
  for (int i = 0; i < npairs; ++i) {
    const rt_bvh_node* r = &nodes[(size_t)fb + 2 * (size_t)i];
    for (int a = 0; a < 3; ++a) {
      const double mn = std::min(r[0].lo[a], r[1].lo[a]), mx = std::max(r[0].hi[a], r[1].hi[a]);
      uint16_t ob;
      if (!half_down(mn, ob) || !(mx >= mn) || !(mx < 60000.0)) return false;
      _Float16 h;
      memcpy(&h, &ob, 2);
      const double ext = mx - (double)(float)h;
      int e = -60;
      while (255.0 * std::ldexp(1.0, e) < ext) ++e;
      org[3 * (size_t)i + a] = ob;
      E[3 * (size_t)i + a] = e;
      emax = std::max(emax, e);
    }
  }
  ebias = emax - 31;  // a scale below 2^ebias is widened to it: coarser, still covering
  if (ebias < -120 || emax > 100) return false;
  out.assign((size_t)npairs * 6, 0u);
  for (int i = 0; i < npairs; ++i) {
    const rt_bvh_node* r = &nodes[(size_t)fb + 2 * (size_t)i];
    uint32_t ee = 0;
    uint8_t q[2][6];
    for (int a = 0; a < 3; ++a) {
      const int e = std::max(E[3 * (size_t)i + a], ebias);
      ee |= (uint32_t)(e - ebias) << (5 * a);
      _Float16 h;
      memcpy(&h, &org[3 * (size_t)i + a], 2);
      const double o = (double)(float)h, sc = std::ldexp(1.0, e);
      for (int ch = 0; ch < 2; ++ch) {
        const double lo = std::floor(((double)r[ch].lo[a] - o) / sc), hi = std::ceil(((double)r[ch].hi[a] - o) / sc);
        if (!(lo >= 0.0 && hi <= 255.0 && lo <= hi)) return false;
        if (!(o + lo * sc <= (double)r[ch].lo[a] && o + hi * sc >= (double)r[ch].hi[a])) return false;
        q[ch][a] = (uint8_t)lo;
        q[ch][3 + a] = (uint8_t)hi;
      }
    }
    const int c0 = r[0].leaf_a, c1 = r[0].leaf_b;
    if (c0 < -32768 || c0 > 32767 || c1 < -32768 || c1 > 32767) return false;
    uint32_t* w = &out[6 * (size_t)i];
    w[0] = (uint32_t)org[3 * (size_t)i] | (uint32_t)org[3 * (size_t)i + 1] << 16;
    w[1] = (uint32_t)org[3 * (size_t)i + 2] | ee << 16;
    const uint8_t b[12] = {q[0][0], q[0][1], q[0][2], q[0][3], q[0][4], q[0][5],
                           q[1][0], q[1][1], q[1][2], q[1][3], q[1][4], q[1][5]};
    memcpy(&w[2], b, 12);
    w[5] = ((uint32_t)c0 & 0xffffu) | ((uint32_t)c1 << 16);
  }
  return true;
}

}  // namespace

int prepare(const rt_scene_soa* s, const Options& opt, Prepared& P, std::string& why) {
  P = Prepared{};
  std::vector<rt_prim>& prims = P.prims;
  std::vector<rt_bvh_node>& nodes = P.nodes;
  std::vector<rt_object>& objects = P.objects;
  // Device copies: primitives with the u,v flag folded into the type word and their reference
  // leaf rank in p[9]; nodes = reference trees followed by the traversal trees built here.
  prims.assign(s->prims, s->prims + s->n_prims);
  for (rt_prim& p : prims) {
    const rt_material& m = s->materials[p.material];
    if (p.type == RT_PRIM_SPHERE && m.type != RT_MAT_DIELECTRIC && tex_needs_uv(s, m.texture)) p.type |= RT_PRIM_FLAG_UV;
    if (p.type == RT_PRIM_MOVING_SPHERE && p.p[7] == 0.0f && p.p[8] == 1.0f) p.type |= RT_PRIM_FLAG_UNIT_T;
    int32_t none = -1;
    memcpy(&p.p[9], &none, 4);
  }
  nodes.assign(s->nodes, s->nodes + s->n_nodes);
  objects.assign(s->objects, s->objects + s->n_objects);
  P.pmargin.assign(s->n_prims, Float2{-INFINITY, -INFINITY});
  // (pvalid of a primitive outside every BVH: safe = -inf, so chain_ok's first test never applies)
  P.pvalid.assign(3 * (size_t)s->n_prims, Float4{0.0f, 0.0f, 0.0f, -INFINITY});
  std::vector<int> tree_pairs(objects.size(), 0);  // records of each BVH object's traversal tree
  for (size_t k = 0; k < objects.size(); ++k) {
    rt_object& o = objects[k];
    o.c = -1;
    if (o.kind == RT_OBJ_MEDIUM && medium_inert(s, o)) o.c = 1;  // object_query skips it for sane rays
    if (o.kind == RT_OBJ_BVH) {
      const int fast = build_traversal_tree(s, o.a, o.b, prims, nodes, P.pmargin, P.pvalid, &tree_pairs[k],
                                            opt.dedup_triangles != 0);
      o.c = fast;
    }
  }
  // Triangles: the Moller-Trumbore operands (v0, e0, e1) in p[0..8] of the device record and the
  // triangle's index in the type word's bits 12..31, so a hit test is one 48-byte fetch; the
  // 144-byte record is read only for the winner's hit record.
  for (rt_prim& p : prims) {
    if ((p.type & 0xff) != RT_PRIM_TRIANGLE) continue;
    const int ti = (int)p.p[0];
    const rt_triangle& t = s->triangles[ti];
    for (int k = 0; k < 3; ++k) {
      p.p[k] = t.v0[k];
      p.p[3 + k] = t.e0[k];
      p.p[6 + k] = t.e1[k];
    }
    p.type |= ti << 12;
  }
  bool world_step = s->n_world <= 8 && s->objects[s->world[0]].kind == RT_OBJ_BVH;
  for (int w = 1; w < s->n_world; ++w) world_step = world_step && s->objects[s->world[w]].kind == RT_OBJ_PRIM;
  // The world tree is opt-in (options.world_tree): measured slower than render_kernel's entry loop on
  // both list-world configs (MI355X: C5 3840x2159 4x4 97.2 ms vs 78.4; C3 800x800 10x10 24.7 vs 19.1)
  const bool world_tree = !world_step && opt.world_tree != 0 &&
                          build_world_tree(s, prims, nodes, P.wleaf, P.wxf, P.wt_fb, P.w_media, P.w_inert);
  if (world_step && opt.quantized_tree != 0) {  // the world BVH's traversal tree, quantized (F_QLDS)
    // (the tree's own record count: coincident triangles are not leaves of it)
    const rt_object& wo = objects[(size_t)s->world[0]];
    const int np = tree_pairs[(size_t)s->world[0]];
    const size_t tables = 16 * ((size_t)s->n_materials + 2 * (size_t)s->n_textures + (size_t)s->n_images) + 16;
    if (np >= 1 && (size_t)np * 24 + 1024 * kStackDepth * 2 + tables <= (size_t)kLdsBudget &&
        build_qtree(nodes, wo.c, np, P.qnodes, P.q_ebias))
      P.q_pairs = np;
    else
      P.qnodes.clear();  // (a tree that does not fit its format fails part-way)
  }
  if (P.pmargin.size() & 1) P.pmargin.push_back(Float2{-INFINITY, -INFINITY});  // whole float4s for LDS staging
  // Image textures in 8x8-texel tiles (row-major tiles, row-major texels inside a tile): a texel's 2-D
  // neighbours share its cache lines, whichever way the texture's axes run across the image.  The
  // device image records point into the tiled copy; texel values are unchanged.
  P.images.assign(s->images, s->images + s->n_images);
  std::vector<uint8_t>& dtexels = P.texels;
  for (rt_image& im : P.images) {
    if (im.width <= 0) continue;  // no data: the cyan fallback (texture.h:146-147)
    const long long n = (long long)im.width * im.height * im.bytes_per_pixel;
    if (dtexels.size() + ((size_t)n * (im.bytes_per_pixel < 3 ? 6 : 2)) >= (size_t)1 << 31) {
      why = "textures too large";
      return RT_ERR_SCENE;
    }
    const uint8_t* src = s->texels + im.offset;
    // A texel's value is pixel[0..2] whatever bytes_per_pixel is (texture.h:160-162): with 1 or 2
    // bytes per pixel the second and third byte are the row-major neighbours' (rt_scene_validate keeps
    // them inside texels), which are not the tiled copy's neighbours, so such an image is widened to
    // 3 bytes per texel here, each texel carrying the three bytes the reference reads.
    const int sbpp = im.bytes_per_pixel, bpp = sbpp < 3 ? 3 : sbpp;
    const int tpr = (im.width + 7) >> 3, tpc = (im.height + 7) >> 3;
    const size_t base = dtexels.size();
    dtexels.resize(base + (size_t)tpr * tpc * 64 * bpp, 0);
    for (int j = 0; j < im.height; ++j)
      for (int i = 0; i < im.width; ++i)
        memcpy(&dtexels[base + (((size_t)((j >> 3) * tpr + (i >> 3)) << 6) + ((j & 7) << 3) + (i & 7)) * bpp],
               src + ((size_t)j * im.width + i) * sbpp, (size_t)bpp);
    im.bytes_per_pixel = bpp;
    im.offset = (int32_t)base;
  }
  // world_search applies: a list of primitives, BVHs (up to 2^20 leaves) and instances of them, and
  // inert media (options.merged_search: RT_MERGE_OFF keeps the entry loop; RT_MERGE_FALLBACK_ALL runs
  // the search, then every query takes the exact list -- tests)
  P.merge_ok = !world_step && s->n_world >= 2 && s->n_world < (1 << (31 - RT_WKEY_SHIFT)) &&
               opt.merged_search != RT_MERGE_OFF;
  for (int w = 0; w < s->n_world && P.merge_ok; ++w) {
    const rt_object& o = s->objects[s->world[w]];
    const rt_object& x = o.kind == RT_OBJ_XFORM ? s->objects[o.a] : o;
    if (o.kind == RT_OBJ_MEDIUM) P.merge_ok = medium_inert(s, o);
    else if (x.kind == RT_OBJ_BVH) P.merge_ok = x.b <= RT_WKEY_SHIFT;
    else P.merge_ok = x.kind == RT_OBJ_PRIM;
  }
  if (P.merge_ok && opt.merged_search == RT_MERGE_FALLBACK_ALL) P.merge_ok = 2;
  // world_search's visiting order (the winner does not depend on it: tie keys carry the list
  // position): the primitive entries first (one test each; their hits cull the traversals after
  // them), then the BVH and instance entries nearest first by the distance from the camera's origin
  // to their world-space box over the shutter, then the (inert) media.  C5, same box, Mrays/s: list
  // order 5 010-5 017, primitives first 5 036-5 044, primitives first + ground, door, instance (the
  // distance order) 5 093, + door, instance, ground 5 086, BVHs first 4 960.  options.merge_order:
  // RT_ORDER_LIST keeps list order, RT_ORDER_REVERSED reverses it (tests: both arrival orders of a tie).
  std::vector<int32_t>& worder = P.worder;
  worder.resize((size_t)s->n_world);
  for (int w = 0; w < s->n_world; ++w) worder[(size_t)w] = w;
  if (opt.merge_order == RT_ORDER_REVERSED) std::reverse(worder.begin(), worder.end());
  if (opt.merge_order == RT_ORDER_DISTANCE) {
    const float t0 = std::min(s->camera.time0, s->camera.time1), t1 = std::max(s->camera.time0, s->camera.time1);
    auto rank = [&](int w) -> double {  // < 0: primitive; distance: BVH / instance; +inf: medium / no box
      const rt_object& o = s->objects[s->world[w]];
      if (o.kind == RT_OBJ_PRIM) return -1.0;
      rth::Box b;
      if (o.kind == RT_OBJ_MEDIUM || !object_box(s, s->world[w], t0, t1, b)) return INFINITY;
      double d2 = 0.0;
      for (int a = 0; a < 3; ++a) {
        const double c = s->camera.origin[a], g = c < b.lo[a] ? b.lo[a] - c : (c > b.hi[a] ? c - b.hi[a] : 0.0);
        d2 += g * g;
      }
      return d2;
    };
    std::vector<double> key((size_t)s->n_world);
    for (int w = 0; w < s->n_world; ++w) key[(size_t)w] = rank(w);
    std::stable_sort(worder.begin(), worder.end(), [&](int x, int y) { return key[(size_t)x] < key[(size_t)y]; });
  }
  P.features = scene_features(s);
  P.world_bvh = s->n_world == 1 && s->objects[s->world[0]].kind == RT_OBJ_BVH;
  P.world_step = world_step;
  P.world_tree = world_tree;
  const Shutter sh = shutter(s);
  if (P.world_bvh) {  // bounding spheres of the world BVH's primitives (boxes over the shutter)
    const rt_object& o = s->objects[s->world[0]];
    for_each_leaf(s, o.a, o.b, [&](int id, int) {
      P.bin_sph.push_back(box_sphere(geom_box(s->prims[id], s->triangles, sh.t0, sh.t1)));
      P.bin_ids.push_back(id);
    });
    P.bin_n = (int)P.bin_ids.size();
  } else {  // list world: bounding spheres of the top-level entries (camera-ray entry masks)
    for (int w = 0; w < s->n_world && w < 32; ++w) {
      rth::Box b;
      P.bin_sph.push_back(object_box(s, s->world[w], sh.t0, sh.t1, b)
                              ? box_sphere(b) : Float4{0.0f, 0.0f, 0.0f, INFINITY});
    }
    P.bin_n = -(int)P.bin_sph.size();  // negative: entry spheres (masks), not primitive spheres (lists)
  }
  // the stepwise LDS variant stages the world BVH's traversal tree in planes (stage_lds): it must be
  // the last tree of the node array and have at most kPlanePairs records.  A larger sphere tree (more
  // than 512 primitives) runs the stepwise kernel from global memory instead (documented cap: the
  // plane offsets are immediates, and every reference sphere scene fits; C2 has 487 pairs)
  if (world_step) {
    const rt_object& wo = objects[(size_t)s->world[0]];
    const int np = tree_pairs[(size_t)s->world[0]];
    if (np >= 1 && np <= kPlanePairs && wo.c + 2 * np == (int)nodes.size()) {
      P.plane_fb = wo.c;
      P.plane_pairs = np;
    }
  }
  return RT_OK;
}

}  // namespace rtprep
