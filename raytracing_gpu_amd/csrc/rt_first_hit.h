// rt_first_hit.h -- internal: the first hit of one ray in a flattened scene (include/rt_hip.h, "ray casts and
// feature buffers"), stated once for the device kernels of rt_guide.hip and the host twin of rt_guide_host.cpp.
// It answers world->hit(r, 0.001f, inf) with the reference's semantics and float operations, one rounded IEEE
// operation per operator in the reference's order (-ffp-contract=off on both sides), and the material's texture
// value at the hit.  No HIP header: RT_HD functions over an rt_scene_soa whose pointers the caller made
// addressable (host arrays, or the guide's device copy).  The scene has passed rt_scene_validate and
// rtfh::scene_fits.
//
// What it covers: the top-level list in order (hittable_list.h:23-39: t_max = closest so far, a later entry
// wins a tie); RT_OBJ_PRIM, RT_OBJ_LIST, RT_OBJ_BVH, RT_OBJ_XFORM (translate(rotate_y(child)) with both
// set_face_normal quirks of hittable.h); the seven primitive types, a moving sphere at the ray's time, a box as
// its list of six rects; triangle normals flat (unnormalised) and per-vertex; the exact BVH visit of bvh.h:348-436,
// RT_FLAG_EXACT_TRAVERSAL's: depth first, left then right, every box tested against the caller's interval, no
// culling by the closest hit, a leaf replaces the record only with a strictly smaller t.
//
// Media.  constant_medium::hit draws a random number, and a feature must not.  For an RT_OBJ_MEDIUM the cast
// reports the nearest hit of the boundary object in (0.001, closest so far]: t, p, u, v, prim, front and the
// normal are the boundary's; `material` is the phase material and the albedo is that material's texture.
//
// Traversal needs no stack: a BVH is a perfect tree in heap order, so the node after a subtree is found from the
// node's index alone (next_node).  The bound that stands in for a stack depth is kMaxRows, the deepest tree
// whose 1-based node indices fit 31 bits -- rt_scene_validate's own limit; nesting is at most
// MEDIUM > XFORM > BVH > BOX and is walked by straight-line code.  scene_fits refuses anything deeper.
#ifndef RT_FIRST_HIT_H
#define RT_FIRST_HIT_H

#include <stdint.h>

#include "../../include/rt_hip.h"
#include "rt_detmath.h"

namespace rtfh {

constexpr int kMaxRows = 30;  // inner levels of a BVH
constexpr float kTMin = 0.001f;

struct V3 {
  float x, y, z;
};
RT_HD V3 v3(float x, float y, float z) {
  V3 r;
  r.x = x, r.y = y, r.z = z;
  return r;
}
RT_HD V3 v3(const float* p) { return v3(p[0], p[1], p[2]); }
RT_HD V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
RT_HD V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
RT_HD V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
RT_HD V3 operator*(float t, V3 v) { return v3(t * v.x, t * v.y, t * v.z); }
RT_HD V3 operator/(V3 v, float t) { return (1.0f / t) * v; }  // vec3.h: multiplies by the reciprocal
RT_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RT_HD V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
RT_HD float axis(V3 v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }
RT_HD float inf() { return __builtin_inff(); }

struct Ray {
  V3 o, d;
  float tm;
};
RT_HD V3 at(const Ray& r, float t) { return r.o + t * r.d; }

// hit_record (hittable.h:8-23); `out` is a sphere's outward normal in its own frame, from which its u, v are
// taken once the nearest hit is known (sphere.h:25-26 costs two transcendentals).
struct Rec {
  float t;
  V3 p, n, out;
  float u, v;
  int32_t prim, material, front;
};
RT_HD void face(Rec& rec, const Ray& r, V3 outward) {  // set_face_normal
  rec.front = dot(r.d, outward) < 0.0f;
  rec.n = rec.front ? outward : -outward;
}

// ---------------------------------------------------------------- primitives
RT_HD bool sphere_hit(V3 c, float rad, const Ray& r, float tmin, float tmax, Rec& rec) {  // sphere.h:35-78
  const V3 oc = r.o - c;
  const float a = dot(r.d, r.d);
  const float hb = dot(oc, r.d);
  const float cc = dot(oc, oc) - rad * rad;
  const float disc = hb * hb - a * cc;
  if (disc < 0.0f) return false;
  const float sq = __builtin_sqrtf(disc);
  const float root = (-hb - sq) / a;  // the reference's second-root retest repeats this value
  if (root < tmin || tmax < root) return false;
  rec.t = root;
  rec.p = at(r, root);
  rec.out = (rec.p - c) / rad;
  face(rec, r, rec.out);
  rec.u = 0.0f;  // a moving sphere's stay 0; a sphere's follow in cast()
  rec.v = 0.0f;
  return true;
}

// aarect.h:8-150; ax = the normal's axis: 2 xy, 1 xz, 0 yz.  p = a0 a1 b0 b1 k (a1-a0) (b1-b0).
RT_HD bool rect_hit(int ax, float a0, float a1, float b0, float b1, float k, float wa, float wb, const Ray& r, float tmin,
                    float tmax, Rec& rec) {
  const int ia = ax == 0 ? 1 : 0, ib = ax == 2 ? 1 : 2;
  const float t = (k - axis(r.o, ax)) / axis(r.d, ax);
  if (t < tmin || t > tmax) return false;
  const float a = axis(r.o, ia) + t * axis(r.d, ia);
  const float b = axis(r.o, ib) + t * axis(r.d, ib);
  if (a < a0 || a > a1 || b < b0 || b > b1) return false;
  rec.u = (a - a0) / wa;
  rec.v = (b - b0) / wb;
  rec.t = t;
  rec.out = v3(0.0f, 0.0f, 0.0f);
  face(rec, r, v3(ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f));
  rec.p = at(r, t);
  return true;
}

RT_HD bool triangle_hit(const rt_triangle& T, const Ray& r, float tmin, float tmax, Rec& rec) {  // triangle.h:120-178
  const float eps = 0.0000001f;
  const V3 p0 = v3(T.v0), e0 = v3(T.e0), e1 = v3(T.e1);
  const V3 hh = cross(r.d, e1);
  const float a = dot(e0, hh);
  if (a > -eps && a < eps) return false;
  const float f = 1.0f / a;
  const V3 sv = r.o - p0;
  const float u = f * dot(sv, hh);
  if (u < 0.0f || u > 1.0f) return false;
  const V3 q = cross(sv, e0);
  const float v = f * dot(r.d, q);
  if ((v < 0.0f) | (u + v > 1.0f)) return false;
  const float t = f * dot(e1, q);
  if (t < tmin || t > tmax || t < eps) return false;
  rec.t = t;
  rec.out = v3(0.0f, 0.0f, 0.0f);
  rec.p = at(r, t);
  const V3 v2 = rec.p - p0;
  const float d20 = dot(v2, e0), d21 = dot(v2, e1);
  const float b0 = (T.d11 * d20 - T.d01 * d21) * T.inv_denom;
  const float b1 = (T.d00 * d21 - T.d01 * d20) * T.inv_denom;
  const float b2 = 1.0f - b0 - b1;
  rec.u = b2 * T.uv[0] + b0 * T.uv[2] + b1 * T.uv[4];
  rec.v = b2 * T.uv[1] + b0 * T.uv[3] + b1 * T.uv[5];
  if (!T.vertex_normals) {
    face(rec, r, cross(e1, e0));  // the unnormalised face normal
  } else {
    face(rec, r, v3(b2 * T.n0[0] + b0 * T.n1[0] + b1 * T.n2[0], b2 * T.n0[1] + b0 * T.n1[1] + b1 * T.n2[1],
                    b2 * T.n0[2] + b0 * T.n1[2] + b1 * T.n2[2]));
  }
  return true;
}

// One primitive record against (tmin, tmax); rec is written only on a hit.
RT_HD bool prim_hit(const rt_scene_soa& sc, int32_t id, const Ray& r, float tmin, float tmax, Rec& rec) {
  const rt_prim& q = sc.prims[id];
  const float* p = q.p;
  bool hit = false;
  switch (q.type) {
    case RT_PRIM_SPHERE: hit = sphere_hit(v3(p), p[3], r, tmin, tmax, rec); break;
    case RT_PRIM_MOVING_SPHERE: {  // moving_sphere.h:20-66: centre(time) = c0 + ((time - t0) / dt) d
      const V3 c = v3(p) + ((r.tm - p[7]) / p[8]) * v3(p + 4);
      hit = sphere_hit(c, p[3], r, tmin, tmax, rec);
      break;
    }
    case RT_PRIM_RECT_XY: hit = rect_hit(2, p[0], p[1], p[2], p[3], p[4], p[5], p[6], r, tmin, tmax, rec); break;
    case RT_PRIM_RECT_XZ: hit = rect_hit(1, p[0], p[1], p[2], p[3], p[4], p[5], p[6], r, tmin, tmax, rec); break;
    case RT_PRIM_RECT_YZ: hit = rect_hit(0, p[0], p[1], p[2], p[3], p[4], p[5], p[6], r, tmin, tmax, rec); break;
    case RT_PRIM_TRIANGLE: hit = triangle_hit(sc.triangles[(int32_t)p[0]], r, tmin, tmax, rec); break;
    default: {  // RT_PRIM_BOX, box.h:8-40: the list of its six rects, z1 z0 y1 y0 x1 x0
      float best = tmax;
      for (int s = 0; s < 6; ++s) {
        const int ax = 2 - (s >> 1);
        const float k = p[ax + ((s & 1) ? 0 : 3)];
        const int ia = ax == 0 ? 1 : 0, ib = ax == 2 ? 1 : 2;
        Rec tmp;
        if (rect_hit(ax, p[ia], p[ia + 3], p[ib], p[ib + 3], k, p[ia + 3] - p[ia], p[ib + 3] - p[ib], r, tmin, best, tmp)) {
          hit = true;
          best = tmp.t;
          rec = tmp;
        }
      }
      break;
    }
  }
  if (hit) {
    rec.prim = id;
    rec.material = q.material;
  }
  return hit;
}

// ---------------------------------------------------------------- BVH (bvh.h:348-436, aabb.h:19-104)
RT_HD bool box_hit(const rt_bvh_node& nd, const Ray& r, float tmin, float tmax) {
  for (int a = 0; a < 3; ++a) {
    const float inv = 1.0f / axis(r.d, a);
    float t0 = (nd.lo[a] - axis(r.o, a)) * inv;
    float t1 = (nd.hi[a] - axis(r.o, a)) * inv;
    if (inv < 0.0f) {
      const float s = t0;
      t0 = t1;
      t1 = s;
    }
    tmin = t0 > tmin ? t0 : tmin;
    tmax = t1 < tmax ? t1 : tmax;
    if (tmax <= tmin) return false;
  }
  return true;
}
// The node visited after the whole subtree of 1-based node m in a depth-first, left-first walk: the right
// sibling of the nearest ancestor-or-self that is a left child; 1 (the root) when the walk is over.
RT_HD uint32_t next_node(uint32_t m) {
  const uint32_t n = m + 1;
  return n >> __builtin_ctz(n);
}
RT_HD bool bvh_hit(const rt_scene_soa& sc, int32_t first, int32_t rows, const Ray& r, float tmin, float tmax, Rec& rec) {
  const rt_bvh_node* nodes = sc.nodes + first;
  const uint32_t last0 = 1u << (rows - 1);  // 1-based index of the first node of the last inner row
  float best = inf();
  bool any = false;
  uint32_t m = 1;
  do {
    const rt_bvh_node& nd = nodes[m - 1];
    if (!box_hit(nd, r, tmin, tmax)) {
      m = next_node(m);
    } else if (m >= last0) {
      Rec tmp;
      if (prim_hit(sc, nd.leaf_a, r, tmin, tmax, tmp) && tmp.t < best) best = tmp.t, rec = tmp, any = true;
      if (nd.leaf_b >= 0 && prim_hit(sc, nd.leaf_b, r, tmin, tmax, tmp) && tmp.t < best) best = tmp.t, rec = tmp, any = true;
      m = next_node(m);
    } else {
      m = 2 * m;
    }
  } while (m != 1);
  return any;
}

// ---------------------------------------------------------------- objects
// PRIM, LIST or BVH.
RT_HD bool leaf_object_hit(const rt_scene_soa& sc, const rt_object& o, const Ray& r, float tmin, float tmax, Rec& rec) {
  if (o.kind == RT_OBJ_BVH) return bvh_hit(sc, o.a, o.b, r, tmin, tmax, rec);
  const int32_t n = o.kind == RT_OBJ_LIST ? o.b : 1;
  bool any = false;
  float best = tmax;
  for (int32_t k = 0; k < n; ++k) {
    Rec tmp;
    if (prim_hit(sc, o.a + k, r, tmin, best, tmp)) any = true, best = tmp.t, rec = tmp;
  }
  return any;
}
// Any top-level entry: a medium stands for its boundary (see the file comment), a transform is
// translate(rotate_y(child)), hittable.h:31-143.
RT_HD bool object_hit(const rt_scene_soa& sc, int32_t oi, const Ray& r, float tmin, float tmax, Rec& rec) {
  const rt_object* o = &sc.objects[oi];
  int32_t phase = -1;
  if (o->kind == RT_OBJ_MEDIUM) {
    phase = o->b;
    o = &sc.objects[o->a];
  }
  Ray rr = r;
  bool tr = false, rot = false;
  V3 off = v3(0.0f, 0.0f, 0.0f);
  float sn = 0.0f, cs = 1.0f;
  if (o->kind == RT_OBJ_XFORM) {
    tr = (o->b & 1) != 0;
    rot = (o->b & 2) != 0;
    off = v3(o->f);
    sn = o->f[3];
    cs = o->f[4];
    o = &sc.objects[o->a];
    if (tr) rr.o = r.o - off;
    if (rot) {
      const V3 mo = rr.o, md = rr.d;
      rr.o.x = cs * mo.x - sn * mo.z;
      rr.o.z = sn * mo.x + cs * mo.z;
      rr.d.x = cs * md.x - sn * md.z;
      rr.d.z = sn * md.x + cs * md.z;
    }
  }
  if (!leaf_object_hit(sc, *o, rr, tmin, tmax, rec)) return false;
  if (rot) {
    const V3 p = rec.p, n = rec.n;
    rec.p.x = cs * p.x + sn * p.z;
    rec.p.z = -sn * p.x + cs * p.z;
    face(rec, rr, v3(cs * n.x + sn * n.z, n.y, -sn * n.x + cs * n.z));  // the rotated-frame ray, as the reference
  }
  if (tr) {
    rec.p = rec.p + off;
    Ray mr = r;
    mr.o = r.o - off;
    face(rec, mr, rec.n);  // translate::hit faces the already faced normal again
  }
  if (phase >= 0) rec.material = phase;
  return true;
}

RT_HD bool world_hit(const rt_scene_soa& sc, const Ray& r, Rec& rec) {
  bool any = false;
  float best = inf();
  for (int32_t w = 0; w < sc.n_world; ++w) {
    Rec tmp;
    if (object_hit(sc, sc.world[w], r, kTMin, best, tmp)) any = true, best = tmp.t, rec = tmp;
  }
  return any;
}

// ---------------------------------------------------------------- textures (texture.h, perlin.h)
RT_HD float perlin_noise(const rt_perlin& pn, V3 p) {  // perlin.h:36-100
  const float fx = __builtin_floorf(p.x), fy = __builtin_floorf(p.y), fz = __builtin_floorf(p.z);
  const float u = p.x - fx, v = p.y - fy, w = p.z - fz;
  const int i = (int)fx, j = (int)fy, k = (int)fz;
  const float uu = u * u * (3.0f - 2.0f * u);
  const float vv = v * v * (3.0f - 2.0f * v);
  const float ww = w * w * (3.0f - 2.0f * w);
  float acc = 0.0f;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < 2; ++c) {
        const float* g = pn.ranvec[pn.perm_x[(i + a) & 255] ^ pn.perm_y[(j + b) & 255] ^ pn.perm_z[(k + c) & 255]];
        const V3 wv = v3(u - (float)a, v - (float)b, w - (float)c);
        acc += ((float)a * uu + (float)(1 - a) * (1.0f - uu)) * ((float)b * vv + (float)(1 - b) * (1.0f - vv)) *
               ((float)c * ww + (float)(1 - c) * (1.0f - ww)) * dot(v3(g), wv);
      }
  return acc;
}
RT_HD float perlin_turb(const rt_perlin& pn, V3 p, int depth) {
  double acc = 0.0, w = 1.0;
  for (int i = 0; i < depth; ++i) {
    acc += w * (double)perlin_noise(pn, p);
    w *= 0.5;
    p = 2.0f * p;
  }
  return (float)__builtin_fabs(acc);
}
RT_HD V3 texture_value(const rt_scene_soa& sc, int32_t ti, float u, float v, V3 p) {
  const rt_texture* t = &sc.textures[ti];
  if (t->type == RT_TEX_CHECKER) {  // texture.h:26-46; its two textures are not checkers (rt_scene_validate)
    const float s = rtm::det_sinf(10.0f * p.x) * rtm::det_sinf(10.0f * p.y) * rtm::det_sinf(10.0f * p.z);
    t = &sc.textures[s < 0.0f ? t->b : t->a];
  }
  switch (t->type) {
    case RT_TEX_NOISE: {
      const float g = 0.5f * (float)(1.0 + (double)perlin_noise(sc.perlins[t->a], t->scale * p));
      return v3(g, g, g);
    }
    case RT_TEX_TURBULENT: {
      const float g = perlin_turb(sc.perlins[t->a], t->scale * p, t->b);
      return v3(g, g, g);
    }
    case RT_TEX_MARBLE: {
      const float g = 0.5f * (1.0f + rtm::det_sinf(t->scale * p.z + 10.0f * perlin_turb(sc.perlins[t->a], t->scale * p, 7)));
      return v3(g, g, g);
    }
    case RT_TEX_IMAGE: {  // texture.h:125-163
      const rt_image& im = sc.images[t->a];
      if (im.width <= 0) return v3(0.0f, 1.0f, 1.0f);
      // clamp_d; a NaN (a sphere of radius 0) is taken to 0 so that the casts below are defined
      const float uc = !(u >= 0.0f) ? 0.0f : (u > 1.0f ? 1.0f : u);
      const float vc = !(v >= 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v);
      const double vd = 1.0 - vc;
      int i = (int)(uc * im.width);
      int j = (int)(vd * im.height);
      if (i >= im.width) i = im.width - 1;
      if (j >= im.height) j = im.height - 1;
      const float cs = 1.0f / 255.0f;
      const uint8_t* px = sc.texels + im.offset + (size_t)j * (size_t)(im.bytes_per_pixel * im.width) + (size_t)i * im.bytes_per_pixel;
      return v3(cs * px[0], cs * px[1], cs * px[2]);
    }
    default: return v3(t->color);  // RT_TEX_SOLID
  }
}

// ---------------------------------------------------------------- the cast
// One ray (8 floats: o, d, time, unused) into an rt_guide_hit.
RT_HD void cast(const rt_scene_soa& sc, const float* e, rt_guide_hit* h) {
  Ray r;
  r.o = v3(e), r.d = v3(e + 3), r.tm = e[6];
  Rec rec;
  rt_guide_hit g;
  if (!world_hit(sc, r, rec)) {
    g.t = 0.0f;
    for (int c = 0; c < 3; ++c) g.p[c] = 0.0f, g.n[c] = 0.0f, g.albedo[c] = sc.background[c];
    g.u = g.v = 0.0f;
    g.prim = -1, g.material = -1, g.front = 0, g.pad = 0;
    *h = g;
    return;
  }
  if (sc.prims[rec.prim].type == RT_PRIM_SPHERE) {  // sphere.h:25-26
    rec.u = (rtm::det_atan2f(-rec.out.z, rec.out.x) + 3.1415927f) / (2.0f * 3.1415927f);
    rec.v = rtm::det_acosf(-rec.out.y) / 3.1415927f;
  }
  const rt_material& m = sc.materials[rec.material];
  const V3 a = m.type == RT_MAT_DIELECTRIC ? v3(1.0f, 1.0f, 1.0f) : texture_value(sc, m.texture, rec.u, rec.v, rec.p);
  g.t = rec.t;
  g.p[0] = rec.p.x, g.p[1] = rec.p.y, g.p[2] = rec.p.z;
  g.n[0] = rec.n.x, g.n[1] = rec.n.y, g.n[2] = rec.n.z;
  g.albedo[0] = a.x, g.albedo[1] = a.y, g.albedo[2] = a.z;
  g.u = rec.u, g.v = rec.v;
  g.prim = rec.prim, g.material = rec.material, g.front = rec.front, g.pad = 0;
  *h = g;
}

// The centre ray of pixel (i, j) of a W x H image, row 0 at the bottom: camera.h get_ray with a lens offset
// of 0 at s = (i + 0.5) / W, t = (j + 0.5) / H, at the middle of the shutter.
RT_HD void centre_ray(const rt_camera& c, int i, int j, int W, int H, float* e) {
  const float s = ((float)i + 0.5f) / (float)W, t = ((float)j + 0.5f) / (float)H;
  const V3 d = v3(c.lower_left) + s * v3(c.horizontal) + t * v3(c.vertical) - v3(c.origin);
  e[0] = c.origin[0], e[1] = c.origin[1], e[2] = c.origin[2];
  e[3] = d.x, e[4] = d.y, e[5] = d.z;
  e[6] = c.time0 + 0.5f * (c.time1 - c.time0);
  e[7] = 0.0f;
}

// What the traversal above is bounded by, beyond rt_scene_validate: every BVH at most kMaxRows inner levels.
inline bool scene_fits(const rt_scene_soa* s) {
  for (int32_t k = 0; k < s->n_objects; ++k)
    if (s->objects[k].kind == RT_OBJ_BVH && (s->objects[k].b < 1 || s->objects[k].b > kMaxRows)) return false;
  return true;
}

}  // namespace rtfh

#endif  // RT_FIRST_HIT_H
