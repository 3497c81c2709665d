// rt_validate.cpp — rt_scene_validate: every index, count, type and nesting of a flattened scene
// (include/rt_hip.h, rt_scene_soa) checked on the host before anything is copied to the device, where
// a bad index would first show as an out-of-range read.  Host only: no HIP call, no context.
//
// What passes here is what the kernels render as the reference's objects would (tests/test_flat_gpu.py
// against the oracle's ref_scene_from_flat), within the promise include/rt_hip.h states at
// rt_scene_validate.  Shapes the header does not document are refused.  The only checks of the scene's
// arrays: rt_scene_upload has none of its own.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/rt_hip.h"

namespace {

struct Msg {
  char* buf;
  size_t cap;
  int fail(const char* fmt, ...) const {
    if (buf && cap) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(buf, cap, fmt, ap);
      va_end(ap);
    }
    return RT_ERR_SCENE;
  }
};

// A sphere of a BVH that camera rays can reach from more than kResolveRadii radii away, under any
// nesting (a BVH in the world, under a transform, as a medium's boundary), a moving sphere at both
// ends of the shutter: index of the primitive, or -1.  sphere.h's float discriminant hb^2 - a cc
// carries a rounding error of the order of 2^-23 a L^2 (L = distance from the ray origin to the centre),
// so the reference's hit() answers "hit" for rays passing within about sqrt(r^2 + 2^-23 L^2) of the
// centre: at L = 512 r that is 1.016 r, beyond any box that bounds the sphere, and the reference
// returns such a hit wherever its stored boxes let the test run.  No search that culls by the sphere's
// own extent reproduces that, so such a scene is outside what the header promises.  (A sphere that is a
// PRIM or LIST entry is always tested by the same float operations and needs no rule.)
constexpr double kResolveRadii = 512.0;

struct Frame {  // translate(rotate_y(.)) of the enclosing transform: world = Ry(p) + off
  double sn = 0.0, cs = 1.0, off[3] = {0.0, 0.0, 0.0};
};

int far_sphere_of_bvh(const rt_scene_soa* s, const rt_object& bvh, const Frame& fr, const double f[3], double fl,
                      double half) {
  const rt_camera& C = s->camera;
  const int inner = (1 << bvh.b) - 1, last0 = (1 << (bvh.b - 1)) - 1;
  for (int k = last0; k < inner; ++k)
    for (int id : {s->nodes[bvh.a + k].leaf_a, s->nodes[bvh.a + k].leaf_b}) {
      if (id < 0 || s->prims[id].type > RT_PRIM_MOVING_SPHERE) continue;
      const float* p = s->prims[id].p;
      const double r = std::fabs((double)p[3]);
      const bool moving = s->prims[id].type == RT_PRIM_MOVING_SPHERE;
      for (int e = 0; e < (moving ? 2 : 1); ++e) {
        double c[3] = {p[0], p[1], p[2]};
        if (moving) {
          const double sc = ((double)(e ? C.time1 : C.time0) - p[7]) / p[8];
          for (int q = 0; q < 3; ++q) c[q] += sc * p[4 + q];
        }
        const double w[3] = {fr.cs * c[0] + fr.sn * c[2] + fr.off[0], c[1] + fr.off[1],
                             -fr.sn * c[0] + fr.cs * c[2] + fr.off[2]};
        double L2 = 0.0, along = 0.0;
        for (int q = 0; q < 3; ++q) {
          const double oc = w[q] - C.origin[q];
          L2 += oc * oc;
          along += oc * f[q] / fl;
        }
        if (!(L2 > kResolveRadii * kResolveRadii * r * r)) continue;  // (a NaN centre is not this rule's business)
        const double L = std::sqrt(L2);
        const double angle = std::acos(std::fmax(-1.0, std::fmin(1.0, along / L)));
        // inside the view cone (its half diagonal), widened by the sphere, the lens and the error zone
        if (angle <= half + (r + std::fabs((double)C.lens_radius)) / L + 0x1p-10) return id;
      }
    }
  return -1;
}

int far_sphere(const rt_scene_soa* s) {
  const rt_camera& C = s->camera;
  double f[3], fl = 0.0, hl = 0.0, vl = 0.0;
  for (int k = 0; k < 3; ++k) {
    f[k] = (double)C.lower_left[k] + 0.5 * C.horizontal[k] + 0.5 * C.vertical[k] - C.origin[k];
    fl += f[k] * f[k];
    hl += (double)C.horizontal[k] * C.horizontal[k];
    vl += (double)C.vertical[k] * C.vertical[k];
  }
  fl = std::sqrt(fl);
  if (!(fl > 0.0)) return -1;
  const double half = std::atan(0.5 * std::sqrt(hl + vl) / fl);
  for (int w = 0; w < s->n_world; ++w) {
    const rt_object* o = &s->objects[s->world[w]];
    if (o->kind == RT_OBJ_MEDIUM) o = &s->objects[o->a];
    Frame fr;
    if (o->kind == RT_OBJ_XFORM) {
      if (o->b & 2) {
        fr.sn = o->f[3];
        fr.cs = o->f[4];
      }
      if (o->b & 1)
        for (int q = 0; q < 3; ++q) fr.off[q] = o->f[q];
      o = &s->objects[o->a];
    }
    if (o->kind != RT_OBJ_BVH) continue;
    const int id = far_sphere_of_bvh(s, *o, fr, f, fl, half);
    if (id >= 0) return id;
  }
  return -1;
}

}  // namespace

extern "C" int rt_scene_validate(const rt_scene_soa* s, char* msg, size_t cap) {
  const Msg m{msg, cap};
  if (msg && cap) msg[0] = 0;
  if (!s) return RT_ERR_ARG;
  if (s->n_world <= 0 || !s->world || s->n_objects <= 0 || !s->objects || s->n_materials <= 0 || !s->materials)
    return m.fail("empty scene");
  if (s->n_prims < 0 || s->n_triangles < 0 || s->n_nodes < 0 || s->n_textures < 0 || s->n_perlins < 0 ||
      s->n_images < 0 || s->n_texels < 0)
    return m.fail("negative count");
  if ((s->n_prims && !s->prims) || (s->n_triangles && !s->triangles) || (s->n_nodes && !s->nodes) ||
      (s->n_textures && !s->textures) || (s->n_perlins && !s->perlins) || (s->n_images && !s->images) ||
      (s->n_texels && !s->texels))
    return m.fail("null array with a nonzero count");

  // images, perlin tables, textures, materials
  for (int k = 0; k < s->n_images; ++k) {
    const rt_image& im = s->images[k];
    if (im.width <= 0) continue;  // no data: the cyan fallback (texture.h:146-147)
    const long long n = (long long)im.width * im.height * im.bytes_per_pixel;
    // a texel is read as pixel[0..2] whatever bytes_per_pixel is (texture.h:160-162)
    const long long reach = n + (im.bytes_per_pixel < 3 ? 3 - im.bytes_per_pixel : 0);
    if (im.height <= 0 || im.bytes_per_pixel < 1 || im.bytes_per_pixel > 4 || im.offset < 0 || n >= (1LL << 31) ||
        im.offset + reach > s->n_texels)
      return m.fail("image %d: texels out of range", k);
  }
  for (int k = 0; k < s->n_perlins; ++k) {
    const rt_perlin& p = s->perlins[k];
    for (int i = 0; i < 256; ++i)
      if ((p.perm_x[i] | p.perm_y[i] | p.perm_z[i]) & ~255) return m.fail("perlin %d: permutation entry out of range", k);
  }
  for (int k = 0; k < s->n_textures; ++k) {
    const rt_texture& t = s->textures[k];
    switch (t.type) {
      case RT_TEX_SOLID: break;
      case RT_TEX_CHECKER:
        if (t.a < 0 || t.a >= s->n_textures || t.b < 0 || t.b >= s->n_textures)
          return m.fail("texture %d: checker texture out of range", k);
        if (s->textures[t.a].type == RT_TEX_CHECKER || s->textures[t.b].type == RT_TEX_CHECKER)
          return m.fail("texture %d: a checker of a checker", k);
        break;
      case RT_TEX_NOISE:
      case RT_TEX_TURBULENT:
      case RT_TEX_MARBLE:
        if (t.a < 0 || t.a >= s->n_perlins) return m.fail("texture %d: perlin table out of range", k);
        if (t.type == RT_TEX_TURBULENT && (t.b < 0 || t.b > 64)) return m.fail("texture %d: turbulence depth", k);
        break;
      case RT_TEX_IMAGE:
        if (t.a < 0 || t.a >= s->n_images) return m.fail("texture %d: image out of range", k);
        break;
      default: return m.fail("texture %d: unknown type %d", k, t.type);
    }
  }
  for (int k = 0; k < s->n_materials; ++k) {
    const rt_material& mt = s->materials[k];
    if (mt.type < RT_MAT_LAMBERTIAN || mt.type > RT_MAT_ISOTROPIC) return m.fail("material %d: unknown type %d", k, mt.type);
    if (mt.type != RT_MAT_DIELECTRIC && (mt.texture < 0 || mt.texture >= s->n_textures))
      return m.fail("material %d: texture out of range", k);
  }

  // primitives
  for (int k = 0; k < s->n_prims; ++k) {
    const rt_prim& p = s->prims[k];
    if (p.type < RT_PRIM_SPHERE || p.type > RT_PRIM_BOX) return m.fail("prim %d: unknown type %d", k, p.type);
    if (p.material < 0 || p.material >= s->n_materials) return m.fail("prim %d: prim material out of range", k);
    if (p.type == RT_PRIM_TRIANGLE) {
      const float ti = p.p[0];
      if (!(ti >= 0.0f && ti < (float)s->n_triangles && ti < (float)(1 << 19)) || ti != (float)(int)ti)
        return m.fail("prim %d: triangle index out of range", k);
    }
  }

  // objects: ranges, then the documented nesting (XFORM over PRIM/LIST/BVH, MEDIUM over those and
  // XFORM), which also rules out cycles
  std::vector<char> in_bvh((size_t)s->n_prims, 0);
  for (int k = 0; k < s->n_objects; ++k) {
    const rt_object& o = s->objects[k];
    switch (o.kind) {
      case RT_OBJ_PRIM:
        if (o.a < 0 || o.a >= s->n_prims) return m.fail("object %d: prim index out of range", k);
        break;
      case RT_OBJ_LIST:
        if (o.a < 0 || o.b < 1 || (long long)o.a + o.b > s->n_prims) return m.fail("object %d: prim index out of range", k);
        break;
      case RT_OBJ_BVH: {
        if (o.b < 2 || o.b > 30 || o.a < 0 || (long long)o.a + (1LL << o.b) - 1 > s->n_nodes)
          return m.fail("object %d: bvh out of range", k);
        const int inner = (1 << o.b) - 1, last0 = (1 << (o.b - 1)) - 1;
        for (int q = last0; q < inner; ++q) {
          const rt_bvh_node& nd = s->nodes[o.a + q];
          if (nd.leaf_a < 0 || nd.leaf_a >= s->n_prims || nd.leaf_b < -1 || nd.leaf_b >= s->n_prims)
            return m.fail("object %d: bvh leaf out of range (node %d)", k, q);
          for (int id : {nd.leaf_a, nd.leaf_b})
            if (id >= 0 && in_bvh[(size_t)id]++) return m.fail("object %d: prim %d is a bvh leaf twice", k, id);
        }
        break;
      }
      case RT_OBJ_XFORM:
        if (o.a < 0 || o.a >= s->n_objects) return m.fail("object %d: child object out of range", k);
        if (o.b < 0 || o.b > 3) return m.fail("object %d: transform flags", k);
        if (s->objects[o.a].kind != RT_OBJ_PRIM && s->objects[o.a].kind != RT_OBJ_LIST && s->objects[o.a].kind != RT_OBJ_BVH)
          return m.fail("object %d: transform child kind %d", k, s->objects[o.a].kind);
        break;
      case RT_OBJ_MEDIUM:
        if (o.a < 0 || o.a >= s->n_objects) return m.fail("object %d: child object out of range", k);
        if (o.b < 0 || o.b >= s->n_materials) return m.fail("object %d: phase material out of range", k);
        if (s->objects[o.a].kind < RT_OBJ_PRIM || s->objects[o.a].kind > RT_OBJ_XFORM)
          return m.fail("object %d: medium boundary kind %d", k, s->objects[o.a].kind);
        break;
      default: return m.fail("object %d: unknown kind %d", k, o.kind);
    }
  }
  // a BVH's leaves are its own: the traversal keeps per-primitive leaf ranks and ancestor boxes
  for (int k = 0; k < s->n_objects; ++k) {
    const rt_object& o = s->objects[k];
    if (o.kind != RT_OBJ_PRIM && o.kind != RT_OBJ_LIST) continue;
    for (int q = 0; q < (o.kind == RT_OBJ_LIST ? o.b : 1); ++q)
      if (in_bvh[(size_t)(o.a + q)]) return m.fail("object %d: prim %d is also a bvh leaf", k, o.a + q);
  }
  for (int k = 0; k < s->n_world; ++k)
    if (s->world[k] < 0 || s->world[k] >= s->n_objects) return m.fail("world index out of range (entry %d)", k);
  const int far = far_sphere(s);
  if (far >= 0) return m.fail("prim %d: a bvh sphere in view more than 512 radii from the camera", far);
  return RT_OK;
}
