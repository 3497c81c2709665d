// ref_headers.cpp -- TEST INFRASTRUCTURE: the reference's own class headers, compiled for the host.
//
// `make -C oracle ref` builds this into oracle/_ref/libref_headers.so with the reference's headers
// included by name (-I$(REF_ROOT)); nothing of them is copied here and the library is never committed.
// tests/test_refhdr_cpu.py holds the oracle (oracle/ref_cpu.cpp, a restatement by reading) to it bit for
// bit, and tests/golden/make_refhdr_golden.py records its results for the GPU tests.
//
// Compiled from the reference: hit, scatter, emitted, value, get_ray, bounding_box, the BVH's layout,
// build and traversal, perlin's tables and noise -- common.h, vec3.h, ray.h, aabb.h, hittable.h,
// hittable_list.h, sphere.h, moving_sphere.h, aarect.h, box.h, triangle.h, constant_medium.h, bvh.h,
// material.h, texture.h, perlin.h, camera.h.  Not compiled: render.h (its <<<>>> launches), scenes.h and
// triangle_mesh.h (nvcc, assimp, png++).  The sample loop and the path loop of render.h:55-113 are
// therefore written here against the reference's classes, in this file's own words.
//
// Definitions this file and its shim (curand_kernel.h, which lists its own) fix:
//   * -ffp-contract=off -fno-fast-math: every operation of the reference's expressions rounds once.
//   * clang evaluates the arguments of a call left to right; the reference passes several draws as the
//     arguments of one call (vec3.h:62-69, hazard H9) and the oracle pins the same order.
//   * the camera race (H2): RT_CAM_REF_SLOT0 hands get_ray a private copy of the pristine slot-0 state
//     per pixel and frame buffer, RT_CAM_PER_PIXEL the pixel's own state.
//   * stale u, v (H13): moving_sphere::hit and constant_medium::hit leave rec.u and rec.v as the caller's
//     record had them; the subclasses below set them to 0 after a hit, as the oracle and the kernels do.
//   * operator new[] zero-fills and pads both ends: bvh.h:35 allocates one element too few for the
//     writes of :59 (H26), bvh.h:353 allocates ceil(log2 n) counters and :411 writes the leaf row's, one
//     past the end (H27), and :357 zeroes only the first two.  Neither overrun changes a result.
//   * what a flat record stores and a reference class computes itself (rect extents, moving-sphere
//     differences, a triangle's derived fields) is never overwritten: the constructor's value stands and a
//     record with other bits is refused (status 6).  What no constructor input survives for is set as
//     stored (camera vectors, sin / cos, -1/density, perlin tables, BVH leaves and boxes, metal's fuzz;
//     -fno-access-control for the private ones); refhdr_camera_build and refhdr_instance_consts run those
//     constructors on real inputs.
//   * objects are built and never destroyed (so do not render large scenes in a loop with this library):
//     the reference's destructors free what they do not own (hittable_list.h:17, texture.h:120) and perlin's copy assignment leaves texture.h:54 with freed
//     tables, which refhdr_scene_from_flat replaces with the flattened scene's at once.
#include "curand_kernel.h"

#include "bvh.h"
#include "camera.h"
#include "constant_medium.h"
#include "moving_sphere.h"
#include "sphere.h"
#include "triangle.h"

#include <string.h>

#include <atomic>
#include <new>
#include <thread>

#include "../../include/rt_hip.h"  // struct layouts of the flattened scene only

#define REFHDR_API extern "C" __attribute__((visibility("default")))

namespace refhdr {
thread_local long long draws = 0;
}

// ---------------------------------------------------------------- the padded, zero-filled array heap
static const size_t kPad = 64;
void* operator new[](size_t n) {
  char* p = static_cast<char*>(calloc(1, n + 2 * kPad));
  if (!p) throw std::bad_alloc();
  return p + kPad;
}
void operator delete[](void* p) noexcept {
  if (p) free(static_cast<char*>(p) - kPad);
}
void operator delete[](void* p, size_t) noexcept {
  if (p) free(static_cast<char*>(p) - kPad);
}

// ---------------------------------------------------------------- H13
struct moving_sphere_uv0 : public moving_sphere {
  using moving_sphere::moving_sphere;
  bool hit(const ray& r, const float t_min, const float t_max, hit_record& rec, curandState* s) const override {
    if (!moving_sphere::hit(r, t_min, t_max, rec, s)) return false;
    rec.u = rec.v = 0.0f;
    return true;
  }
};
struct constant_medium_uv0 : public constant_medium {
  using constant_medium::constant_medium;
  bool hit(const ray& r, const float t_min, const float t_max, hit_record& rec, curandState* s) const override {
    if (!constant_medium::hit(r, t_min, t_max, rec, s)) return false;
    rec.u = rec.v = 0.0f;
    return true;
  }
};

struct refhdr_scene {
  hittable* world = nullptr;
  camera* cam = nullptr;
  color background;
  std::vector<texturez*> tex;
  std::vector<material*> mat;
  std::vector<hittable*> prim;
  std::vector<hittable*> obj;
  std::vector<unsigned char> texels;
};

namespace {

vec3 v3(const float* p) { return vec3(p[0], p[1], p[2]); }
bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }
bool same_v3(const vec3& a, const float* b) { return same_bits(a[0], b[0]) && same_bits(a[1], b[1]) && same_bits(a[2], b[2]); }

// x1 with fl(x1 - x0) == d bit for bit, looked for around fl(x0 + d): the flattened moving sphere stores
// center1 - center0 and time1 - time0, the reference's class the ends.
bool end_for(float x0, float d, float& x1) {
  const float mid = x0 + d;
  float lo = mid, hi = mid;
  for (int k = 0; k < 4; ++k) {
    if (same_bits(lo - x0, d)) { x1 = lo; return true; }
    if (same_bits(hi - x0, d)) { x1 = hi; return true; }
    lo = nextafterf(lo, -infinity);
    hi = nextafterf(hi, infinity);
  }
  return false;
}

struct Builder {
  const rt_scene_soa& f;
  refhdr_scene& s;
  int err = 0;
  Builder(const rt_scene_soa& ff, refhdr_scene& ss) : f(ff), s(ss) {}
  bool fail(int code) {
    if (!err) err = code;
    return false;
  }

  texturez* leaf_texture(const rt_texture& t) {
    switch (t.type) {
      case RT_TEX_SOLID: return new solid_color(v3(t.color));
      case RT_TEX_NOISE:
      case RT_TEX_TURBULENT:
      case RT_TEX_MARBLE: {
        if (t.a < 0 || t.a >= f.n_perlins) { fail(2); return nullptr; }
        const rt_perlin& tab = f.perlins[t.a];
        curandState st = {};
        perlin* pn;
        texturez* out;
        if (t.type == RT_TEX_NOISE) {
          noise_texture* x = new noise_texture(&st, t.scale);
          pn = &x->noise, out = x;
        } else if (t.type == RT_TEX_MARBLE) {
          marble_texture* x = new marble_texture(&st, t.scale);
          pn = &x->noise, out = x;
        } else {
          turbulent_texture* x = new turbulent_texture(&st, t.scale, t.b);
          pn = &x->noise, out = x;
        }
        pn->ranvec = new vec3[256];
        pn->perm_x = new int[256];
        pn->perm_y = new int[256];
        pn->perm_z = new int[256];
        for (int i = 0; i < 256; ++i) {
          pn->ranvec[i] = v3(tab.ranvec[i]);
          pn->perm_x[i] = tab.perm_x[i];
          pn->perm_y[i] = tab.perm_y[i];
          pn->perm_z[i] = tab.perm_z[i];
          if ((tab.perm_x[i] | tab.perm_y[i] | tab.perm_z[i]) & ~255) { fail(2); return nullptr; }
        }
        return out;
      }
      case RT_TEX_IMAGE: {
        if (t.a < 0 || t.a >= f.n_images) { fail(2); return nullptr; }
        const rt_image& im = f.images[t.a];
        int w = im.width, h = im.height, bpp = im.bytes_per_pixel;
        if (w <= 0) {  // no data: the reference's cyan (texture.h:146-147)
          w = h = 0;
          return new image_texture(nullptr, &w, &h, &bpp, 0);
        }
        image_texture* x = new image_texture(s.texels.data(), &w, &h, &bpp, 0);
        x->index = im.offset;
        return x;
      }
      default: fail(2); return nullptr;
    }
  }
  bool textures() {
    s.tex.assign((size_t)f.n_textures, nullptr);
    for (int k = 0; k < f.n_textures; ++k)
      if (f.textures[k].type != RT_TEX_CHECKER && !(s.tex[k] = leaf_texture(f.textures[k]))) return false;
    for (int k = 0; k < f.n_textures; ++k) {
      const rt_texture& t = f.textures[k];
      if (t.type != RT_TEX_CHECKER) continue;
      if (t.a < 0 || t.a >= f.n_textures || t.b < 0 || t.b >= f.n_textures || !s.tex[t.a] || !s.tex[t.b]) return fail(2);
      s.tex[k] = new checker_texture(s.tex[t.a], s.tex[t.b]);  // (even, odd)
    }
    return true;
  }
  bool materials() {
    for (int k = 0; k < f.n_materials; ++k) {
      const rt_material& m = f.materials[k];
      if (m.type != RT_MAT_DIELECTRIC && (m.texture < 0 || m.texture >= f.n_textures)) return fail(2);
      texturez* t = m.type != RT_MAT_DIELECTRIC ? s.tex[m.texture] : nullptr;
      switch (m.type) {
        case RT_MAT_LAMBERTIAN: s.mat.push_back(new lambertian(t)); break;
        case RT_MAT_METAL: {
          metal* x = new metal(t);  // (this constructor leaves fuzz unset)
          x->fuzz = m.param;
          s.mat.push_back(x);
          break;
        }
        case RT_MAT_DIELECTRIC: s.mat.push_back(new dielectric(m.param)); break;
        case RT_MAT_DIFFUSE_LIGHT: s.mat.push_back(new diffuse_light(t)); break;
        case RT_MAT_ISOTROPIC: s.mat.push_back(new isotropic(t)); break;
        default: return fail(2);
      }
    }
    return true;
  }
  bool prims() {
    for (int k = 0; k < f.n_prims; ++k) {
      const rt_prim& q = f.prims[k];
      const float* p = q.p;
      if (q.material < 0 || q.material >= f.n_materials) return fail(2);
      material* m = s.mat[q.material];
      switch (q.type) {
        case RT_PRIM_SPHERE: s.prim.push_back(new sphere(v3(p), p[3], m)); break;
        case RT_PRIM_MOVING_SPHERE: {
          float c1[3], t1;
          for (int a = 0; a < 3; ++a)
            if (!end_for(p[a], p[4 + a], c1[a])) return fail(6);
          if (!end_for(p[7], p[8], t1)) return fail(6);
          s.prim.push_back(new moving_sphere_uv0(v3(p), v3(c1), p[7], t1, p[3], m));
          break;
        }
        case RT_PRIM_RECT_XY:
        case RT_PRIM_RECT_XZ:
        case RT_PRIM_RECT_YZ:  // the classes recompute the extents the record stores
          if (!same_bits(p[1] - p[0], p[5]) || !same_bits(p[3] - p[2], p[6])) return fail(6);
          if (q.type == RT_PRIM_RECT_XY) s.prim.push_back(new xy_rect(p[0], p[1], p[2], p[3], p[4], m));
          else if (q.type == RT_PRIM_RECT_XZ) s.prim.push_back(new xz_rect(p[0], p[1], p[2], p[3], p[4], m));
          else s.prim.push_back(new yz_rect(p[0], p[1], p[2], p[3], p[4], m));
          break;
        case RT_PRIM_TRIANGLE: {
          if (!(p[0] >= 0.0f && p[0] < (float)f.n_triangles) || p[0] != (float)(int)p[0]) return fail(2);
          const rt_triangle& t = f.triangles[(int)p[0]];
          triangle* x = new triangle(v3(t.v0), v3(t.v1), v3(t.v2), v3(t.n0), v3(t.n1), v3(t.n2), t.uv[0], t.uv[1], t.uv[2],
                                     t.uv[3], t.uv[4], t.uv[5], m);
          x->vertex_normals = t.vertex_normals != 0;
          // the constructor's derived fields (triangle.h:25-31) stand; the record must hold the same bits
          if (!same_v3(x->v0, t.e0) || !same_v3(x->v1, t.e1) || !same_bits(x->d00, t.d00) || !same_bits(x->d01, t.d01) ||
              !same_bits(x->d11, t.d11) || !same_bits(x->invDenom, t.inv_denom))
            return fail(6);
          s.prim.push_back(x);
          break;
        }
        case RT_PRIM_BOX: s.prim.push_back(new box(v3(p), v3(p + 3), m)); break;
        default: return fail(2);
      }
    }
    return true;
  }
  // bvh.h's layout constructor, then leaves and boxes from the flat nodes (the stored boxes need not nest).
  hittable* bvh(const rt_object& o) {
    if (o.b < 2 || o.b > 20 || o.a < 0 || (long long)o.a + (1LL << o.b) - 1 > f.n_nodes) { fail(4); return nullptr; }
    const rt_bvh_node* nd = f.nodes + o.a;
    const int inner = (1 << o.b) - 1, last0 = (1 << (o.b - 1)) - 1;
    int n = 0;
    for (int k = last0; k < inner; ++k) {
      if (nd[k].leaf_a < 0 || nd[k].leaf_a >= f.n_prims || nd[k].leaf_b < -1 || nd[k].leaf_b >= f.n_prims) { fail(4); return nullptr; }
      n += nd[k].leaf_b >= 0 ? 2 : 1;
    }
    if (n < 3 || n <= (1 << (o.b - 1)) || n > (1 << o.b)) { fail(7); return nullptr; }  // not bvh_node(int)'s rows
    bvh_node* b = new bvh_node(n);
    b->objs = s.prim.data();  // ids index the scene's primitives
    b->bounds = new aabb[inner];
    for (int k = 0; k < inner; ++k) b->bounds[k] = aabb(v3(nd[k].lo), v3(nd[k].hi));
    for (int k = last0; k < inner; ++k) {
      const node_info& in = b->info[k];
      if (in.end || in.num != (nd[k].leaf_b >= 0 ? 2 : 1)) { fail(7); return nullptr; }  // another split of n
      b->info[in.left].ids = new int[1];
      b->info[in.left].ids[0] = nd[k].leaf_a;
      if (in.num == 2) {
        b->info[in.right].ids = new int[1];
        b->info[in.right].ids[0] = nd[k].leaf_b;
      }
    }
    return b;
  }
  hittable* object(int oi, unsigned allowed) {
    if (oi < 0 || oi >= f.n_objects) { fail(2); return nullptr; }
    const rt_object& o = f.objects[oi];
    if (o.kind < RT_OBJ_PRIM || o.kind > RT_OBJ_MEDIUM) { fail(2); return nullptr; }
    if (!((allowed >> o.kind) & 1u)) { fail(3); return nullptr; }
    if (s.obj[oi]) return s.obj[oi];
    hittable* h = nullptr;
    const unsigned leafs = 1u << RT_OBJ_PRIM | 1u << RT_OBJ_LIST | 1u << RT_OBJ_BVH;
    switch (o.kind) {
      case RT_OBJ_PRIM:
        if (o.a < 0 || o.a >= f.n_prims) { fail(2); return nullptr; }
        h = s.prim[o.a];
        break;
      case RT_OBJ_LIST:
        if (o.a < 0 || o.b < 1 || (long long)o.a + o.b > f.n_prims) { fail(2); return nullptr; }
        h = new hittable_list(s.prim.data() + o.a, o.b);
        break;
      case RT_OBJ_BVH:
        if (!(h = bvh(o))) return nullptr;
        break;
      case RT_OBJ_XFORM: {
        if (o.b < 0 || o.b > 3) { fail(2); return nullptr; }
        hittable* c = object(o.a, leafs);
        if (!c) return nullptr;
        if (o.b & 2) {
          rotate_y* r = new rotate_y(c, 0.0f);
          r->sin_theta = o.f[3];  // as stored
          r->cos_theta = o.f[4];
          c = r;
        }
        if (o.b & 1) c = new translate(c, v3(o.f));
        h = c;
        break;
      }
      default: {  // RT_OBJ_MEDIUM
        if (o.b < 0 || o.b >= f.n_materials) { fail(2); return nullptr; }
        hittable* c = object(o.a, leafs | 1u << RT_OBJ_XFORM);
        if (!c) return nullptr;
        constant_medium_uv0* m = new constant_medium_uv0(c, 1.0f, color(0, 0, 0));
        m->neg_inv_density = o.f[0];  // as stored
        m->phase_function = s.mat[o.b];
        h = m;
        break;
      }
    }
    s.obj[oi] = h;
    return h;
  }
  bool build() {
    if (f.n_world <= 0 || !f.world || f.n_objects <= 0 || !f.objects || f.n_materials <= 0 || !f.materials || f.n_prims < 0 ||
        f.n_textures < 0 || f.n_texels < 0)
      return fail(2);
    if (f.n_texels > 0) s.texels.assign(f.texels, f.texels + f.n_texels);
    s.texels.resize(s.texels.size() + 4);  // (a last texel of fewer than 3 bytes reads its neighbours')
    if (!textures() || !materials() || !prims()) return false;
    s.obj.assign((size_t)f.n_objects, nullptr);
    hittable** w = new hittable*[f.n_world];
    for (int k = 0; k < f.n_world; ++k)
      if (!(w[k] = object(f.world[k], 0x1fu))) return false;
    s.world = new hittable_list(w, f.n_world);
    const rt_camera& c = f.camera;
    camera* cam = new camera();
    cam->origin = v3(c.origin);
    cam->lower_left_corner = v3(c.lower_left);
    cam->horizontal = v3(c.horizontal);
    cam->vertical = v3(c.vertical);
    cam->u = v3(c.u);
    cam->v = v3(c.v);
    cam->w = v3(c.w);
    cam->lens_radius = c.lens_radius;
    cam->time0 = c.time0;
    cam->time1 = c.time1;
    s.cam = cam;
    s.background = v3(f.background);
    return true;
  }
};

curandState load_state(const uint32_t* w) {
  curandState st;
  st.d = w[0];
  for (int k = 0; k < 5; ++k) st.v[k] = w[1 + k];
  return st;
}
void store_state(const curandState& st, uint32_t* w) {
  w[0] = st.d;
  for (int k = 0; k < 5; ++k) w[1 + k] = st.v[k];
}

// One path (render.h:55-81's job): follow the ray until it leaves the scene, is absorbed, or has made
// `depth` world queries; `segments` counts the queries.
color path(const refhdr_scene& s, ray cur, curandState* st, int depth, int& segments) {
  color through(1, 1, 1);
  for (int bounce = 0; bounce < depth; ++bounce) {
    hit_record rec = {};
    ++segments;
    if (!s.world->hit(cur, 0.001f, infinity, rec, st)) return through * s.background;
    const color light = rec.mat_ptr->emitted(rec.u, rec.v, rec.p);
    ray next;
    color filter;
    if (!rec.mat_ptr->scatter(cur, rec, filter, next, st)) return through * light;
    through *= filter;
    cur = next;
  }
  return color(0, 0, 0);
}

}  // namespace

// ---------------------------------------------------------------- C API (ctypes, tests only)
// 0 on success.  2..5: a malformed scene, as ref_scene_from_flat reports it; 6: a stored derived field
// (a rect's extent, a moving sphere's centre or time difference, a triangle's edges, dot products or
// inverse denominator) that the reference's class, which computes it itself, would not hold; 7: a BVH whose leaves are not bvh_node(int)'s layout.
REFHDR_API int refhdr_scene_from_flat(const rt_scene_soa* flat, refhdr_scene** out) {
  if (!flat || !out) return 1;
  *out = nullptr;
  refhdr_scene* s = new refhdr_scene;
  Builder b(*flat, *s);
  if (!b.build()) {
    delete s;
    return b.err ? b.err : 1;
  }
  *out = s;
  return 0;
}
REFHDR_API void refhdr_scene_destroy(refhdr_scene* s) { delete s; }  // (the reference's objects stay: see the top)

// Frame buffer fb_id of a W x H image, spp samples per pixel (render.h:94-113's job).  states: W*H
// curand_init(seed, slot, 0) states of six words (d, v0..v4).  fb: W*H*3 floats, p = j*W + i, j = 0 the
// bottom row.  segments (may be NULL): W*H world-query counts.
REFHDR_API int refhdr_render(const refhdr_scene* s, int W, int H, int spp, int fb_id, int max_depth, int cam_mode,
                             const uint32_t* states, float* fb, int* segments) {
  if (!s || W <= 0 || H <= 0 || spp <= 0 || !states || !fb) return 1;
  const long long N = (long long)W * H;
  std::atomic<int> next_row{0};
  auto work = [&]() {
    for (;;) {
      const int j = next_row.fetch_add(1);
      if (j >= H) break;
      for (int i = 0; i < W; ++i) {
        const long long p = (long long)j * W + i;
        const long long slot = ((long long)(fb_id + 1) * p + fb_id + 1) % N;
        curandState own = load_state(states + 6 * slot);
        curandState lens = load_state(states);  // pristine slot 0, private to this pixel and fb (H2)
        curandState* cam_state = cam_mode == RT_CAM_PER_PIXEL ? &own : &lens;
        color sum(0, 0, 0);
        int seg = 0;
        for (int k = 0; k < spp; ++k) {
          const float u = ((float)i + random_float(&own)) / (float)W;
          const float v = ((float)j + random_float(&own)) / (float)H;
          const ray r = s->cam->get_ray(cam_state, u, v);
          sum += path(*s, r, &own, max_depth, seg);
        }
        const color mean = sum / (float)spp;
        fb[3 * p + 0] = mean.x();
        fb[3 * p + 1] = mean.y();
        fb[3 * p + 2] = mean.z();
        if (segments) segments[p] = seg;
      }
    }
  };
  const int nt = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
  return 0;
}

// The reference's build constructor (bvh.h:270-346) over primitives [first, first + n) of the scene in
// that order, from state_in.  Outputs per inner node in heap order (2^rows - 1 of them, rows =
// ceil(log2 n)): lo / hi (3 floats each); leaf_a / leaf_b: the scene primitives of a last-row node's
// leaves (-1: none; both -1 above the last row); axes: the axis random_int drew for it (:294, replayed
// from state_in with the reference's random_int; the build draws nothing else, which is checked).
REFHDR_API int refhdr_bvh_build(const refhdr_scene* s, int first, int n, float t0, float t1, const uint32_t* state_in,
                                int32_t* leaf_a, int32_t* leaf_b, float* lo, float* hi, int32_t* axes, uint32_t* state_out) {
  if (!s || n < 3 || first < 0 || (size_t)first + n > s->prim.size()) return 1;
  curandState st = load_state(state_in);
  hittable** hits = const_cast<hittable**>(s->prim.data()) + first;
  const long long before = refhdr::draws;
  bvh_node* b = new bvh_node(hits, n, t0, t1, &st);
  const int inner = b->num_nodes() - n;
  if (refhdr::draws - before != inner) return 8;
  int rows = 0;
  while ((1 << rows) < n) ++rows;
  if (inner != (1 << rows) - 1) return 9;
  curandState replay = load_state(state_in);
  for (int k = 0; k < inner; ++k) {
    axes[k] = random_int(&replay, 0, 2);
    leaf_a[k] = leaf_b[k] = -1;
    for (int a = 0; a < 3; ++a) {
      lo[3 * k + a] = b->bounds[k].min()[a];
      hi[3 * k + a] = b->bounds[k].max()[a];
    }
    const node_info& in = b->info[k];
    if (k >= (1 << (rows - 1)) - 1) {
      leaf_a[k] = first + b->info[in.left].ids[0];
      if (in.num == 2) leaf_b[k] = first + b->info[in.right].ids[0];
    }
  }
  store_state(st, state_out);
  return 0;
}

// camera.h's constructor (:18-47): the vectors it derives, in rt_camera's layout.
REFHDR_API int refhdr_camera_build(const float* from, const float* at, const float* vup, float vfov, float aspect, float aperture,
                                   float focus, float t0, float t1, rt_camera* out) {
  const camera c(v3(from), v3(at), v3(vup), vfov, aspect, aperture, focus, t0, t1);
  for (int a = 0; a < 3; ++a) {
    out->origin[a] = c.origin[a];
    out->lower_left[a] = c.lower_left_corner[a];
    out->horizontal[a] = c.horizontal[a];
    out->vertical[a] = c.vertical[a];
    out->u[a] = c.u[a];
    out->v[a] = c.v[a];
    out->w[a] = c.w[a];
  }
  out->lens_radius = c.lens_radius;
  out->time0 = c.time0;
  out->time1 = c.time1;
  return 0;
}

// What rotate_y's constructor (hittable.h:77-81) and constant_medium's (constant_medium.h:15-16) derive
// from an angle in degrees and a density: out = sin_theta, cos_theta, neg_inv_density.
REFHDR_API int refhdr_instance_consts(float angle, float density, float* out) {
  sphere* ball = new sphere(vec3(0, 0, 0), 1.0f, nullptr);
  const rotate_y r(ball, angle);
  const constant_medium m(ball, density, color(0, 0, 0));
  out[0] = r.sin_theta;
  out[1] = r.cos_theta;
  out[2] = m.neg_inv_density;
  return 0;
}

// perlin.h's constructor from state_in: ranvec (256 x 3 floats), the three permutations (256 ints each).
REFHDR_API int refhdr_perlin_build(const uint32_t* state_in, float* ranvec, int32_t* perm_x, int32_t* perm_y, int32_t* perm_z,
                                   uint32_t* state_out) {
  curandState st = load_state(state_in);
  perlin* p = new perlin(&st);
  for (int i = 0; i < 256; ++i) {
    for (int a = 0; a < 3; ++a) ranvec[3 * i + a] = p->ranvec[i][a];
    perm_x[i] = p->perm_x[i];
    perm_y[i] = p->perm_y[i];
    perm_z[i] = p->perm_z[i];
  }
  store_state(st, state_out);
  return 0;
}
