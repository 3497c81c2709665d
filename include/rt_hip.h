/* rt_hip.h — C ABI of the MI355X (gfx950) path-tracing hot path.
 *
 * Drop-in replacement for the per-pixel render path of daRoyalCacti/Raytracing_GPU:
 *
 *   rt_render_init   replaces  __global__ render_init(W, H, curandState*)        render.h:84-92
 *   rt_render        replaces  __global__ render(fb, W, H, ns, cam, states, world,
 *                                                max_depth, id, background)     render.h:94-113
 *                              (and color_f, render.h:55-81, plus everything it calls:
 *                               bvh.h:348-436, aabb.h:19-104, hittable_list.h:23-39,
 *                               sphere.h, moving_sphere.h, aarect.h, box.h, hittable.h:31-143,
 *                               constant_medium.h, material.h, texture.h, perlin.h)
 *   rt_resolve       replaces  write_frame_buffer + average_images (the per-fb 8-bit quantise
 *                              and square-average of draw())            color.h:19-170
 *   rt_scene_upload  replaces  the device-side object graph that struct scene's constructor
 *                              builds with <<<1,1>>> kernels            scenes.h:36-79
 *   rt_draw          replaces  void draw(scene&, render_settings)       render.h:118-174
 *
 * Conventions (render.h:99): a frame buffer is row-major, p = j*W + i, j = 0 the BOTTOM row,
 * 3 floats per pixel.  Every call returns 0 on success or a nonzero rt_status; rt_last_error()
 * gives the message.  Nothing exits or throws across the boundary (the reference's
 * checkCudaErrors -> exit(99), common.h:30-38, becomes a status code).  A context belongs to one
 * device and one host thread at a time.  Calls are synchronous unless named _async.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum rt_status {
  RT_OK = 0,
  RT_ERR_ARG = 1,     /* invalid argument / shape */
  RT_ERR_HIP = 2,     /* HIP runtime error */
  RT_ERR_STATE = 3,   /* call order (e.g. render before upload) */
  RT_ERR_SCENE = 4,   /* malformed scene arrays */
  RT_ERR_NOMEM = 5
};

/* ------------------------------------------------------------------ flattened scene (host) */
/* Camera as built by camera::camera(), camera.h:18-47. */
typedef struct rt_camera {
  float origin[3], lower_left[3], horizontal[3], vertical[3];
  float u[3], v[3], w[3];
  float lens_radius, time0, time1;
} rt_camera;

enum rt_prim_type {
  RT_PRIM_SPHERE = 0,        /* sphere.h          p = cx cy cz r                           */
  RT_PRIM_MOVING_SPHERE = 1, /* moving_sphere.h   p = c0x c0y c0z r  dx dy dz t0  dt
                                                  (d = center1-center0, dt = time1-time0)   */
  RT_PRIM_RECT_XY = 2,       /* aarect.h xy_rect  p = x0 x1 y0 y1 k  (x1-x0) (y1-y0)        */
  RT_PRIM_RECT_XZ = 3,       /* aarect.h xz_rect  p = x0 x1 z0 z1 k  (x1-x0) (z1-z0)        */
  RT_PRIM_RECT_YZ = 4,       /* aarect.h yz_rect  p = y0 y1 z0 z1 k  (y1-y0) (z1-z0)        */
  RT_PRIM_TRIANGLE = 5,      /* triangle.h        p[0] = index into rt_scene_soa.triangles  */
  RT_PRIM_BOX = 6            /* box.h: the list of six rects  p = x0 y0 z0 x1 y1 z1         */
};
/* 48-byte primitive record; three 16-byte loads on the device. */
typedef struct rt_prim {
  float p[10];
  int32_t type;
  int32_t material;
} rt_prim;

/* Triangle (triangle.h:19-41 constructor output), 144 bytes. */
typedef struct rt_triangle {
  float v0[3], v1[3], v2[3];
  float e0[3], e1[3];        /* vertex1-vertex0, vertex2-vertex0 (triangle.h:26-27) */
  float d00, d01, d11, inv_denom;
  float uv[6];               /* u0 v0 u1 v1 u2 v2 */
  float n0[3], n1[3], n2[3];
  int32_t vertex_normals;
  int32_t pad;
} rt_triangle;

/* Inner node of a reference-layout BVH (bvh.h:133-346): a perfect binary tree of `rows` inner
 * levels stored in heap order (children of k are 2k+1, 2k+2).  Nodes of the last inner level
 * carry the one or two primitives of their leaves in leaf_a / leaf_b (-1 = none); nodes above it
 * carry their split axis (0..2, drawn at build time) in leaf_a and -1 in leaf_b. */
typedef struct rt_bvh_node {
  float lo[3];
  int32_t leaf_a;
  float hi[3];
  int32_t leaf_b;
} rt_bvh_node;

enum rt_object_kind {
  RT_OBJ_PRIM = 0,   /* a = prim index                                                         */
  RT_OBJ_LIST = 1,   /* a = first prim, b = count; hittable_list semantics (box.h)             */
  RT_OBJ_BVH = 2,    /* a = first node, b = rows (inner levels)                                */
  RT_OBJ_XFORM = 3,  /* translate(rotate_y(child)), hittable.h:31-143; a = child object
                        (PRIM/LIST/BVH), b = flags (1 translate, 2 rotate_y);
                        f[0..2] = offset, f[3] = sin, f[4] = cos                               */
  RT_OBJ_MEDIUM = 4  /* constant_medium.h; a = boundary object (PRIM/LIST/BVH/XFORM),
                        b = phase material, f[0] = -1/density                                  */
};
typedef struct rt_object {
  int32_t kind, a, b, c;
  float f[8];
} rt_object;

enum rt_material_type {
  RT_MAT_LAMBERTIAN = 0, RT_MAT_METAL = 1, RT_MAT_DIELECTRIC = 2,
  RT_MAT_DIFFUSE_LIGHT = 3, RT_MAT_ISOTROPIC = 4
};
typedef struct rt_material {
  int32_t type;
  int32_t texture; /* albedo / emit texture (unused by dielectric) */
  float param;     /* metal fuzz or dielectric index of refraction */
  int32_t pad;
} rt_material;

enum rt_texture_type {
  RT_TEX_SOLID = 0, RT_TEX_CHECKER = 1, RT_TEX_NOISE = 2, RT_TEX_TURBULENT = 3,
  RT_TEX_MARBLE = 4, RT_TEX_IMAGE = 5
};
typedef struct rt_texture {
  int32_t type;
  int32_t a;       /* checker: even texture; noise/turb/marble: perlin table; image: image   */
  int32_t b;       /* checker: odd texture; turbulent: depth                                  */
  int32_t pad;
  float color[3];  /* solid colour                                                            */
  float scale;     /* noise scale                                                             */
} rt_texture;

/* Perlin tables (perlin.h:9-34). */
typedef struct rt_perlin {
  float ranvec[256][3];
  int32_t perm_x[256], perm_y[256], perm_z[256];
} rt_perlin;

/* Image texture (texture.h:97-164): width, height, bytes per pixel, byte offset into texels. */
typedef struct rt_image {
  int32_t width, height, bytes_per_pixel;
  int32_t offset;
} rt_image;

typedef struct rt_scene_soa {
  rt_camera camera;
  float background[3];
  float aspect;
  const int32_t* world;          int32_t n_world;   /* top-level hittable_list */
  const rt_object* objects;      int32_t n_objects;
  const rt_prim* prims;          int32_t n_prims;
  const rt_triangle* triangles;  int32_t n_triangles;
  const rt_bvh_node* nodes;      int32_t n_nodes;
  const rt_material* materials;  int32_t n_materials;
  const rt_texture* textures;    int32_t n_textures;
  const rt_perlin* perlins;      int32_t n_perlins;
  const rt_image* images;        int32_t n_images;
  const uint8_t* texels;         int64_t n_texels;
} rt_scene_soa;

/* ------------------------------------------------------------------ render arguments */
enum rt_cam_mode {
  RT_CAM_REF_SLOT0 = 0, /* reference mode: lens/time draws from a private copy of
                           the pristine slot-0 state, restarted per pixel and per fb        */
  RT_CAM_PER_PIXEL = 1  /* lens/time draws from the pixel's own state                       */
};

/* rt_render_args.flags */
#define RT_FLAG_EXACT_TRAVERSAL 1 /* visit exactly the reference's BVH node set (bvh.h:348-436)
                                     instead of the margin-culled near-first traversal; both give
                                     the same pixels, only node/prim test counts differ          */
#define RT_FLAG_NO_LDS 4          /* keep the scene in global memory even when it fits in LDS   */
#define RT_FLAG_AUDIT 2           /* run both traversals per BVH query, keep the exact result and
                                     log every disagreement (read back with rt_audit_log)       */
#define RT_FLAG_WIDEST 8          /* testing: run the widest compiled kernel variant that covers
                                     the scene instead of the narrowest (same pixels)           */
#define RT_FLAG_NO_STEP 16        /* testing: world = one BVH still runs the segment-per-trip
                                     kernel instead of the stepwise one (same pixels)           */
#define RT_FLAG_NO_SCHEDULE 32    /* natural item order on every launch (no longest-first
                                     schedule from the previous launch; same pixels)            */
#define RT_FLAG_NO_CAMERA_BINS 64 /* camera rays traverse the BVH instead of testing their 8x8
                                     tile's candidate list (world = one BVH; same pixels)       */
#define RT_FLAG_NO_SPLIT 128      /* never split the samples of the longest items over work items
                                     on warm launches (stepwise kernel; same pixels)            */
#define RT_FLAG_FRESH 256         /* forget the context's item schedule first: the launch runs as
                                     the first launch of its configuration does (benchmarks of a
                                     one-shot draw; same pixels)                                */

typedef struct rt_render_args {
  int32_t width, height;  /* full image size; N = width*height drives the RNG slots (H3)  */
  int32_t spp;            /* samples_per_pixel_per_fb (render.h:24)                      */
  int32_t fb_first;       /* first frame-buffer id `id` (render.h:154)                   */
  int32_t fb_count;       /* number of consecutive fb ids rendered by this call          */
  int32_t max_depth;      /* render.h:27                                                 */
  int32_t cam_mode;       /* rt_cam_mode                                                 */
  int32_t band_rows;      /* row tiling: rows grouped in bands of band_rows (>= 1)       */
  int32_t band_first;     /* this call renders bands b = band_first, +band_stride, ...   */
  int32_t band_stride;
  int32_t stats;          /* 1: also count BVH node and primitive tests                  */
  int32_t flags;          /* RT_FLAG_*                                                   */
  uint64_t seed;          /* 1984 in the reference (render.h:91)                         */
} rt_render_args;

typedef struct rt_counters {
  uint64_t segments;      /* top-level world->hit queries, primary + bounces (render.h:63) */
  uint64_t node_tests;    /* stats only: BVH box tests                                     */
  uint64_t prim_tests;    /* stats only: primitive hit() tests                             */
  uint64_t samples;
  uint64_t fallbacks;     /* stats only: culled BVH queries re-run on the reference visit set */
} rt_counters;

typedef struct rt_ctx rt_ctx;

/* ------------------------------------------------------------------ context */
int rt_ctx_create(int hip_device, rt_ctx** out);
int rt_ctx_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);

/* Implementation options of a context.  None of them changes a pixel or a segment count (every
 * setting is parity-tested against the oracle); they choose kernel variants, search algorithms and
 * schedule thresholds.  rt_ctx_options_default gives the measured product configuration, which a new
 * context starts with; the library reads no environment variable.  The upload-time fields apply from
 * the next rt_scene_upload; rt_ctx_set_options also drops the context's item schedule, so the next
 * launch of any configuration is a cold one. */
enum rt_merge_mode {
  RT_MERGE_ON = 0,           /* list worlds of primitives, BVHs, instances and inert media: one
                                candidate search over every entry (world_search)                 */
  RT_MERGE_OFF = 1,          /* the per-entry list loop of hittable_list.h:23-39 (world_hit)     */
  RT_MERGE_FALLBACK_ALL = 2  /* testing: run the search, then answer every query exactly         */
};
enum rt_merge_order {
  RT_ORDER_DISTANCE = 0,     /* merged search visits primitives, then BVHs / instances nearest the
                                camera first, then inert media                                    */
  RT_ORDER_LIST = 1,         /* the list's own order                                               */
  RT_ORDER_REVERSED = 2      /* testing: the list reversed                                         */
};
typedef struct rt_ctx_options {
  /* upload time (rt_scene_upload) */
  int32_t world_tree;        /* 1: a list world flattened into ONE traversal tree for the stepwise
                                kernel (measured slower than the merged search; default 0).  This
                                and the other 0/1 fields reject any other value                    */
  int32_t quantized_tree;    /* 1: the world BVH's traversal tree as 24-byte records in LDS when it
                                fits (C4's mesh; default 1)                                         */
  int32_t merged_search;     /* rt_merge_mode (default RT_MERGE_ON)                                */
  int32_t merge_order;       /* rt_merge_order (default RT_ORDER_DISTANCE)                         */
  int32_t dedup_triangles;   /* 1: coincident triangles leave the traversal trees, the first of a
                                group stands for it (default 1)                                     */
  /* per launch (rt_render) */
  int32_t shade_min;         /* stepwise kernel: lanes waiting before a wave shades; 0 = the
                                variant's measured value (60, 48 for triangle meshes)               */
  float bins_min_items_per_lane; /* camera-ray tile lists from this many items per resident lane
                                (default 6; 0 = always)                                             */
  float split_min_segments;  /* > 0: split the samples of items of at least this many segments;
                                0 = the share-size rule (default)                                   */
  int32_t split_order;       /* 1: split samples and unsplit items claimed in one longest-first
                                sequence (default); 0: split samples first, in item order          */
  int32_t cost_shift;        /* item-schedule cost buckets of 2^cost_shift segments, 0..12; -1 =
                                automatic                                                           */
  float long_pct;            /* share of the longest items whose waves run at raised priority
                                (default 2)                                                         */
  int32_t probe_schedule;    /* k > 0: the first launch of a configuration (>= 4 samples per pixel,
                                a scene with BVHs) claims its items longest first by a probe
                                launch's estimate: sample 0 of the first fb at every k-th row and
                                pixel (output discarded), smoothed over neighbouring grid points;
                                -1 (default): the smallest k with k*k*spp*fb_count >= 200; 0: natural
                                order; at most 64                                                   */
  float probe_max_items_per_lane; /* > 0: probe only launches with fewer items per resident lane (a
                                multi-GPU share); 0 (default): any launch                           */
  int32_t probe_depth;       /* k > 0: a probe sample's path ends after k segments (the probe launch
                                lasts as long as its longest path); 0: the launch's max_depth; -1
                                (default): 10 for the stepwise kernel, 20 for the others            */
  int32_t spread_first;      /* k = 1..64: a probe-ordered first launch gives each wave's first
                                claim k of the order's first k x waves items, strided (one wave
                                does not start with many of the longest), and 64 - k neighbours
                                in order; 0: the order as is; -1 (default): automatic              */
} rt_ctx_options;
void rt_ctx_options_default(rt_ctx_options* opts);
int rt_ctx_set_options(rt_ctx* ctx, const rt_ctx_options* opts);
int rt_ctx_get_options(const rt_ctx* ctx, rt_ctx_options* opts);
/* Rows of the image owned by a band tiling (ascending); returns the count. rows may be NULL. */
int32_t rt_owned_rows(const rt_render_args* a, int32_t* rows);

/* Checks a flattened scene on the host (no context, no HIP call): every index, count and type, the
 * nesting rt_object_kind documents (which rules out cycles), the last BVH row's leaf_a (a primitive)
 * and leaf_b (a primitive or -1), and the image records.  Beyond the struct comments above it holds
 * a scene to this: a primitive is a leaf of at most one BVH, once, and is then not also named by a
 * PRIM or LIST object; a checker's two textures are not checkers; perlin permutation entries are
 * 0..255; a turbulence depth is 0..64; a triangle primitive's p[0] is a whole number below 2^19; an
 * image with width <= 0 has no data (the reference's cyan), any other has height > 0, 1..4 bytes per
 * pixel, and the three bytes pixel[0..2] of its last texel inside texels (texture.h:160-162 reads
 * three bytes whatever bytes_per_pixel is: with 1 or 2 the row-major neighbours'); no sphere of a
 * BVH (in the world, under a transform or as a medium's boundary; a moving one at both ends of the
 * shutter) lies inside the camera's view cone more than 512 radii from the camera.  Returns RT_OK or
 * RT_ERR_SCENE with the reason in msg (cap bytes, may be NULL).
 *
 * What is promised for a scene that passes: the reference's objects' pixels and segment counts, bit
 * for bit, as far as sphere.h's float test resolves its spheres.  Its discriminant hb^2 - a cc carries a
 * rounding error of the order of 2^-23 a L^2 (L = distance from the ray's origin to the centre), so the
 * reference reports a BVH sphere "hit" by rays that pass up to sqrt(r^2 + 2^-23 L^2) from its centre,
 * wherever its stored boxes let the test run; the culled search tests a sphere only where the ray
 * enters the sphere's own box (padded by 2^-16), and the camera-ray tile lists where it enters the tile.
 * Not promised, therefore: the outcome of a query whose ray starts more than 512 radii from a BVH sphere
 * and passes it within that error zone but outside its box.  The rule above keeps camera rays out of that
 * case; a bounce ray can get there (a path that leaves a far surface towards a small sphere), which no
 * check at upload can rule out.  RT_FLAG_EXACT_TRAVERSAL has no such case. */
int rt_scene_validate(const rt_scene_soa* scene, char* msg, size_t cap);

/* Copies the flattened scene to device memory owned by the context; rt_scene_validate first. */
int rt_scene_upload(rt_ctx* ctx, const rt_scene_soa* scene);

/* Per-slot XORWOW states curand_init(seed, slot, 0) for slot < width*height (render.h:84-92). */
int rt_render_init(rt_ctx* ctx, int32_t width, int32_t height, uint64_t seed);
/* Copies states [first, first+count) to host as 6 words each: d, v0..v4 (the curandStateXORWOW
 * words the reference's render_init leaves in its state array). */
int rt_read_states(rt_ctx* ctx, int64_t first, int64_t count, uint32_t* out);

/* Renders fb ids [fb_first, fb_first+fb_count) for the owned rows into fb: layout
 * [fb_count][owned_rows][width][3] floats, owned rows ascending.  fb may be a device (or managed)
 * pointer, written by the kernel directly, or a host pointer (pinned or pageable): then the frame
 * buffers are rendered into a temporary device buffer and copied back before the call returns.
 * counters may be NULL. */
int rt_render(rt_ctx* ctx, const rt_render_args* args, float* fb, rt_counters* counters);
/* Device time in ms of the last rt_render call, from HIP events recorded on the context stream: a first
 * launch's probe launch and item schedule (RT_SCHED_PROBE) included, the host staging of a host fb
 * excluded. */
float rt_last_render_ms(const rt_ctx* ctx);
/* ... of its render kernel alone (with the split-sample merge after it, RT_SCHED_SPLIT_REPLAY). */
float rt_last_kernel_ms(const rt_ctx* ctx);
/* Kernel of the last render launch as rocprof names it (stem, e.g. "render_step_kernel<25730>"):
 * the kernel variant the context picked for the scene's features and flags. */
const char* rt_last_render_kernel(const rt_ctx* ctx);
/* How the last render launch ordered its work (RT_SCHED_* bits; 0 = a cold launch: nothing from an
 * earlier launch of the same configuration was used). */
#define RT_SCHED_PREVIOUS 1     /* items claimed longest first by the segment counts of an earlier
                                   launch of this configuration (same scene, size, spp, depth, fb
                                   range, tiling and camera mode)                               */
#define RT_SCHED_SPLIT_REPLAY 2 /* split samples started from RNG states an earlier launch recorded */
#define RT_SCHED_PROBE 4        /* items claimed longest first by a probe launch's estimate (the
                                   first launch of a configuration, options.probe_schedule)     */
int32_t rt_last_render_schedule(const rt_ctx* ctx);
/* Which body of render_step_kernel the last render launch ran: 1 = the plain one (the sphere stepwise
 * variants, for a launch that splits no samples and has at most 2^32 items, width, height and fb_count
 * at most 65536), 0 = the general one, and every other kernel.  The frame buffers do not depend on it.
 * The general body of a variant that has both is a kernel of the same name one namespace down: rocprof
 * lists it as "general::render_step_kernel<25730>", and rt_last_render_kernel reports the same stem for
 * both. */
int32_t rt_last_render_body(const rt_ctx* ctx);

/* Debug view of the item schedule: what the context holds after the last rt_render.  Read
 * only: neither call changes what a later launch does, and rt_render does no work for them (the fields
 * below are host values it has anyway).  rt_render_tiles leaves everything here as it was. */
typedef struct rt_schedule_info {
  int64_t items;        /* items of the configuration whose counts RT_SCHED_ITEM_COST holds (0: none) */
  int64_t n_long;       /* positions of the raised-priority prefix of RT_SCHED_PERM */
  int64_t n_split;      /* positions of RT_SCHED_PERM whose samples are split */
  int64_t rest_n;       /* unsplit positions (items - n_split) the claim order was sized for, -1: none */
  int64_t pitems;       /* probe grid of the last probe launch: prow * pw points (0: no probe launch yet) */
  int64_t spread_waves; /* waves of the last probe launch's render kernel */
  int32_t split_state;  /* -1 nothing to split, 0 the next launch records, 1 recorded */
  int32_t order_ok;     /* RT_SCHED_ORDER is built */
  int32_t perm_kind;    /* what RT_SCHED_PERM holds: 0 nothing, 1 a measured schedule, 2 a probe's */
  int32_t shift;        /* cost buckets of 2^shift segments in that schedule (-1: none) */
  int32_t spp;          /* samples per item of that schedule's configuration */
  int32_t ps, prow, pw; /* probe grid step, rows and columns */
  int32_t spread_ran;   /* the last probe schedule's head was spread (spread_head_kernel ran) */
  int32_t spread_top;   /* ... with this many strided positions per chunk of 64 (options.spread_first) */
  int32_t perm_key_valid;    /* a later launch of the same configuration would claim through RT_SCHED_PERM */
  int32_t pending_key_valid; /* ... would build its schedule from RT_SCHED_ITEM_COST */
} rt_schedule_info;
int rt_schedule_get_info(const rt_ctx* ctx, rt_schedule_info* info);
/* Copies one device array of the schedule to the host after waiting for the context's stream.  which: */
#define RT_SCHED_ITEM_COST 0    /* uint16[items]: segments of every item in the measuring launch       */
#define RT_SCHED_PERM 1         /* uint32[items]: the claim order of the items                          */
#define RT_SCHED_PROBE_RAW 2    /* uint16[pitems]: the probe launch's segment counts                    */
#define RT_SCHED_PROBE_SMOOTH 3 /* uint16[pitems]: their neighbourhood means in 1/16 segment           */
#define RT_SCHED_SPLIT_LEN 4    /* uint8[n_split * spp]: recorded segments of every split sample (<=255),
                                   computed into a temporary from the recorded sample starts            */
#define RT_SCHED_ORDER 5        /* uint32[n_split * spp + rest_n]: claim order of a split replay        */
/* *need (may be NULL) receives the array's size in bytes, as rt_accum_save reports its blob's: out = NULL
 * with cap_bytes = 0 asks for the size; a smaller cap_bytes is RT_ERR_ARG with nothing copied. RT_ERR_STATE when the array does not exist (nothing
 * measured, no probe launch, nothing recorded, order not built); RT_ERR_ARG for another `which`. */
int rt_schedule_read(rt_ctx* ctx, int32_t which, void* out, size_t cap_bytes, size_t* need);

/* Debug view of the camera-ray culling tables: the per-tile candidate lists (world = one
 * BVH, the stepwise kernel) or top-level entry masks (list worlds) the context holds, and the bounding
 * spheres they were built from.  Read only, as the schedule view above: rt_render and rt_render_tiles only
 * store host values they have anyway. */
typedef struct rt_camera_tiles_info {
  int32_t kind;       /* what the tile buffer holds for the uploaded scene: 0 nothing valid, 1 lists, 2 masks */
  int32_t width, height;     /* image size the table was built for (0 when kind = 0) */
  int32_t tiles_x, tiles_y;  /* tiles of (1 << tile_shift)^2 pixels, the last column / row partial */
  int32_t cap;        /* pairs per tile list (a fuller tile has count -1 and traverses the tree) */
  int32_t tile_shift;
  int32_t n;          /* bounding spheres of the uploaded scene (RT_CTILES_SPHERES) */
  int32_t n_kind;     /* ... of: 0 none, 1 the world BVH's primitives, 2 the world list's entries */
  int32_t last_used;  /* what the last rt_render / rt_render_tiles launch passed to its kernel: 0 nothing,
                         1 lists, 2 masks */
} rt_camera_tiles_info;
int rt_camera_tiles_get_info(const rt_ctx* ctx, rt_camera_tiles_info* info);
/* Copies one array to the host after waiting for the context's stream.  which: */
#define RT_CTILES_COUNT 0   /* int32[tiles]: pairs of every tile's list, -1 = overflowed (lists)            */
#define RT_CTILES_ENTRIES 1 /* int32[tiles * cap * 2]: (primitive id, float bits of `nearest`) pairs, ascending
                               by `nearest`; only the first count pairs of a tile are defined (lists)      */
#define RT_CTILES_MASK 2    /* uint32[tiles]: bit w set = a camera ray of the tile may hit entry w (masks)  */
#define RT_CTILES_SPHERES 3 /* float[4 * n]: centre and radius of every bounding sphere                     */
#define RT_CTILES_IDS 4     /* int32[n]: the primitive every sphere stands for (n_kind = 1)                 */
/* Sizes and errors as rt_schedule_read: RT_ERR_STATE when the array does not exist (no table of that kind,
 * no spheres), RT_ERR_ARG for another `which` or a buffer that is too small. */
int rt_camera_tiles_read(rt_ctx* ctx, int32_t which, void* out, size_t cap_bytes, size_t* need);
/* Audit log of the last RT_FLAG_AUDIT render: 16 floats per disagreeing BVH query (ray o[3] d[3]
 * time, tmin, tmax, culled t, culled prim (int bits), exact t, exact prim, culled rank, 0, 0).
 * Copies up to cap entries into out (may be NULL); returns the total number of disagreements. */
int rt_audit_log(rt_ctx* ctx, float* out, int32_t cap);

/* Quantise each fb (write_frame_buffer) and square-average them in fb order (average_images)
 * for the owned rows: out = [owned_rows][width][3] bytes, owned rows ascending (row 0 of a PNG is
 * image row height-1).  fb and out may each be a device or a host pointer (host buffers are
 * staged through temporary device memory). */
int rt_resolve(rt_ctx* ctx, const rt_render_args* args, const float* fb, uint8_t* out);

/* draw(): init + render every fb + resolve, whole image, host output in PNG row order
 * (top row first), W*H*3 bytes.  counters may be NULL. */
int rt_draw(rt_ctx* ctx, const rt_render_args* args, uint8_t* png_rgb_host, rt_counters* counters);

/* ------------------------------------------------------------------ progressive accumulator */
/* draw() one frame buffer at a time (render.h:152-162 writes tmp/<id>.ppm after each fb,
 * average_images folds the files at the end, color.h:57-170).  The image of k frame buffers is
 * quant(sum / k) with sum += float(c*c) / (255*255) per fb in fb order, so the float sums and the
 * count are the whole state: an accumulator can be previewed, saved and continued after any fb, and
 * continuing is bit-identical to never having stopped.  An accumulator belongs to its context (and
 * must be destroyed before it); it holds owned_rows x width x 3 float sums and a float frame-buffer
 * scratch of chunk_fbs frame buffers, nothing else. */
typedef struct rt_accum rt_accum;
typedef struct rt_accum_info {
  rt_render_args args;    /* as given to rt_accum_create; fb_count = frame buffers folded in so far */
  int64_t n_values;       /* owned_rows x width x 3                                              */
  uint64_t scene_fp;      /* FNV-1a of the uploaded scene's arrays, camera and background         */
} rt_accum_info;

/* args fixes width, height, spp, max_depth, cam_mode, flags, seed and the band tiling; fb_first is
 * the first fb id, fb_count is ignored.  chunk_fbs >= 1: frame buffers per rt_render launch. */
int rt_accum_create(rt_ctx* ctx, const rt_render_args* args, int32_t chunk_fbs, rt_accum** out);
/* Renders the next `count` fb ids (rt_render, at most chunk_fbs per launch) and folds them in.
 * counters may be NULL; it receives this call's totals.  RT_ERR_STATE after another rt_scene_upload. */
int rt_accum_add(rt_accum* acc, int32_t count, rt_counters* counters);
/* Folds in `count` frame buffers the caller rendered: [count][owned_rows][width][3] floats, device
 * or host pointer. */
int rt_accum_add_fbs(rt_accum* acc, const float* fb, int32_t count);
/* Image of the frame buffers folded in so far.  png_order = 0: rt_resolve's layout (owned rows
 * ascending, device or host out).  png_order = 1: rt_draw's (whole-image tiling only, top row first,
 * host out).  RT_ERR_STATE with no frame buffer yet. */
int rt_accum_image(rt_accum* acc, uint8_t* out, int32_t png_order);
int rt_accum_get_info(const rt_accum* acc, rt_accum_info* info);
/* Device time in ms, from HIP events on the context stream, of the last accumulate launch (the last
 * chunk of rt_accum_add, or rt_accum_add_fbs) and of the last rt_accum_image's kernel; 0 before one. */
float rt_accum_last_add_ms(const rt_accum* acc);
float rt_accum_last_image_ms(const rt_accum* acc);
int rt_accum_destroy(rt_accum* acc);
/* Checkpoint blob (little-endian): 8 bytes magic "RTACCUM1", u32 version (1), u32 header size (96),
 * the 13 rt_render_args fields in order (12 x i32, u64 seed), i64 n_values, u64 scene_fp,
 * u64 FNV-1a of the payload; then n_values float sums.  rt_accum_save writes *need (may be NULL)
 * and, when cap >= need, the blob (blob = NULL with cap = 0 asks for the size); a smaller cap is
 * RT_ERR_ARG.  rt_accum_load returns RT_ERR_STATE when the context's scene differs from the blob's. */
int rt_accum_save(rt_accum* acc, void* blob, size_t cap, size_t* need);
int rt_accum_load(rt_ctx* ctx, const void* blob, size_t n, int32_t chunk_fbs, rt_accum** out);
/* Host only (no context, no GPU; csrc/rt_accum_blob.cpp): validate a blob (magic, version, size
 * against n_values and the tiling, checksum) and fill info; finalise it into the 8-bit image
 * (rt_resolve's layout, n_values bytes); build a blob from an info and its float sums. */
int rt_accum_blob_info(const void* blob, size_t n, rt_accum_info* info);
int rt_accum_blob_image(const void* blob, size_t n, uint8_t* out);
int rt_accum_blob_pack(const rt_accum_info* info, const float* sums, void* blob, size_t cap, size_t* need);

/* ------------------------------------------------------------------ noise monitor */
/* Is the image finished?  Every frame buffer is an independent estimate of the picture, and
 * average_images only sees its 8-bit quantisation, so the spread of c^2 across frame buffers, per
 * pixel, is the noise of the final image.  A monitor rides on an accumulator and keeps the first two
 * moments of c^2 as integers: exact, independent of order and grouping, identical across chunks,
 * checkpoints and band shares.  It changes no pixel; an accumulator without one launches the kernels
 * it launched before.
 *
 * For every accumulator value k (a channel of an owned pixel), over the n frame buffers folded in
 * since the monitor was created, with c = quant(fb[f][k]) as in accum_add_kernel:
 *
 *   S1[k] = sum of c^2   (u32)
 *   S2[k] = sum of c^4   (u64)
 *
 * A monitor accepts at most 32 768 frame buffers; a fold that would exceed this returns RT_ERR_ARG
 * before anything is rendered or written.  With that cap every quantity below fits in unsigned 64-bit
 * arithmetic: c^2 <= 65 025 and c^4 < 2^32, so n S2 <= 4.6e18 and S1^2 <= 4.6e18, and the
 * three-channel sum is <= 1.4e19 < 2^64.
 *
 * Per pixel, over its three channels j:
 *
 *   D = sum_j (n S2_j - S1_j^2)    (u64; each term is >= 0 by Cauchy-Schwarz)
 *   S = sum_j S1_j                 (u64)
 *
 * In double, with operations in exactly this order:
 *
 *   a     = (double)D / (3.0 * n * n * (n - 1) * 4228250625.0)   mean over channels of var(x)/n, x = c^2/65025
 *   m     = (double)S / (3.0 * n * 65025.0);  if (m < 0x1p-16) m = 0x1p-16;
 *   noise = (float)(128.0 * sqrt(a / m))
 *
 * noise is the standard error of the pixel in 8-bit output levels: the output level is 256 sqrt(m),
 * so an error dm moves it by 128 dm / sqrt(m).  It is 0 for a pixel whose frame buffers all agree,
 * and it needs n >= 2 (otherwise RT_ERR_STATE).
 *
 * Tiles are 16 x 16 pixels over (owned-row index, column), row-major (tile ty * tiles_x + tx); edge
 * tiles are partial.  For a band tiling the row index is the position in the list of rt_owned_rows. */
typedef struct rt_noise rt_noise;
typedef struct rt_noise_report {
  int32_t fbs, tiles_x, tiles_y, pad;
  int64_t pixels, pixels_above;     /* owned pixels; those with noise > threshold */
  float threshold, max_noise;
} rt_noise_report;

/* Attaches a monitor to an accumulator that has folded in no frame buffer and has no monitor
 * (RT_ERR_STATE otherwise: a monitor sees every frame buffer or none).  While it is attached every
 * fold also updates it (one fused kernel instead of accum_add_kernel).  Destroying the accumulator
 * first detaches the monitor: its calls then return RT_ERR_STATE, and the destroy call still frees it.
 * 12 bytes of device memory per accumulator value. */
int rt_noise_create(rt_accum* acc, rt_noise** out);
/* Measures the frame buffers so far: the report, and per tile the maximum noise and the number of
 * pixels with noise > threshold (host arrays of tiles_x x tiles_y, either may be NULL; rep may be
 * NULL).  No float is ever summed, so every output is independent of reduction order. */
int rt_noise_measure(rt_noise* nm, float threshold, rt_noise_report* rep, float* tile_max, int32_t* tile_above);
/* The per-pixel noise, [owned_rows][width] floats, device or host pointer. */
int rt_noise_map(rt_noise* nm, float* out);
/* Side file of a checkpoint (little-endian): the accumulator blob's 96-byte header with magic
 * "RTNOISE1", version 1 and fb_count = frame buffers measured; then n_values u64 S2, then n_values
 * u32 S1.  Save follows the size-query convention of the accumulator's.  Load attaches a monitor in
 * the saved state: RT_ERR_STATE unless every header field equals the accumulator's rt_accum_info
 * (fb_first, fb_count and the scene fingerprint included) and the accumulator has no monitor;
 * RT_ERR_ARG for a malformed blob. */
int rt_noise_save(rt_noise* nm, void* blob, size_t cap, size_t* need);
int rt_noise_load(rt_accum* acc, const void* blob, size_t n, rt_noise** out);
/* Device time in ms of the last measure or map kernel (the reduction to the image totals included);
 * 0 before one. */
float rt_noise_last_measure_ms(const rt_noise* nm);
int rt_noise_destroy(rt_noise* nm);
/* Host only (no context, no GPU; csrc/rt_noise_blob.cpp): validate a side file and fill info
 * (RT_ERR_ARG for truncation, another magic or version, a size that does not match n_values and the
 * tiling, a checksum mismatch, fb_count > 32768); build one from an info and its moments; measure
 * one as the device does (every output may be NULL; map is [owned_rows][width]). */
int rt_noise_blob_info(const void* blob, size_t n, rt_accum_info* info);
int rt_noise_blob_pack(const rt_accum_info* info, const uint32_t* s1, const uint64_t* s2, void* blob, size_t cap, size_t* need);
int rt_noise_blob_measure(const void* blob, size_t n, float threshold, rt_noise_report* rep,
                          float* tile_max, int32_t* tile_above, float* map);

/* ------------------------------------------------------------------ launches over a set of tiles */
/* rt_render for the pixels of the listed tiles only.  Tiles are the noise monitor's: 16 x 16 pixels over
 * (owned-row index, column), row-major, id = ty * tiles_x + tx with tiles_x = ceil(width / 16) and
 * tiles_y = ceil(owned_rows / 16); edge tiles are partial; for a band tiling the row index is the
 * position in rt_owned_rows' list.  (They are not the 8 x 8 camera-ray tiles the kernels use inside.)
 *
 * fb has rt_render's layout for args, [fb_count][owned_rows][width][3], device or host pointer.  Every
 * pixel of a listed tile receives, for every fb id of the call, exactly the floats rt_render writes there
 * (a pixel's value depends on (fb id, pixel) alone); every other float of fb is left as it was (a host fb
 * is copied to the device and back whole).  counters (may be NULL) receives the totals of the rendered
 * items only.  tiles is a host array of n_tiles distinct ids.  RT_ERR_ARG, with fb untouched, for
 * n_tiles <= 0, an id out of range, a repeated id, or fb_count x owned_rows x width > 2^31.
 *
 * The launch runs the kernel variant rt_render would pick for the scene and flags, over an item list
 * built on the device.  It is isolated from the context's item schedule: no probe launch, no split
 * samples, natural row order, nothing read from or recorded into the schedule of any configuration, so
 * the rt_render launches around it run exactly as they would without it.  RT_FLAG_NO_SCHEDULE,
 * RT_FLAG_NO_SPLIT and RT_FLAG_FRESH are accepted and have no effect; the other flags, stats, both
 * camera modes and rt_ctx_options behave as in rt_render.  Afterwards rt_last_render_schedule is 0, and
 * rt_last_render_kernel, rt_last_render_ms and rt_last_kernel_ms describe the tile launch. */
int rt_render_tiles(rt_ctx* ctx, const rt_render_args* args, const int32_t* tiles, int32_t n_tiles, float* fb,
                    rt_counters* counters);

/* ------------------------------------------------------------------ adaptive accumulator */
/* A progressive draw that stops rendering a tile (as above) once the tile's own noise estimate is low
 * enough, and goes on with the others.  An object of its own beside rt_accum (no rt_multi support; its
 * checkpoint, reopening and dilation are the rt_adaptive_* functions below).  Per accumulator value it keeps the float sum of rt_accum (the same operations in
 * the same order) and the integer moments S1, S2 of rt_noise: 16 bytes per value; per tile n_t, the
 * number of frame buffers folded into it; and, from the first add, a scratch of chunk_fbs frame buffers
 * with the item list of its launches.
 *
 * The guarantee: every pixel of tile t of the image is byte-identical to rt_draw with no_fb = n_t and
 * the same fb_first (a pixel of frame buffer id depends on (id, pixel) alone, and the image after k frame
 * buffers is quant(sum / k) with the sum taken in fb order).  The n_t are an output (rt_adapt_counts).
 * They are determined by the sequence of add and retire calls alone -- retire decides on integer
 * moments -- and depend neither on chunk_fbs nor on how the adds between two retires were split.
 *
 * What it does not give: stopping a tile on the spread of its own samples biases it slightly, towards
 * stopping while it happens to look smooth (a rare bright path that has not occurred yet cannot show in
 * the spread).  The guards are the caller's: do not retire before enough frame buffers (min_fbs of the
 * Python driver), and keep the neighbours of a noisy tile active (dilate of rt_adaptive_retire).  The
 * reference has no adaptive mode to compare with. */
typedef struct rt_adapt rt_adapt;
typedef struct rt_adapt_report {
  int32_t fbs;            /* frame buffers rendered for the tiles still active (= max n_t)       */
  int32_t tiles_x, tiles_y, tiles_active;
  int64_t pixels, pixels_active;
  int64_t pixel_fbs;      /* sum over pixels of n_t: the work done; pixels x fbs without retiring */
  int64_t pixels_above;   /* pixels with noise > threshold, each at its own tile's n_t           */
  float threshold, max_noise;
} rt_adapt_report;

/* args as for rt_accum_create (fb_count ignored; band tilings accepted).  chunk_fbs >= 1: frame buffers
 * per launch, chunk_fbs x owned_rows x width <= 2^31.  Every tile starts active with n_t = 0. */
int rt_adapt_create(rt_ctx* ctx, const rt_render_args* args, int32_t chunk_fbs, rt_adapt** out);
/* Renders the next `count` fb ids for the active tiles only (rt_render_tiles' launch, at most chunk_fbs
 * per launch) and folds them in; the fold's traffic is the active tiles'.  counters (may be NULL)
 * receives this call's totals.  With no active tile it renders nothing, zeroes counters and returns
 * RT_OK.  RT_ERR_ARG, before anything is rendered, when fbs + count would exceed rt_noise's 32 768;
 * RT_ERR_STATE after another rt_scene_upload.  Otherwise rt_adaptive_add with limit = 32 768. */
int rt_adapt_add(rt_adapt* ad, int32_t count, rt_counters* counters);
/* Needs fbs >= 2 (RT_ERR_STATE otherwise).  For every active tile: the per-pixel noise by rt_noise's
 * definition with n = n_t (the same device code), and the tile retires when at most max_above (>= 0) of
 * its pixels have noise > threshold.  A retired tile is not rendered again and its n_t stays, unless
 * rt_adaptive_reopen makes it active again.  rt_adaptive_retire with dilate = 0.  rep (may be NULL) describes the state after retiring; max_noise and pixels_above cover all
 * tiles, retired ones at their frozen n_t.  Only maxima and integer counts are reduced. */
int rt_adapt_retire(rt_adapt* ad, float threshold, int32_t max_above, rt_adapt_report* rep);
/* rt_accum_image's conventions; quant(sum / n_t) per pixel.  RT_ERR_STATE before the first frame buffer. */
int rt_adapt_image(rt_adapt* ad, uint8_t* out, int32_t png_order);
/* n_t of every tile: host array of tiles_x x tiles_y. */
int rt_adapt_counts(rt_adapt* ad, int32_t* tile_fbs);
/* The per-pixel noise, each pixel at its tile's n_t: [owned_rows][width] floats, device or host pointer.
 * Needs fbs >= 2. */
int rt_adapt_noise_map(rt_adapt* ad, float* out);
/* The report rt_adapt_retire would give, retiring nothing.  Needs fbs >= 2. */
int rt_adapt_get_report(rt_adapt* ad, float threshold, rt_adapt_report* rep);
/* Device time in ms of the last fold kernel (the last chunk of rt_adapt_add) and of the last
 * rt_adapt_retire's measure kernel; 0 before one. */
float rt_adapt_last_add_ms(const rt_adapt* ad);
float rt_adapt_last_retire_ms(const rt_adapt* ad);
int rt_adapt_destroy(rt_adapt* ad);

/* ---- checkpoint and resume, reopening retired tiles, dilation: further calls on an rt_adapt (their prefix
 * differs only because the rt_adapt_ family is closed).  None of them weakens the guarantee above: tile t
 * of the image stays byte-identical to rt_draw with no_fb = n_t, and the n_t stay an output.
 *
 * dilate = r >= 0 (negative: RT_ERR_ARG) is a Chebyshev radius in tiles over the tile grid, that is over
 * (owned-row index, column): tile (ty, tx) is within r of (uy, ux) when max(|ty - uy|, |tx - ux|) <= r.
 * For a band tiling the neighbours are therefore neighbours in the list of owned rows, not in the image:
 * two tile rows that are adjacent in the grid may lie band_stride bands apart.  dilate_r(F) is the set of
 * tiles within r of a tile of F; dilate_0(F) = F.
 *
 * rt_adaptive_retire: rt_adapt_retire with dilation.  With F = the active tiles that have more than
 * max_above pixels of noise > threshold, the active set becomes its intersection with dilate_r(F): a passing tile within
 * r of a failing active tile stays active (it is the neighbour most likely to look smooth by chance).  When
 * no active tile fails every tile retires, so a draw still ends.
 *
 * rt_adaptive_reopen: needs fbs >= 2 (RT_ERR_STATE otherwise).  Every tile, active or retired, is measured
 * at its own n_t; with F = all the tiles that fail, the active set becomes its union with dilate_r(F).  It never
 * retires a tile.  A reopened tile keeps its n_t, its sums and its moments and continues from frame buffer
 * fb_first + n_t, exactly where it stopped.  rep follows rt_adapt_retire's conventions (fbs = max n_t).
 *
 * rt_adaptive_add: after a reopen the active tiles carry different n_t.  Every active tile receives
 * min(count, limit - n_t) further frame buffers, its next ones; a tile already at the limit receives none and
 * stays active.  count < 1 or limit < 1 is RT_ERR_ARG, and so is, before anything is rendered, a tile that
 * would pass 32 768 frame buffers.  The tiles that receive something are grouped by n_t, the groups taken in
 * ascending n_t; each group is one rt_adapt_add of old over that group alone: the tile launch (at most
 * chunk_fbs frame buffers each) from fb_first + n_t, then the fold over the group's list.  While nothing
 * has been reopened there is one group and the launches are rt_adapt_add's.  counters (may be NULL) receives
 * the call's totals, zero when no tile receives anything.  fbs stays max n_t.
 *
 * rt_adaptive_active: flags[tiles_x x tiles_y], 1 = active.
 *
 * Checkpoint blob (little-endian): the accumulator blob's 96-byte header with magic "RTADAPT1", version 1
 * and fb_count = max n_t; then i32 n_t[tiles]; u8 active[tiles]; zero bytes up to an 8-byte offset;
 * n_values float sums; zero bytes up to an 8-byte offset; n_values u64 S2; n_values u32 S1.  The header's
 * payload hash is FNV-1a over everything after the header.  A valid blob: a header rt_accum_blob_info would
 * accept, n_values and the size matching the tiling's tile grid, 0 <= n_t <= fb_count <= 32768 with some
 * tile at fb_count, flags 0 or 1, every retired tile with n_t >= 2 (so fb_count = 0 means every tile active
 * at 0), zero padding, a matching hash.  Save follows the size-query convention of rt_accum_save.  Load:
 * RT_ERR_ARG for anything but a valid blob, with nothing allocated; RT_ERR_STATE when the context's scene
 * differs from the blob's; chunk_fbs need not be the saved draw's.  A loaded accumulator continues
 * byte-identically to one that never stopped: image, counts, noise map and every integer of the reports. */
int rt_adaptive_add(rt_adapt* ad, int32_t count, int32_t limit, rt_counters* counters);
int rt_adaptive_retire(rt_adapt* ad, float threshold, int32_t max_above, int32_t dilate, rt_adapt_report* rep);
int rt_adaptive_reopen(rt_adapt* ad, float threshold, int32_t max_above, int32_t dilate, rt_adapt_report* rep);
int rt_adaptive_active(rt_adapt* ad, uint8_t* flags);
int rt_adaptive_save(rt_adapt* ad, void* blob, size_t cap, size_t* need);
int rt_adaptive_load(rt_ctx* ctx, const void* blob, size_t n, int32_t chunk_fbs, rt_adapt** out);
/* Host only (no context, no GPU; csrc/rt_adapt_blob.cpp): validate a checkpoint and fill info (RT_ERR_ARG
 * for every violation listed above); its n_t and active flags (either may be NULL); its 8-bit image
 * quant(sum / n_t) in rt_resolve's layout (RT_ERR_STATE with fb_count = 0); the measure as the device does
 * it, each pixel at its tile's n_t (every output may be NULL, map is [owned_rows][width]; RT_ERR_STATE
 * unless every n_t >= 2); build a blob from an info (fb_count = max n_t) and its arrays. */
int rt_adaptive_blob_info(const void* blob, size_t n, rt_accum_info* info);
int rt_adaptive_blob_tiles(const void* blob, size_t n, int32_t* tile_fbs, uint8_t* active);
int rt_adaptive_blob_image(const void* blob, size_t n, uint8_t* out);
int rt_adaptive_blob_measure(const void* blob, size_t n, float threshold, rt_adapt_report* rep, float* tile_max,
                             int32_t* tile_above, float* map);
int rt_adaptive_blob_pack(const rt_accum_info* info, const int32_t* tile_fbs, const uint8_t* active, const float* sums,
                          const uint32_t* s1, const uint64_t* s2, void* blob, size_t cap, size_t* need);

/* ------------------------------------------------------------------ denoiser */
/* A variance-cancelling non-local-means filter (Rousselle, Knaus, Zwicker 2012) over the moments a noise
 * monitor or an adaptive accumulator already holds: per value they give the mean of c^2 and the variance of
 * that mean, which is the input such a filter needs.  Each pixel carries its own n -- the monitor's count, or
 * n_t of its noise tile for an adaptive accumulator -- so tiles that retired early at a higher noise are
 * smoothed more.  The calls below change no state: sums, moments, counts and checkpoints stay byte-identical,
 * and an accumulator that is never denoised launches exactly the kernels it launched before.  (Their names
 * begin with rt_denoise_ because the rt_noise_, rt_adapt_ and rt_adaptive_ families are closed.)
 *
 * The definition is exact: every reduction across pixels is over integers, hence independent of its order,
 * and every float operation is a single correctly rounded IEEE operation.  No float is summed across pixels
 * anywhere.  The device kernels and the host-only twin on a checkpoint agree byte for byte.
 *
 * The image is rows x width pixels of 3 values, whole-image tiling only (a band tiling is RT_ERR_ARG:
 * neighbouring owned-row indices are not neighbouring rows).  Pixel p has n = n(p) >= 2 frame buffers
 * (RT_ERR_STATE otherwise).  Parameters: search_radius R in 0..10, patch_radius f in 0..3, k > 0,
 * alpha >= 0, eps > 0; anything else (a NaN included) is RT_ERR_ARG.
 *
 * Per value j of pixel p, from S1 and S2 as rt_noise defines them:
 *
 *   Q = (256 S1 + n / 2) / n                 u64 integer division; Q < 2^24: the mean of c^2, 8 fractional bits
 *   M = (float)Q / 256.0f                    exact
 *   D = n S2 - S1^2                          u64
 *   V = (float)((double)D / ((double)n * (double)n * (double)(n - 1)))    divisor multiplied left to right;
 *                                            the variance of the mean, in c^2 units
 *
 * Distance term of a pair of pixels (a, b) and a channel j, in float, one rounded operation per operator, in
 * this order:
 *
 *   d   = M_a - M_b
 *   num = d * d - alpha * (V_a + fminf(V_a, V_b))
 *   den = eps + (k * k) * (V_a + V_b)
 *   t   = num / den, clamped to [-64, 64]   (a NaN, possible only with k * k = inf, counts as -64)
 *   T   = (int32)(t * 256.0f)                truncating cast
 *
 * For pixel p and search offset o with |o_x|, |o_y| <= R and q = p + o inside the image:
 *
 *   P   = sum of T(p + u, q + u, j) over the channels j and the patch offsets u, |u_x|, |u_y| <= f, for which
 *         both p + u and q + u are inside the image; an int32 sum, |P| <= 147 x 16384, in any order
 *   cnt = 3 x (number of such u) >= 3
 *
 *   x  = (float)P / (float)(256 cnt);   if (x < 0) x = 0
 *   s  = 1.0f - x * 0.125f;             if (s < 0) s = 0
 *   s2 = s * s;  s4 = s2 * s2;  s8 = s4 * s4
 *   W  = (uint32)(s8 * 65536.0f)        (1 - x / 8)^8 stands for e^-x: no transcendental, no libm difference
 *
 * The centre offset has P <= 0 and therefore W = 65536, always.  Output per value:
 *
 *   Num = sum over o of W Q_q           u64, < 2^49
 *   Den = sum over o of W               u64, >= 65536
 *   lin = (float)((double)Num / ((double)Den * 256.0 * 65025.0))          multiplied left to right
 *   image byte = quant(lin)             write_frame_buffer's quantisation, as every image here
 *   gain[p] = (float)((double)Den / 65536.0)    how many pixels' worth p was averaged over; 1 where nothing
 *                                               matched
 *
 * The arithmetic of a term and of a weight is stated once, in csrc/rt_denoise_math.h, for both halves. */
typedef struct rt_denoise_params {
  int32_t search_radius, patch_radius;
  float k, alpha, eps;
  int32_t pad;
} rt_denoise_params;
/* The shipped defaults (DESIGN.md 3.7 has the measurements behind them). */
void rt_denoise_params_default(rt_denoise_params* p);
/* The denoised image of a monitor's accumulator / of an adaptive accumulator.  out and gain (may be NULL;
 * [rows][width] floats) follow rt_accum_image's conventions: png_order = 0 is rt_resolve's layout, device or
 * host pointers; png_order = 1 is rt_draw's, top row first, host pointers.  params = NULL takes the defaults.
 * Every check comes before anything is written: on an error out and gain are untouched.  Temporary device
 * memory of 24 bytes per pixel is freed before the call returns. */
int rt_denoise_monitor(rt_noise* nm, const rt_denoise_params* params, uint8_t* out, float* gain, int32_t png_order);
int rt_denoise_adaptive(rt_adapt* ad, const rt_denoise_params* params, uint8_t* out, float* gain, int32_t png_order);
/* Device time in ms of the last denoise (the prepare pass and the filter kernel); 0 before one. */
float rt_denoise_monitor_last_ms(const rt_noise* nm);
float rt_denoise_adaptive_last_ms(const rt_adapt* ad);
/* Host only (no context, no GPU; csrc/rt_denoise_blob.cpp): the same filter on a monitor's side file
 * (rt_noise_save) or an adaptive checkpoint (rt_adaptive_save); out in rt_resolve's layout, n_values bytes,
 * gain [rows][width] or NULL, params = NULL for the defaults.  RT_ERR_ARG for a malformed blob, a band tiling,
 * bad parameters or a null out; RT_ERR_STATE for a pixel with n < 2. */
int rt_denoise_monitor_blob(const void* blob, size_t n, const rt_denoise_params* params, uint8_t* out, float* gain);
int rt_denoise_adaptive_blob(const void* blob, size_t n, const rt_denoise_params* params, uint8_t* out, float* gain);

/* ------------------------------------------------------------------ ray casts and feature buffers */
/* A guide answers world->hit(r, 0.001, inf) for rays of the caller's: the hit point, the normal the shading
 * sees (set_face_normal applied), the material, the material's texture value there and the primitive.  No random
 * number is drawn, nothing of a context is touched, and the render kernels are not involved: a guide holds its
 * own validated copy of the scene.  It serves picking, depth and normal images, looking into a scene, and the
 * feature buffers of the guided denoise below.  (The names begin with rt_guide_ because the denoiser's family is
 * closed.)
 *
 * The answer is the reference's, operation for operation (csrc/rt_first_hit.h, compiled by the device kernels
 * and by the host-only calls alike, which therefore agree bit for bit): the top-level list in order, lists,
 * transforms, boxes, the BVH visit of RT_FLAG_EXACT_TRAVERSAL.  albedo is the material's texture at (u, v, p):
 * a diffuse_light's emit texture, (1, 1, 1) for a dielectric.  An RT_OBJ_MEDIUM is seen as its boundary: the
 * boundary's nearest hit with t > 0.001, with the phase material as `material` and that material's texture as
 * albedo.  A BVH of more than 30 inner levels is RT_ERR_SCENE. */
typedef struct rt_guide_hit {
  float t;            /* 0 for a miss */
  float p[3];
  float n[3];         /* as the shading sees it: against the ray; not normalised for a flat triangle; 0 for a miss */
  float albedo[3];    /* the scene's background for a miss */
  float u, v;
  int32_t prim;       /* index into rt_scene_soa.prims (a box is one primitive); -1 for a miss */
  int32_t material;   /* -1 for a miss */
  int32_t front;      /* hit_record::front_face */
  int32_t pad;
} rt_guide_hit;       /* 64 bytes */
typedef struct rt_guide rt_guide;
enum rt_guide_plane { RT_GUIDE_NORMAL = 0, RT_GUIDE_ALBEDO = 1 };

/* rt_scene_validate, then a copy of the scene in the memory of hip_device, with rtacc's scene fingerprint (the
 * one rt_accum_info carries). */
int rt_guide_create(const rt_scene_soa* scene, int hip_device, rt_guide** out);
int rt_guide_destroy(rt_guide* g);
/* n rays of 8 floats each -- o[3], d[3], time, unused: the layout the oracle captures -- into n hits.  rays and
 * out are each a device or a host pointer (host buffers are staged through temporary device memory).  n = 0 is
 * RT_OK. */
int rt_guide_cast(rt_guide* g, const float* rays, long long n, rt_guide_hit* out);
/* The centre ray of every pixel of a width x height image into the guide's planes (28 bytes per pixel, kept
 * until the next rt_guide_render or the destroy): camera.h get_ray at s = (i + 0.5f) / width,
 * t = (j + 0.5f) / height, j = 0 the bottom row, with a lens offset of 0 and time = time0 + 0.5f (time1 - time0). */
int rt_guide_render(rt_guide* g, int32_t width, int32_t height);
/* The planes of the last rt_guide_render (RT_ERR_STATE before one): normal and albedo [height][width][3]
 * floats, depth [height][width] floats (t; 0 for a miss), prim [height][width].  Any pointer may be NULL; each
 * is a device or a host pointer.  png_order = 0: row 0 is the bottom row, as a frame buffer; 1: top row first,
 * host pointers only. */
int rt_guide_planes(rt_guide* g, float* normal, float* albedo, float* depth, int32_t* prim, int32_t png_order);
/* An 8-bit picture of a plane, [height][width][3], out a device or a host pointer: RT_GUIDE_NORMAL is
 * quant((n + 1.0f) / 2.0f) per component (a flat triangle's unnormalised normal saturates), RT_GUIDE_ALBEDO is
 * quant(albedo), with write_frame_buffer's quantisation. */
int rt_guide_image(rt_guide* g, int32_t which, uint8_t* out, int32_t png_order);
/* Device time in ms of the last cast or render kernel; 0 before one. */
float rt_guide_last_ms(const rt_guide* g);
/* Host only (no GPU; csrc/rt_guide_host.cpp): the same answers from the same code.  Host pointers; the planes
 * may each be NULL, row 0 the bottom row. */
int rt_guide_cast_host(const rt_scene_soa* scene, const float* rays, long long n, rt_guide_hit* out);
int rt_guide_render_host(const rt_scene_soa* scene, int32_t width, int32_t height, float* normal, float* albedo, float* depth,
                         int32_t* prim);

/* The guided denoise: the denoiser above with the feature planes of a guide as a second opinion on every
 * weight (Rousselle, Manzi, Zwicker 2013: the minimum of the colour weight and the feature weight).  For pixel
 * p, a search offset o other than the centre and q = p + o, on the centre pixels alone (no patch sum), with N
 * the normal plane, A the albedo plane and z the depth plane; a pixel is a miss when its z equals 0.  In float,
 * one rounded operation per operator, left to right:
 *
 *   fn = sum over c of (N_p,c - N_q,c)^2          ((d0 d0 + d1 d1) + d2 d2)
 *   fa = sum over c of (A_p,c - A_q,c)^2
 *   r  = (z_p - z_q) / (z_p + z_q);  fz = r r
 *   xf = fn normal_gain + fa albedo_gain + fz depth_gain
 *   exactly one of p, q a miss: xf = 64;  both: xf = 0;  a NaN xf counts as 64
 *
 * and the weight's x becomes fmaxf(x, xf) after its clamp at 0, before s = 1 - x / 8.  Everything else is the
 * denoiser's definition: P, Num and Den stay integer sums, the centre offset keeps W = 65536 whatever the
 * planes hold.  With every gain 0 and no pixel a miss (or every pixel) the result is rt_denoise_monitor's, byte
 * for byte.  Gains are >= 0 (anything else, a NaN included, is RT_ERR_ARG). */
typedef struct rt_guide_params {
  float normal_gain, albedo_gain, depth_gain;
  int32_t pad;
} rt_guide_params;
void rt_guide_params_default(rt_guide_params* p);
/* rt_denoise_monitor / rt_denoise_adaptive with the planes of g.  RT_ERR_STATE unless g has rendered planes of
 * the accumulator's width x height, its scene fingerprint is the accumulator's, and it lives on the
 * accumulator's device; otherwise every check, output and error of the unguided call (on an error out and gain
 * are untouched).  params or gparams = NULL takes the defaults.  The guide is read only. */
int rt_guide_denoise_monitor(rt_noise* nm, rt_guide* g, const rt_denoise_params* params, const rt_guide_params* gparams,
                             uint8_t* out, float* gain, int32_t png_order);
int rt_guide_denoise_adaptive(rt_adapt* ad, rt_guide* g, const rt_denoise_params* params, const rt_guide_params* gparams,
                              uint8_t* out, float* gain, int32_t png_order);
/* Host only: rt_denoise_monitor_blob / rt_denoise_adaptive_blob with host planes (rt_guide_planes' layout with
 * png_order = 0) of plane_height x plane_width pixels; RT_ERR_ARG when that is not the blob's image size, for a
 * null plane or a bad gain, besides the unguided calls' errors. */
int rt_guide_denoise_monitor_blob(const void* blob, size_t n, const rt_denoise_params* params, const rt_guide_params* gparams,
                                  const float* normal, const float* albedo, const float* depth, int32_t plane_width,
                                  int32_t plane_height, uint8_t* out, float* gain);
int rt_guide_denoise_adaptive_blob(const void* blob, size_t n, const rt_denoise_params* params, const rt_guide_params* gparams,
                                   const float* normal, const float* albedo, const float* depth, int32_t plane_width,
                                   int32_t plane_height, uint8_t* out, float* gain);

/* ------------------------------------------------------------------ averaged feature planes */
/* A guide's planes from several rays per pixel, spread over the pixel's footprint, the lens and the shutter, and
 * averaged: normal, albedo and depth images that line up with a picture that has antialiased silhouettes, a depth
 * of field and motion blur, where the centre ray's are sharp.  The rays are the guide's own (no render kernel is
 * involved), the averages go into the guide's planes, so the planes, image and guided-denoise calls above work on
 * them unchanged.  (A family of its own because the guide's is closed.)
 *
 * Everything is in float, one correctly rounded operation per operator, left to right, unless it says double.
 *
 * The pattern.  Sample s of S = samples is the same for every pixel (the planes are smooth, not noisy).  With P
 * the smallest power of two >= S and rev2 the reversal of s in log2 P bits:
 *
 *   du = (float)(2 s + 1) / (float)(2 S)
 *   dv = (float)(2 rev2 + 1) / (float)(2 P)                  footprint = 0: du = dv = 0.5f
 *
 * Lens points are the first S accepted candidates k = 1, 2, ... of a rejection walk in double, kept in order:
 *
 *   x = 2.0 (rev3 / 59049.0) - 1.0                           rev3: k's 10 base-3 digits reversed
 *   y = 2.0 (rev5 / 78125.0) - 1.0                           rev5: k's 7 base-5 digits reversed
 *   accepted when x x + y y <= 1.0;  lx = (float)x, ly = (float)y         lens = 0: lx = ly = 0
 *
 *   f = (float)(rev7 / 16807.0)   in double, rev7: s's 5 base-7 digits reversed       shutter = 0: f = 0.5f
 *
 * The ray of pixel (i, j), j = 0 the bottom row, of a W x H image for sample s (render.h:105-106 with the pattern
 * in place of the random numbers, then camera.h:49-57 in the reference's order):
 *
 *   su = ((float)i + du) / (float)W;   sv = ((float)j + dv) / (float)H
 *   rd = (lens_radius lx, lens_radius ly);   offset = rd.x u + rd.y v
 *   origin    = origin + offset
 *   direction = lower_left + su horizontal + sv vertical - origin - offset
 *   time      = time0 + f (time1 - time0)
 *
 * With lens = 0 no offset is formed, added or subtracted: the ray is the centre pass's own expression at
 * (su, sv) from the camera's origin.
 *
 * The average.  Every ray is cast as the guide casts any ray (a miss gives t = 0, n = 0, albedo = background).
 * The sums start as sample 0's values, not as zero plus them (the sign of a zero survives), and take samples
 * 1 .. S - 1 in order:
 *
 *   normal   = sum of n / (float)S          over all samples, as cast returns them (not renormalised)
 *   albedo   = sum of albedo / (float)S     over all samples
 *   depth    = sum of t over the hits / (float)hits,  0 with no hit
 *   coverage = (float)hits / (float)S
 *   prim     = the primitive of the hit of lowest s,  -1 with no hit
 *
 * samples = 1 with lens = 0 and shutter = 0 is therefore the centre pass, bit for bit (du = dv = 0.5f whatever
 * footprint says).  The pattern and the per-pixel loop are stated once, in csrc/rt_aov.h, for both halves. */
typedef struct rt_aov_params {
  int32_t samples;    /* 1..256 */
  int32_t lens;       /* 0 or 1: sample the lens (a camera with lens_radius 0 is unaffected) */
  int32_t footprint;  /* 0 or 1: sample the pixel's area */
  int32_t shutter;    /* 0 or 1: sample the shutter interval */
} rt_aov_params;      /* 16 bytes */
/* 16 samples, every switch 1. */
void rt_aov_params_default(rt_aov_params* p);
/* Host only: the table of p, out[samples][5] = du, dv, lx, ly, f.  RT_ERR_ARG for a null out, samples outside
 * 1..256 or a switch that is neither 0 nor 1 (so everywhere below); p = NULL takes the defaults. */
int rt_aov_pattern(const rt_aov_params* p, float* out);
/* The averaged planes of a width x height image in place of the guide's planes (the centre pass's limits on width
 * and height), with a coverage plane [height][width] beside them; kept until the next render of either kind. */
int rt_aov_render(rt_guide* g, int32_t width, int32_t height, const rt_aov_params* p);
/* The coverage plane, with the pointer and png_order conventions of the planes call (out may be NULL).
 * RT_ERR_STATE unless the guide's current planes came from the averaged pass: a later centre pass drops it. */
int rt_aov_coverage(rt_guide* g, float* out, int32_t png_order);
/* Host only (no GPU; csrc/rt_guide_host.cpp): the same planes from the same code.  Host pointers, each may be
 * NULL, row 0 the bottom row. */
int rt_aov_render_host(const rt_scene_soa* scene, int32_t width, int32_t height, const rt_aov_params* p,
                       float* normal, float* albedo, float* depth, int32_t* prim, float* coverage);
/* Device time in ms of the last averaged pass's kernel; 0 before one. */
float rt_aov_last_ms(const rt_guide* g);

/* ------------------------------------------------------------------ casts and planes through specular surfaces */
/* The casts and planes above describe the first surface a ray meets.  On a mirror or a glass ball that surface
 * says nothing about the picture, which is of whatever the mirror shows.  A chain follows a ray through such
 * surfaces without a random number: a metal of little fuzz reflects, a dielectric refracts unless it cannot, and
 * the answer is the first surface that is neither, with the tint gathered on the way and the length travelled.
 * It serves "what do I see along this ray, through the mirror" and feature planes that have edges where the
 * reflected or refracted picture has them.  (A family of its own because the guide's and the averaged planes' are
 * closed.)  Nothing above changes what it returns.
 *
 * Everything is in float, one correctly rounded operation per operator, left to right, unless it says double;
 * a segment is one cast of the guide, of which only p, n, front, material, albedo, t and prim are read.  dot is
 * (x x + y y) + z z, v / s is (1.0f / s) v as in vec3.h.  The chain of a ray e0 = (o, d, time):
 *
 *   1. h = cast(e0), thr = (1, 1, 1), k = 0.
 *   2. h.prim < 0: the chain ends, RT_SPEC_MISS when k = 0, otherwise RT_SPEC_ESCAPED.
 *   3. m = materials[h.material] is specular when it is an RT_MAT_METAL with m.param <= max_fuzz, or an
 *      RT_MAT_DIELECTRIC and glass is set.  Anything else ends the chain: RT_SPEC_SURFACE.  (A medium is its
 *      boundary with the phase material, as cast says, and therefore ends it.)
 *   4. k == max_bounces: RT_SPEC_LIMIT.
 *   5. ud = d / sqrtf(dot(d, d)).
 *   6. Metal (material.h:46-54 with the fuzz term at its mean, 0):  dir = ud - (2.0f dot(ud, n)) n;
 *      !(dot(dir, n) > 0): RT_SPEC_ABSORBED, the reference's scatter returning false;  otherwise
 *      thr = thr * h.albedo per component.
 *   7. Dielectric (material.h:67-90 without Schlick's random choice: the refraction whenever there is one):
 *        ratio = front ? 1.0f / ir : ir;   c = fminf(dot(-ud, n), 1.0f);   s = sqrtf(1.0f - c c)
 *        ratio s > 1.0f:  dir as the metal's
 *        otherwise (vec3.h:152-158):  perp = ratio (ud + c n)
 *                                     par  = -sqrtf(fabsf((float)(1.0 - (double)dot(perp, perp))))
 *                                     dir  = perp + par n
 *   8. The next ray is (h.p, dir, time): k = k + 1, h = cast of it, back to 2.
 *
 * Per ray the chain gives the last cast's rt_guide_hit unchanged (for RT_SPEC_ESCAPED the hit before the miss; its
 * albedo stays that surface's own texture value) and an rt_spec_path.  depth is in the primary ray's parameter
 * units, so that neighbouring pixels compare whatever the length of the camera's direction:
 *
 *   depth = t_0                                                            no continuation segment hit
 *   depth = t_0 + (sum of t_k sqrtf(dot(d_k, d_k)), k >= 1) / sqrtf(dot(d_0, d_0))
 *
 * over the continuation segments that hit; the sum starts as its first term and takes the others in order.  With
 * max_bounces = 0 the hit is cast's, byte for byte.  The chain is stated once, in csrc/rt_spec.h, for both halves. */
enum rt_spec_status { RT_SPEC_MISS = 0, RT_SPEC_SURFACE = 1, RT_SPEC_ESCAPED = 2, RT_SPEC_LIMIT = 3, RT_SPEC_ABSORBED = 4 };
typedef struct rt_spec_params {
  int32_t max_bounces;  /* 0..16 continuation segments */
  float max_fuzz;       /* 0..1: a metal of at most this fuzz is a mirror */
  int32_t glass;        /* 0 or 1: follow dielectrics */
  int32_t reserved;     /* 0 */
} rt_spec_params;       /* 16 bytes */
typedef struct rt_spec_path {
  int32_t bounces;         /* continuation segments cast */
  int32_t status;          /* rt_spec_status */
  int32_t first_prim;      /* the primary hit's prim and material; -1 for a miss */
  int32_t first_material;
  float throughput[3];     /* thr */
  float depth;             /* 0 for a miss */
} rt_spec_path;            /* 32 bytes */
/* max_bounces 4, max_fuzz 0.1, glass 1 (DESIGN.md 3.10 has the measurements behind max_fuzz). */
void rt_spec_params_default(rt_spec_params* p);
/* The chains of n rays in rt_guide_cast's layout.  rays, hits and paths are each a device or a host pointer; hits
 * or paths may be NULL.  p = NULL takes the defaults; RT_ERR_ARG for a field outside its range (so everywhere
 * below).  n = 0 is RT_OK. */
int rt_spec_cast(rt_guide* g, const float* rays, long long n, const rt_spec_params* p, rt_guide_hit* hits, rt_spec_path* paths);
/* The averaged pass with a chain per sample, into the guide's planes and coverage, so the planes, image, coverage
 * and guided-denoise calls work on them as they are.  aov = NULL means the centre ray: samples 1, lens 0,
 * footprint 0, shutter 0 (not the averaged pass's defaults); spec = NULL takes the defaults.  Per sample the normal
 * is the chain's hit's n (0 for RT_SPEC_MISS), the albedo is thr * albedo per component with the background in
 * place of the surface for RT_SPEC_MISS and RT_SPEC_ESCAPED, and the depth is the path's.  Whether a sample counts
 * as a hit, and so coverage, prim and which samples' depths are averaged, is decided by the primary ray: the
 * silhouette stays the first surface's.  Sums, order and divisions are the averaged pass's.  With max_bounces = 0
 * the five planes are rt_aov_render's byte for byte; with aov = NULL as well, rt_guide_render's. */
int rt_spec_render(rt_guide* g, int32_t width, int32_t height, const rt_aov_params* aov, const rt_spec_params* spec);
/* Host only (no GPU; csrc/rt_guide_host.cpp): the same answers from the same code.  Host pointers, each output
 * may be NULL, row 0 the bottom row. */
int rt_spec_cast_host(const rt_scene_soa* scene, const float* rays, long long n, const rt_spec_params* p, rt_guide_hit* hits,
                      rt_spec_path* paths);
int rt_spec_render_host(const rt_scene_soa* scene, int32_t width, int32_t height, const rt_aov_params* aov,
                        const rt_spec_params* spec, float* normal, float* albedo, float* depth, int32_t* prim, float* coverage);
/* Device time in ms of the last rt_spec_cast or rt_spec_render kernel; 0 before one. */
float rt_spec_last_ms(const rt_guide* g);

/* ------------------------------------------------------------------ host scene library */
/* Builds one of the reference scenes (scenes.h) on the host: "basic", "first", "big1" (alias
 * "random"), "two_spheres", "two_perlin", "cornell", "cornell_smoke", "triangle", "triangles",
 * "backpack" (renders only its ground, H17).  The returned handle owns the arrays its
 * rt_scene_soa points at. */
typedef struct rt_scene_host rt_scene_host;
int rt_scene_build(const char* name, rt_scene_host** out);
const rt_scene_soa* rt_scene_view(const rt_scene_host* s);
void rt_scene_free(rt_scene_host* s);

/* Decoded image, the stbi_load layout make_image() uploads (texture.h:166-203): rows top to
 * bottom, bytes_per_pixel interleaved channels. */
typedef struct rt_image_asset {
  int32_t width, height, bytes_per_pixel;
  int32_t pad;
  const uint8_t* data;
} rt_image_asset;
/* One mesh as create_meshes_d() builds it (triangle_mesh.h:147-204): 24 floats per triangle,
 * v0[3] v1[3] v2[3] n0[3] n1[3] n2[3] u0 v0 u1 v1 u2 v2.  vertex_normals = 0 uses the face
 * normal (triangle.h:166); image = index into the assets' images for its lambertian texture. */
typedef struct rt_mesh_asset {
  int32_t n_triangles;
  int32_t vertex_normals;
  int32_t image;
  int32_t pad;
  const float* data;
} rt_mesh_asset;
typedef struct rt_scene_assets {
  int32_t n_images;
  int32_t n_meshes;
  const rt_image_asset* images;
  const rt_mesh_asset* meshes;
} rt_scene_assets;
/* rt_scene_build with external assets (the files the reference reads at scene construction):
 * "earth" (images[0] = earthmap, scenes.h:278-320), "door" / "cup" (meshes[0] with its texture,
 * scenes.h:478-523,576-621), "final" (the composed book-2 final scene of config C5: images[0]
 * and meshes[0]), and every name rt_scene_build accepts (assets may be NULL). */
int rt_scene_build_ex(const char* name, const rt_scene_assets* assets, rt_scene_host** out);

/* OBJ mesh ingestion: create_meshes() (triangle_mesh.h:208-352) with assimp's OBJ import
 * (ReadFile(Triangulate | GenNormals), processNode order) restated, see csrc/rt_obj.cpp.
 * RT_OBJ_INDEX_REFERENCE reproduces create_meshes_d's indexing of the concatenated vertex array
 * with per-mesh local indices; RT_OBJ_INDEX_GLOBAL offsets each mesh's indices. */
enum { RT_OBJ_INDEX_REFERENCE = 0, RT_OBJ_INDEX_GLOBAL = 1 };
typedef struct rt_obj_mesh rt_obj_mesh;
typedef struct rt_obj_info {
  int32_t n_triangles;   /* rows of `triangles` (rt_mesh_asset layout, 24 floats each)         */
  int32_t n_meshes;      /* aiMeshes the import produced                                        */
  int32_t n_vertices;    /* concatenated vertex count                                            */
  int32_t n_textures;    /* distinct diffuse textures of the used materials (reference needs 1) */
  const float* triangles;
  const char* texture;   /* first diffuse texture path (OBJ directory + map_Kd), "" if none     */
} rt_obj_info;
int rt_obj_load(const char* path, int32_t index_mode, rt_obj_mesh** out);
/* Image decoding for textures: make_image()/imread() (texture.h:166-203) through the reference's
 * stb_image v2.26, restated for baseline JPEGs (csrc/rt_image.cpp): identical texel bytes.
 * Output = stbi_load(.., 0) layout (rows top to bottom, 1 or 3 channels). */
typedef struct rt_image_host rt_image_host;
int rt_image_decode(const uint8_t* bytes, int64_t n, rt_image_host** out);
int rt_image_load(const char* path, rt_image_host** out);
const rt_image_asset* rt_image_view(const rt_image_host* im);
void rt_image_free(rt_image_host* im);
const rt_obj_info* rt_obj_view(const rt_obj_mesh* m);
void rt_obj_free(rt_obj_mesh* m);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
