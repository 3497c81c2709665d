// rt_scene_prep.h -- internal: everything rt_scene_upload computes on the host before it copies a scene to
// the device (rt_scene_prep.cpp), and the constants that preparation shares with the kernels of
// rt_kernels.hip.  Host-only: no HIP header here or in the .cpp, so scripts/check_scene_prep.cpp links the
// unit into a stand-alone program.  Hidden visibility: the library exports nothing from this file.
#ifndef RT_SCENE_PREP_H
#define RT_SCENE_PREP_H

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_hip.h"

#define RT_PRIM_TYPE_MASK 0xff
#define RT_PRIM_FLAG_UV 0x100      // material needs sphere u,v (image texture)
#define RT_PRIM_FLAG_UNIT_T 0x200  // moving sphere with time0 = 0, time1 - time0 = 1
#define RT_PRIM_FLAG_XF 0x400      // world-tree leaf under a translate/rotate_y instance (F_WORLD)
#define RT_PRIM_FLAG_OUT 0x800     // BVH leaf whose box sticks out of a stored box of its reference chain
#define RT_WKEY_SHIFT 20           // world-tree tie key: (n_world - 1 - entry) << 20 | reference leaf rank

// Scene feature mask: the render kernel is instantiated per feature set so that a scene pays
// registers only for the primitive / object / texture kinds it contains.
enum : int {
  F_STATS = 1 << 0,
  F_MOVING = 1 << 1,
  F_RECT = 1 << 2,
  F_TRI = 1 << 3,
  F_LIST = 1 << 4,
  F_XFORM = 1 << 5,
  F_MEDIUM = 1 << 6,
  F_CHECKER = 1 << 7,
  F_NOISE = 1 << 8,
  F_IMAGE = 1 << 9,
  F_BVH = 1 << 10,
  F_EXACT = 1 << 11,  // reference BVH visit set (no culling): node/prim counts equal the oracle's
  F_CHECK = 1 << 12,  // culled search + exact re-run per query; disagreements logged (audit mode)
  F_LDS = 1 << 13,    // BVH nodes + primitives staged in LDS (1024-thread workgroups, 1 per CU)
  F_STEP = 1 << 14,   // world = one BVH object: render_step_kernel (one traversal step per loop trip)
  F_WORLD = 1 << 15,  // list world flattened into ONE traversal tree (render_step_kernel; build_world_tree)
  F_QLDS = 1 << 16,   // the world BVH's traversal tree quantized to 24-byte pair records in LDS (qpair)
  F_MERGE = 1 << 17,  // render_kernel answers world queries with world_search only (merge_ok scenes)
  F_PROBE = 1 << 18,  // the same code under its own symbol for the probe launches of a first launch
                      // (rt_render): rocprof then times the render launches apart from the probes
  F_ALL = (1 << 11) - 2,
  F_SPHERES = F_MOVING | F_CHECKER | F_BVH,           // basic, first, big1 (C2), two_spheres
  F_CORNELL = F_RECT | F_LIST | F_XFORM | F_MEDIUM,   // cornell, cornell_smoke (C3)
  F_MESH = F_TRI | F_IMAGE | F_BVH | F_LIST,            // triangle meshes with image textures (C4)
  F_FINAL = F_ALL & ~F_CHECKER,                         // final (C5): everything but the checker texture
};

#pragma GCC visibility push(hidden)
namespace rtprep {

// Per-lane traversal stack in LDS (after the staged scene for F_LDS variants), lane-interleaved
// (entry d of thread t at [d * block + t]) so a wave's pushes/pops hit 64 distinct banks.
constexpr int kStackDepth = 16;
// The stepwise LDS variant stages the world BVH's traversal tree in four planes of kPlanePairs float4
// each (stage_lds): a larger tree runs the stepwise kernel from global memory.
constexpr int kPlanePairs = 512;
constexpr int kLdsBudget = 156 * 1024;  // bytes of staged nodes + primitives + stacks per workgroup

// The device's float4 and float2 as the host lays them out (rt_scene_upload asserts the sizes).
struct Float4 {
  float x, y, z, w;
};
struct Float2 {
  float x, y;
};

// The upload-time fields of rt_ctx_options.
struct Options {
  int32_t dedup_triangles, world_tree, quantized_tree, merged_search, merge_order;
};

// Every array rt_scene_upload copies that is not the caller's own, and every scalar it stores in the
// device scene view or the context.
struct Prepared {
  std::vector<rt_object> objects;   // c = first node of a BVH's traversal tree, 1 for an inert medium, else -1
  std::vector<rt_prim> prims;       // flags and a triangle's index in the type word, its operands in p[0..8],
                                    // the reference leaf rank in p[9]
  std::vector<rt_bvh_node> nodes;   // the reference trees, then the traversal trees built here
  std::vector<Float2> pmargin;      // per primitive, padded to an even count (whole float4s for LDS staging)
  std::vector<Float4> pvalid;       // per primitive, 3 each
  std::vector<rt_image> images;     // pointing into the tiled texels
  std::vector<uint8_t> texels;      // 8x8-texel tiles, at least 3 bytes per texel
  std::vector<Float4> wleaf, wxf;   // world tree: 4 per leaf, 2 per instance
  std::vector<int32_t> worder;      // world_search's visiting order
  std::vector<uint32_t> qnodes;     // quantized tree: 6 words per pair, empty unless q_pairs > 0
  std::vector<Float4> bin_sph;      // camera-bin bounding spheres
  std::vector<int32_t> bin_ids;     // ... and their primitives (world = one BVH)
  int wt_fb = -1, w_media = 0, w_inert = 0, merge_ok = 0;
  int q_pairs = 0, q_ebias = 0;
  int features = 0;
  bool world_bvh = false, world_step = false, world_tree = false;
  int bin_n = 0;  // > 0: primitive spheres (tile lists); < 0: entry spheres (masks)
  int plane_fb = -1, plane_pairs = 0;
};

// Prepares a scene that rt_scene_validate accepts.  RT_OK, or RT_ERR_SCENE with the reason in why.
int prepare(const rt_scene_soa* s, const Options& opt, Prepared& out, std::string& why);

}  // namespace rtprep
#pragma GCC visibility pop

#endif  // RT_SCENE_PREP_H
