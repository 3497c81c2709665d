// rt_adapt_blob.cpp — the host-only half of the adaptive accumulator's checkpoint (rt_adaptive_blob_* of
// include/rt_hip.h): a checkpoint packed, validated, finalised into the 8-bit image and measured without a
// context or a GPU.  Plain C++ with no HIP include; a stand-alone program links this file and
// rt_accum_blob.cpp.
//
// Blob (little-endian): the 96-byte header of rt_accum_blob.cpp with magic "RTADAPT1", version 1 and
// fb_count = max n_t, then (tiles = tiles_x x tiles_y noise tiles of 16 x 16 pixels over (owned-row index,
// column), rtacc::adapt_layout has the offsets)
//   i32[tiles]     n_t, the frame buffers folded into every tile
//   u8[tiles]      1 = active, 0 = retired
//   zero bytes up to an 8-byte offset
//   f32[n_values]  the sums, owned rows ascending
//   zero bytes up to an 8-byte offset
//   u64[n_values]  S2 = sum of c^4
//   u32[n_values]  S1 = sum of c^2
//
// The measure is adapt_measure_kernel's (rt_progressive.hip), tile for tile: the noise monitor's per-pixel
// formula (rtacc::host_pixel_noise) with n = n_t of the pixel's tile.
#include "rt_accum_blob.h"

#include <cstring>

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the payload is copied as little-endian values");

namespace {

const char kMagic[8] = {'R', 'T', 'A', 'D', 'A', 'P', 'T', '1'};
constexpr uint32_t kVersion = 1;
constexpr size_t kBytesPerValue = sizeof(float) + sizeof(uint64_t) + sizeof(uint32_t);

struct Grid {
  int64_t rows, width, tiles_x, tiles_y, tiles;
};

// The header's own limits, and the tile grid of its tiling; false when the blob's size would not fit size_t.
bool adapt_info_ok(const rt_accum_info* i, Grid* g) {
  if (!rtacc::info_ok(i) || i->args.fb_count > rtacc::kNoiseMaxFbs) return false;
  g->width = i->args.width;
  g->rows = i->n_values / (3 * g->width);
  g->tiles_x = (g->width + rtacc::kNoiseTile - 1) / rtacc::kNoiseTile;
  g->tiles_y = (g->rows + rtacc::kNoiseTile - 1) / rtacc::kNoiseTile;
  g->tiles = g->tiles_x * g->tiles_y;
  if (g->tiles > INT32_MAX) return false;
  return (uint64_t)i->n_values <= (SIZE_MAX - rtacc::kHeaderBytes - 5 * (size_t)g->tiles - 16) / kBytesPerValue;
}

// What the tiles of a checkpoint may hold (p_n, p_active: possibly unaligned): 0 <= n_t <= fb_count with
// some tile at fb_count, flags 0 or 1, a retired tile with n_t >= 2.  fb_count = 0 then leaves only
// "every tile active with n_t = 0".
bool tiles_ok(const unsigned char* p_n, const unsigned char* p_active, int64_t tiles, int32_t fb_count) {
  bool at_max = false;
  for (int64_t t = 0; t < tiles; ++t) {
    int32_t n;
    memcpy(&n, p_n + 4 * t, 4);
    if (n < 0 || n > fb_count || p_active[t] > 1) return false;
    if (!p_active[t] && n < 2) return false;
    at_max = at_max || n == fb_count;
  }
  return at_max;
}

// The validated blob's header, grid and layout.
int open_blob(const void* blob, size_t n, rt_accum_info* info, Grid* g, rtacc::AdaptLayout* l) {
  if (!blob || n < rtacc::kHeaderBytes) return RT_ERR_ARG;
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  rt_accum_info i = {};
  uint64_t hash = 0;
  if (!rtacc::get_header(p, kMagic, kVersion, &i, &hash)) return RT_ERR_ARG;
  if (!adapt_info_ok(&i, g)) return RT_ERR_ARG;
  *l = rtacc::adapt_layout((size_t)i.n_values, (size_t)g->tiles);
  if (n != l->total) return RT_ERR_ARG;
  if (!tiles_ok(p + l->n_t, p + l->active, g->tiles, i.args.fb_count)) return RT_ERR_ARG;
  for (size_t k = l->pad0; k < l->sums; ++k)
    if (p[k]) return RT_ERR_ARG;
  for (size_t k = l->pad1; k < l->s2; ++k)
    if (p[k]) return RT_ERR_ARG;
  if (rtacc::fnv1a(p + rtacc::kHeaderBytes, n - rtacc::kHeaderBytes) != hash) return RT_ERR_ARG;
  *info = i;
  return RT_OK;
}

int32_t tile_n(const unsigned char* p, const rtacc::AdaptLayout& l, int64_t t) {
  int32_t n;
  memcpy(&n, p + l.n_t + 4 * t, 4);
  return n;
}

}  // namespace

extern "C" {

int rt_adaptive_blob_pack(const rt_accum_info* info, const int32_t* tile_fbs, const uint8_t* active, const float* sums,
                          const uint32_t* s1, const uint64_t* s2, void* blob, size_t cap, size_t* need) {
  Grid g;
  if (!info || !adapt_info_ok(info, &g)) return RT_ERR_ARG;
  const size_t nv = (size_t)info->n_values, tiles = (size_t)g.tiles;
  const rtacc::AdaptLayout l = rtacc::adapt_layout(nv, tiles);
  if (need) *need = l.total;
  if (!blob && cap == 0) return RT_OK;  // size query
  if (!blob || !tile_fbs || !active || !sums || !s1 || !s2 || cap < l.total) return RT_ERR_ARG;
  if (!tiles_ok(reinterpret_cast<const unsigned char*>(tile_fbs), active, g.tiles, info->args.fb_count)) return RT_ERR_ARG;
  unsigned char* p = static_cast<unsigned char*>(blob);
  // memmove: rt_adaptive_save has the arrays in the blob's payload already
  memmove(p + l.n_t, tile_fbs, 4 * tiles);
  memmove(p + l.active, active, tiles);
  memset(p + l.pad0, 0, l.sums - l.pad0);
  memmove(p + l.sums, sums, 4 * nv);
  memset(p + l.pad1, 0, l.s2 - l.pad1);
  memmove(p + l.s2, s2, 8 * nv);
  memmove(p + l.s1, s1, 4 * nv);
  rtacc::put_header(p, kMagic, kVersion, info, rtacc::fnv1a(p + rtacc::kHeaderBytes, l.total - rtacc::kHeaderBytes));
  return RT_OK;
}

int rt_adaptive_blob_info(const void* blob, size_t n, rt_accum_info* info) {
  Grid g;
  rtacc::AdaptLayout l;
  if (!info) return RT_ERR_ARG;
  return open_blob(blob, n, info, &g, &l);
}

int rt_adaptive_blob_tiles(const void* blob, size_t n, int32_t* tile_fbs, uint8_t* active) {
  rt_accum_info i;
  Grid g;
  rtacc::AdaptLayout l;
  const int rc = open_blob(blob, n, &i, &g, &l);
  if (rc) return rc;
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  if (tile_fbs) memcpy(tile_fbs, p + l.n_t, 4 * (size_t)g.tiles);
  if (active) memcpy(active, p + l.active, (size_t)g.tiles);
  return RT_OK;
}

int rt_adaptive_blob_image(const void* blob, size_t n, uint8_t* out) {
  rt_accum_info i;
  Grid g;
  rtacc::AdaptLayout l;
  const int rc = open_blob(blob, n, &i, &g, &l);
  if (rc) return rc;
  if (!out) return RT_ERR_ARG;
  if (i.args.fb_count < 1) return RT_ERR_STATE;
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  for (int64_t r = 0; r < g.rows; ++r)
    for (int64_t x = 0; x < g.width; ++x) {
      const float d = (float)tile_n(p, l, (r / rtacc::kNoiseTile) * g.tiles_x + x / rtacc::kNoiseTile);
      const int64_t k = 3 * (r * g.width + x);
      float s[3];
      memcpy(s, p + l.sums + 4 * k, sizeof(s));
      for (int j = 0; j < 3; ++j) out[k + j] = (uint8_t)rtacc::host_quant(s[j] / d);
    }
  return RT_OK;
}

int rt_adaptive_blob_measure(const void* blob, size_t n, float threshold, rt_adapt_report* rep, float* tile_max,
                             int32_t* tile_above, float* map) {
  rt_accum_info i;
  Grid g;
  rtacc::AdaptLayout l;
  const int rc = open_blob(blob, n, &i, &g, &l);
  if (rc) return rc;
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  for (int64_t t = 0; t < g.tiles; ++t)  // the formula divides by n_t - 1
    if (tile_n(p, l, t) < 2) return RT_ERR_STATE;
  if (tile_max) for (int64_t t = 0; t < g.tiles; ++t) tile_max[t] = 0.0f;
  if (tile_above) for (int64_t t = 0; t < g.tiles; ++t) tile_above[t] = 0;
  float max_noise = 0.0f;
  int64_t above = 0;
  for (int64_t r = 0; r < g.rows; ++r)
    for (int64_t x = 0; x < g.width; ++x) {
      const int64_t px = r * g.width + x, t = (r / rtacc::kNoiseTile) * g.tiles_x + x / rtacc::kNoiseTile;
      uint64_t s2[3];
      uint32_t s1[3];
      memcpy(s2, p + l.s2 + 8 * 3 * px, sizeof(s2));
      memcpy(s1, p + l.s1 + 4 * 3 * px, sizeof(s1));
      const float noise = rtacc::host_pixel_noise(s1, s2, tile_n(p, l, t));
      if (map) map[px] = noise;
      if (noise > max_noise) max_noise = noise;
      if (tile_max && noise > tile_max[t]) tile_max[t] = noise;
      if (noise > threshold) {
        ++above;
        if (tile_above) ++tile_above[t];
      }
    }
  if (rep) {
    rep->fbs = i.args.fb_count;
    rep->tiles_x = (int32_t)g.tiles_x;
    rep->tiles_y = (int32_t)g.tiles_y;
    rep->tiles_active = 0;
    rep->pixels = g.rows * g.width;
    rep->pixels_active = 0;
    rep->pixel_fbs = 0;
    rep->pixels_above = above;
    rep->threshold = threshold;
    rep->max_noise = max_noise;
    for (int64_t t = 0; t < g.tiles; ++t) {
      const int64_t tx = t % g.tiles_x, ty = t / g.tiles_x;
      const int64_t tw = g.width - tx * rtacc::kNoiseTile < rtacc::kNoiseTile ? g.width - tx * rtacc::kNoiseTile : rtacc::kNoiseTile;
      const int64_t th = g.rows - ty * rtacc::kNoiseTile < rtacc::kNoiseTile ? g.rows - ty * rtacc::kNoiseTile : rtacc::kNoiseTile;
      rep->pixel_fbs += tw * th * tile_n(p, l, t);
      if (p[l.active + t]) {
        ++rep->tiles_active;
        rep->pixels_active += tw * th;
      }
    }
  }
  return RT_OK;
}

}  // extern "C"
