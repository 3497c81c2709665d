// rt_noise_blob.cpp — the host-only half of the noise monitor (rt_noise_* of include/rt_hip.h): the
// monitor's side file packed, validated and measured without a context or a GPU.  Plain C++ with no
// HIP include; a stand-alone program links this file and rt_accum_blob.cpp.
//
// Blob (little-endian): the 96-byte header of rt_accum_blob.cpp with magic "RTNOISE1", version 1 and
// fb_count = frame buffers measured, then
//   96              u64[n_values]  S2 = sum of c^4
//   96 + 8 n_values u32[n_values]  S1 = sum of c^2        (c = quant(fb[f][k]), owned rows ascending)
//
// The measure is the one of noise_measure_kernel (rt_progressive.hip), tile for tile; rt_hip.h has the
// definitions and the bound that keeps every integer below 2^64.
#include "rt_accum_blob.h"

#include <cmath>
#include <cstring>

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the payload is copied as little-endian integers");

namespace {

const char kMagic[8] = {'R', 'T', 'N', 'O', 'I', 'S', 'E', '1'};
constexpr uint32_t kVersion = 1;
constexpr size_t kBytesPerValue = sizeof(uint64_t) + sizeof(uint32_t);

bool noise_info_ok(const rt_accum_info* i) {
  return rtacc::info_ok(i) && i->args.fb_count <= rtacc::kNoiseMaxFbs &&
         (uint64_t)i->n_values <= (SIZE_MAX - rtacc::kHeaderBytes) / kBytesPerValue;
}

}  // namespace

extern "C" {

int rt_noise_blob_pack(const rt_accum_info* info, const uint32_t* s1, const uint64_t* s2, void* blob, size_t cap,
                       size_t* need) {
  if (!info || !noise_info_ok(info)) return RT_ERR_ARG;
  const size_t nv = (size_t)info->n_values, payload = nv * kBytesPerValue, total = rtacc::kHeaderBytes + payload;
  if (need) *need = total;
  if (!blob && cap == 0) return RT_OK;  // size query
  if (!blob || !s1 || !s2 || cap < total) return RT_ERR_ARG;
  unsigned char* p = static_cast<unsigned char*>(blob);
  // memmove: rt_noise_save has the moments in the blob's payload already
  memmove(p + rtacc::kHeaderBytes, s2, nv * sizeof(uint64_t));
  memmove(p + rtacc::kHeaderBytes + nv * sizeof(uint64_t), s1, nv * sizeof(uint32_t));
  rtacc::put_header(p, kMagic, kVersion, info, rtacc::fnv1a(p + rtacc::kHeaderBytes, payload));
  return RT_OK;
}

int rt_noise_blob_info(const void* blob, size_t n, rt_accum_info* info) {
  if (!blob || !info || n < rtacc::kHeaderBytes) return RT_ERR_ARG;
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  rt_accum_info i = {};
  uint64_t hash = 0;
  if (!rtacc::get_header(p, kMagic, kVersion, &i, &hash)) return RT_ERR_ARG;
  if (!noise_info_ok(&i)) return RT_ERR_ARG;
  const size_t payload = (size_t)i.n_values * kBytesPerValue;
  if (n - rtacc::kHeaderBytes != payload) return RT_ERR_ARG;
  if (rtacc::fnv1a(p + rtacc::kHeaderBytes, payload) != hash) return RT_ERR_ARG;
  *info = i;
  return RT_OK;
}

int rt_noise_blob_measure(const void* blob, size_t n, float threshold, rt_noise_report* rep, float* tile_max,
                          int32_t* tile_above, float* map) {
  rt_accum_info i;
  const int rc = rt_noise_blob_info(blob, n, &i);
  if (rc) return rc;
  if (i.args.fb_count < 2) return RT_ERR_STATE;
  const int64_t width = i.args.width, rows = i.n_values / (3 * width);
  const int64_t tiles_x = (width + rtacc::kNoiseTile - 1) / rtacc::kNoiseTile;
  const int64_t tiles_y = (rows + rtacc::kNoiseTile - 1) / rtacc::kNoiseTile;
  if (tiles_x * tiles_y > INT32_MAX) return RT_ERR_ARG;
  const unsigned char* p2 = static_cast<const unsigned char*>(blob) + rtacc::kHeaderBytes;
  const unsigned char* p1 = p2 + (size_t)i.n_values * sizeof(uint64_t);
  if (tile_max) for (int64_t t = 0; t < tiles_x * tiles_y; ++t) tile_max[t] = 0.0f;
  if (tile_above) for (int64_t t = 0; t < tiles_x * tiles_y; ++t) tile_above[t] = 0;
  float max_noise = 0.0f;
  int64_t above = 0;
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t x = 0; x < width; ++x) {
      const int64_t px = r * width + x;
      uint64_t s2[3];
      uint32_t s1[3];
      memcpy(s2, p2 + 8 * 3 * px, sizeof(s2));
      memcpy(s1, p1 + 4 * 3 * px, sizeof(s1));
      const float noise = rtacc::host_pixel_noise(s1, s2, i.args.fb_count);  // the formula and its bound: rt_accum_blob.h
      if (map) map[px] = noise;
      const int64_t t = (r / rtacc::kNoiseTile) * tiles_x + x / rtacc::kNoiseTile;
      if (noise > max_noise) max_noise = noise;
      if (tile_max && noise > tile_max[t]) tile_max[t] = noise;
      if (noise > threshold) {
        ++above;
        if (tile_above) ++tile_above[t];
      }
    }
  if (rep) {
    rep->fbs = i.args.fb_count;
    rep->tiles_x = (int32_t)tiles_x;
    rep->tiles_y = (int32_t)tiles_y;
    rep->pad = 0;
    rep->pixels = rows * width;
    rep->pixels_above = above;
    rep->threshold = threshold;
    rep->max_noise = max_noise;
  }
  return RT_OK;
}

}  // extern "C"
