// rt_accum_blob.h — internal: what rt_kernels.hip and rt_progressive.hip share with the host-only checkpoint code of
// rt_accum_blob.cpp (the rt_accum_blob_* entry points themselves are declared in include/rt_hip.h).
#ifndef RT_ACCUM_BLOB_H
#define RT_ACCUM_BLOB_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_hip.h"

namespace rtacc {

constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;
constexpr size_t kHeaderBytes = 96;

// 64-bit FNV-1a over n bytes, continuing from h.
uint64_t fnv1a(const void* data, size_t n, uint64_t h = kFnvBasis);
// FNV-1a over the camera, the background and every array of the flattened scene (each preceded by
// its element count), in rt_scene_soa's field order.
uint64_t scene_fingerprint(const rt_scene_soa* s);
// Rows owned by the tiling of a (rt_owned_rows without the row list); 0 for a malformed tiling.
int64_t owned_row_count(const rt_render_args* a);
// What a blob header may hold: render arguments rt_render accepts (fb_count >= 0: frame buffers
// done) and n_values = owned rows x width x 3 of their tiling.
bool info_ok(const rt_accum_info* info);
// The 96-byte header shared by the accumulator's checkpoint and the noise monitor's side file
// (rt_noise_blob.cpp): magic[8], version, header bytes, the 13 rt_render_args fields, n_values, scene
// fingerprint, FNV-1a of the payload.  get_header is false for another magic, version or header size;
// it does not judge the fields (info_ok does).
void put_header(unsigned char* p, const char* magic, uint32_t version, const rt_accum_info* info, uint64_t payload_hash);
bool get_header(const unsigned char* p, const char* magic, uint32_t version, rt_accum_info* info, uint64_t* payload_hash);

// Noise monitor (rt_noise_* of include/rt_hip.h).
constexpr int32_t kNoiseMaxFbs = 32768;  // frame buffers a monitor accepts, see rt_hip.h for the bound
constexpr int kNoiseTile = 16;           // tiles of 16 x 16 pixels over (owned-row index, column)

// The noise of one pixel on the host, from its three channels' moments after n >= 2 frame buffers: the
// formula of include/rt_hip.h in its order, as pixel_noise (rt_progressive.hip) has it on the device.  The
// one statement of it for rt_noise_blob_measure and rt_adaptive_blob_measure.  n <= 32768 = 2^15,
// c^2 <= 65025 < 2^16, c^4 < 2^32: n S2 <= 2^15 n c^4 < 2^62 and S1^2 <= (n c^2)^2 < 2^62 per channel (both
// <= 4.6e18), their three-channel sum <= 1.4e19 < 2^64; each term n S2 - S1^2 >= 0 by Cauchy-Schwarz.
inline float host_pixel_noise(const uint32_t s1[3], const uint64_t s2[3], int32_t n) {
  uint64_t D = 0, S = 0;
  for (int j = 0; j < 3; ++j) {
    D += (uint64_t)n * s2[j] - (uint64_t)s1[j] * s1[j];
    S += s1[j];
  }
  const double dn = (double)n, dn1 = (double)(n - 1);
  const double a = (double)D / (3.0 * dn * dn * dn1 * 4228250625.0);
  double m = (double)S / (3.0 * dn * 65025.0);
  if (m < 0x1p-16) m = 0x1p-16;
  return (float)(128.0 * __builtin_sqrt(a / m));
}

// write_frame_buffer's quantisation (color.h:40-44) on the host, as the device code has it; NaN defined as 0.
inline int host_quant(float x) {
  const float r = __builtin_sqrtf(x);
  if (!(r == r)) return 0;
  const float c = r < 0.0f ? 0.0f : (r > 0.999f ? 0.999f : r);
  return (int)(256.0f * c);
}

// Adaptive accumulator's checkpoint (rt_adaptive_* of include/rt_hip.h, rt_adapt_blob.cpp): where the
// sections of a blob for n_values values and `tiles` noise tiles lie.
struct AdaptLayout {
  size_t n_t, active, pad0, sums, pad1, s2, s1, total;  // byte offsets; pad0 / pad1: first padding byte
};
inline AdaptLayout adapt_layout(size_t n_values, size_t tiles) {
  AdaptLayout l;
  l.n_t = kHeaderBytes;
  l.active = l.n_t + 4 * tiles;
  l.pad0 = l.active + tiles;
  l.sums = (l.pad0 + 7) & ~(size_t)7;
  l.pad1 = l.sums + 4 * n_values;
  l.s2 = (l.pad1 + 7) & ~(size_t)7;
  l.s1 = l.s2 + 8 * n_values;
  l.total = l.s1 + 4 * n_values;
  return l;
}

}  // namespace rtacc

#endif
