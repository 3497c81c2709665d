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

}  // namespace rtacc

#endif
