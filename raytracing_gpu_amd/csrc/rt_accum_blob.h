// rt_accum_blob.h — internal: what rt_kernels.hip shares with the host-only checkpoint code of
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

}  // namespace rtacc

#endif
