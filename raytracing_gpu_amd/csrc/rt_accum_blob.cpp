// rt_accum_blob.cpp — the host-only half of the progressive accumulator (include/rt_hip.h):
// checkpoint blobs packed, validated and finalised into an 8-bit image without a context or a GPU,
// and the scene fingerprint a checkpoint is tied to.  Plain C++ with no HIP include, so that a
// stand-alone program can link this file alone.
//
// Blob (little-endian), 96-byte header then the payload:
//    0  char[8]  magic "RTACCUM1"
//    8  u32      version (1)
//   12  u32      header bytes (96)
//   16  i32[12]  width height spp fb_first fb_count max_depth cam_mode band_rows band_first
//                band_stride stats flags          (fb_count = frame buffers folded in)
//   64  u64      seed
//   72  i64      n_values = owned_rows x width x 3
//   80  u64      scene fingerprint
//   88  u64      FNV-1a of the payload bytes
//   96  f32[n_values]  the sums, owned rows ascending
#include "rt_accum_blob.h"

#include <cmath>
#include <cstring>

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the payload is copied as little-endian floats");

namespace rtacc {

uint64_t fnv1a(const void* data, size_t n, uint64_t h) {
  const unsigned char* p = static_cast<const unsigned char*>(data);
  for (size_t k = 0; k < n; ++k) {
    h ^= p[k];
    h *= 0x100000001b3ull;
  }
  return h;
}

namespace {
template <class T>
uint64_t hash_array(uint64_t h, const T* p, int64_t n) {
  h = fnv1a(&n, sizeof(n), h);
  return p && n > 0 ? fnv1a(p, (size_t)n * sizeof(T), h) : h;
}
}  // namespace

uint64_t scene_fingerprint(const rt_scene_soa* s) {
  uint64_t h = fnv1a(&s->camera, sizeof(s->camera));
  h = fnv1a(s->background, sizeof(s->background), h);
  h = hash_array(h, s->world, s->n_world);
  h = hash_array(h, s->objects, s->n_objects);
  h = hash_array(h, s->prims, s->n_prims);
  h = hash_array(h, s->triangles, s->n_triangles);
  h = hash_array(h, s->nodes, s->n_nodes);
  h = hash_array(h, s->materials, s->n_materials);
  h = hash_array(h, s->textures, s->n_textures);
  h = hash_array(h, s->perlins, s->n_perlins);
  h = hash_array(h, s->images, s->n_images);
  h = hash_array(h, s->texels, s->n_texels);
  return h;
}

int64_t owned_row_count(const rt_render_args* a) {
  if (a->height <= 0 || a->band_rows <= 0 || a->band_stride <= 0 || a->band_first < 0 ||
      a->band_first >= a->band_stride)
    return 0;
  // closed form (a header read from a file may hold any tiling): bands first, first + stride, ...
  // below the band count, the image's last band short by what it lacks
  const int64_t rows = a->band_rows, first = a->band_first, stride = a->band_stride;
  const int64_t bands = (a->height + rows - 1) / rows;
  if (first >= bands) return 0;
  const int64_t owned = (bands - first + stride - 1) / stride;
  const bool owns_last = (bands - 1 - first) % stride == 0;
  return owned * rows - (owns_last ? bands * rows - a->height : 0);
}

namespace {
void put32(unsigned char* p, uint32_t v) {
  for (int k = 0; k < 4; ++k) p[k] = (unsigned char)(v >> (8 * k));
}
void put64(unsigned char* p, uint64_t v) {
  for (int k = 0; k < 8; ++k) p[k] = (unsigned char)(v >> (8 * k));
}
uint32_t get32(const unsigned char* p) {
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k) v |= (uint32_t)p[k] << (8 * k);
  return v;
}
uint64_t get64(const unsigned char* p) {
  uint64_t v = 0;
  for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k);
  return v;
}
}  // namespace

// What a header may hold: render arguments rt_render accepts (fb_count >= 0 here: the frame buffers
// done) and the value count of their tiling.
bool info_ok(const rt_accum_info* i) {
  const rt_render_args& a = i->args;
  if (a.width <= 0 || a.height <= 0 || a.spp <= 0 || a.fb_first < 0 || a.fb_count < 0 || a.max_depth <= 0) return false;
  if (a.cam_mode != RT_CAM_REF_SLOT0 && a.cam_mode != RT_CAM_PER_PIXEL) return false;
  const int64_t rows = owned_row_count(&a);
  // rows, width < 2^31: rows x width fits 64 bits, the factor 3 is checked by division
  return rows > 0 && i->n_values % 3 == 0 && i->n_values / 3 == rows * a.width;
}

void put_header(unsigned char* p, const char* magic, uint32_t version, const rt_accum_info* info, uint64_t payload_hash) {
  memcpy(p, magic, 8);
  put32(p + 8, version);
  put32(p + 12, (uint32_t)kHeaderBytes);
  const rt_render_args& a = info->args;
  const int32_t f[12] = {a.width,    a.height,    a.spp,        a.fb_first,   a.fb_count, a.max_depth,
                         a.cam_mode, a.band_rows, a.band_first, a.band_stride, a.stats,   a.flags};
  for (int k = 0; k < 12; ++k) put32(p + 16 + 4 * k, (uint32_t)f[k]);
  put64(p + 64, a.seed);
  put64(p + 72, (uint64_t)info->n_values);
  put64(p + 80, info->scene_fp);
  put64(p + 88, payload_hash);
}

bool get_header(const unsigned char* p, const char* magic, uint32_t version, rt_accum_info* info, uint64_t* payload_hash) {
  if (memcmp(p, magic, 8) != 0 || get32(p + 8) != version || get32(p + 12) != kHeaderBytes) return false;
  rt_accum_info i = {};
  int32_t f[12];
  for (int k = 0; k < 12; ++k) f[k] = (int32_t)get32(p + 16 + 4 * k);
  rt_render_args& a = i.args;
  a.width = f[0], a.height = f[1], a.spp = f[2], a.fb_first = f[3], a.fb_count = f[4], a.max_depth = f[5];
  a.cam_mode = f[6], a.band_rows = f[7], a.band_first = f[8], a.band_stride = f[9], a.stats = f[10], a.flags = f[11];
  a.seed = get64(p + 64);
  i.n_values = (int64_t)get64(p + 72);
  i.scene_fp = get64(p + 80);
  *payload_hash = get64(p + 88);
  *info = i;
  return true;
}

}  // namespace rtacc

namespace {

const char kMagic[8] = {'R', 'T', 'A', 'C', 'C', 'U', 'M', '1'};
constexpr uint32_t kVersion = 1;

}  // namespace

extern "C" {

int rt_accum_blob_pack(const rt_accum_info* info, const float* sums, void* blob, size_t cap, size_t* need) {
  if (!info || !rtacc::info_ok(info)) return RT_ERR_ARG;
  const size_t payload = (size_t)info->n_values * sizeof(float), total = rtacc::kHeaderBytes + payload;
  if (need) *need = total;
  if (!blob && cap == 0) return RT_OK;  // size query
  if (!blob || !sums || cap < total) return RT_ERR_ARG;
  unsigned char* p = static_cast<unsigned char*>(blob);
  memmove(p + rtacc::kHeaderBytes, sums, payload);
  rtacc::put_header(p, kMagic, kVersion, info, rtacc::fnv1a(p + rtacc::kHeaderBytes, payload));
  return RT_OK;
}

int rt_accum_blob_info(const void* blob, size_t n, rt_accum_info* info) {
  if (!blob || !info || n < rtacc::kHeaderBytes) return RT_ERR_ARG;
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  rt_accum_info i = {};
  uint64_t hash = 0;
  if (!rtacc::get_header(p, kMagic, kVersion, &i, &hash)) return RT_ERR_ARG;
  if (!rtacc::info_ok(&i)) return RT_ERR_ARG;
  const size_t payload = (size_t)i.n_values * sizeof(float);
  if (n - rtacc::kHeaderBytes != payload) return RT_ERR_ARG;
  if (rtacc::fnv1a(p + rtacc::kHeaderBytes, payload) != hash) return RT_ERR_ARG;
  *info = i;
  return RT_OK;
}

int rt_accum_blob_image(const void* blob, size_t n, uint8_t* out) {
  rt_accum_info i;
  const int rc = rt_accum_blob_info(blob, n, &i);
  if (rc) return rc;
  if (!out) return RT_ERR_ARG;
  if (i.args.fb_count < 1) return RT_ERR_STATE;
  const unsigned char* p = static_cast<const unsigned char*>(blob) + rtacc::kHeaderBytes;
  const float nfb = (float)i.args.fb_count;
  for (int64_t k = 0; k < i.n_values; ++k) {
    float s;
    memcpy(&s, p + 4 * k, 4);
    out[k] = (uint8_t)rtacc::host_quant(s / nfb);
  }
  return RT_OK;
}

}  // extern "C"
