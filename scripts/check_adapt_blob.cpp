// check_adapt_blob.cpp — the host-only functions of the adaptive accumulator's checkpoint
// (csrc/rt_adapt_blob.cpp) run once in a stand-alone program, for a sanitizer build:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       -Iraytracing_gpu_amd/csrc scripts/check_adapt_blob.cpp raytracing_gpu_amd/csrc/rt_adapt_blob.cpp \
//       raytracing_gpu_amd/csrc/rt_accum_blob.cpp -o check_adapt_blob && ./check_adapt_blob
//
// A small state with three distinct n_t packed at an aligned and at an odd address; rt_adaptive_blob_info
// at every truncation length, with a flipped byte in every region, and with each violation of what
// include/rt_hip.h calls a valid blob (the payload hash made right again, so that the invariant itself is
// what refuses).  Prints "check_adapt_blob ok" and returns 0, or names the failed check.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_accum_blob.h"
#include "rt_hip.h"

#define CHECK(x)                                       \
  do {                                                 \
    if (!(x)) {                                        \
      printf("FAILED line %d: %s\n", __LINE__, #x);    \
      return 1;                                        \
    }                                                  \
  } while (0)

int main() {
  const int W = 40, H = 20, TILES = 6;  // 3 x 2 tiles, partial in both directions
  rt_accum_info info = {};
  info.args = rt_render_args{W, H, 3, 2, 7, 50, RT_CAM_PER_PIXEL, H, 0, 1, 0, 0, 77};
  info.n_values = (int64_t)W * H * 3;
  info.scene_fp = 0x123456789abcdef0ull;
  const size_t nv = (size_t)info.n_values;
  const int32_t n_t[TILES] = {7, 2, 4, 4, 7, 2};
  const uint8_t active[TILES] = {1, 0, 0, 1, 1, 0};
  std::vector<float> sums(nv);
  std::vector<uint32_t> s1(nv);
  std::vector<uint64_t> s2(nv);
  uint32_t x = 12345;
  for (int r = 0; r < H; ++r)
    for (int col = 0; col < W; ++col) {
      const int n = n_t[(r / 16) * 3 + col / 16];
      for (int j = 0; j < 3; ++j) {  // n values of c per accumulator value from a small LCG
        const size_t k = 3 * ((size_t)r * W + col) + j;
        for (int f = 0; f < n; ++f) {
          x = x * 1664525u + 1013904223u;
          const uint64_t c = (x >> 24) % 256, q = c * c;
          sums[k] += (float)q / (255.0f * 255.0f);
          s1[k] += (uint32_t)q;
          s2[k] += q * q;
        }
      }
    }
  const rtacc::AdaptLayout l = rtacc::adapt_layout(nv, TILES);
  CHECK(l.n_t == 96 && l.active == 96 + 24 && l.pad0 == 126 && l.sums == 128 && l.pad1 == l.s2 && l.total == 128 + 16 * nv);
  size_t need = 0;
  CHECK(rt_adaptive_blob_pack(&info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &need) == RT_OK && need == l.total);
  for (int off = 0; off < 2; ++off) {  // the blob at an 8-byte aligned and at an odd address
    std::vector<unsigned char> store(need + 16);
    unsigned char* blob = store.data() + off;
    CHECK(rt_adaptive_blob_pack(&info, n_t, active, sums.data(), s1.data(), s2.data(), blob, need - 1, nullptr) == RT_ERR_ARG);
    CHECK(rt_adaptive_blob_pack(&info, n_t, active, sums.data(), s1.data(), s2.data(), blob, need, nullptr) == RT_OK);
    rt_accum_info got = {};
    CHECK(rt_adaptive_blob_info(blob, need, &got) == RT_OK);
    CHECK(memcmp(&got.args, &info.args, sizeof(info.args)) == 0 && got.n_values == info.n_values && got.scene_fp == info.scene_fp);
    int32_t tn[TILES];
    uint8_t ta[TILES];
    CHECK(rt_adaptive_blob_tiles(blob, need, tn, ta) == RT_OK && memcmp(tn, n_t, sizeof(tn)) == 0 && memcmp(ta, active, TILES) == 0);
    CHECK(rt_adaptive_blob_tiles(blob, need, nullptr, nullptr) == RT_OK);
    std::vector<uint8_t> img(nv);
    CHECK(rt_adaptive_blob_image(blob, need, img.data()) == RT_OK && rt_adaptive_blob_image(blob, need, nullptr) == RT_ERR_ARG);
    rt_adapt_report rep = {};
    std::vector<float> tmax(TILES), map((size_t)W * H);
    std::vector<int32_t> tabove(TILES);
    CHECK(rt_adaptive_blob_measure(blob, need, 1.0f, &rep, tmax.data(), tabove.data(), map.data()) == RT_OK);
    CHECK(rep.fbs == 7 && rep.tiles_x == 3 && rep.tiles_y == 2 && rep.tiles_active == 3 && rep.pixels == W * H);
    CHECK(rep.pixels_active == 256 + 64 + 64 && rep.pixel_fbs == 256 * 7 + 256 * 2 + 128 * 4 + 64 * 4 + 64 * 7 + 32 * 2);
    int64_t above = 0;
    for (int t = 0; t < TILES; ++t) {
      above += tabove[t];
      CHECK(rep.max_noise >= tmax[t]);
    }
    CHECK(rep.pixels_above == above);
    CHECK(rt_adaptive_blob_measure(blob, need, 1.0f, nullptr, nullptr, nullptr, nullptr) == RT_OK);
    // every truncation length, a byte more, no blob
    for (size_t n = 0; n < need; ++n) CHECK(rt_adaptive_blob_info(blob, n, &got) == RT_ERR_ARG);
    CHECK(rt_adaptive_blob_info(blob, need + 1, &got) == RT_ERR_ARG && rt_adaptive_blob_info(nullptr, need, &got) == RT_ERR_ARG);
    CHECK(rt_adaptive_blob_info(blob, need, nullptr) == RT_ERR_ARG);
    // blob with n bytes at `at` replaced; fix: the payload hash made right again
    auto with = [&](size_t at, const void* bytes, size_t n, bool fix) {
      std::vector<unsigned char> v(need + 16);
      unsigned char* p = v.data() + off;
      memcpy(p, blob, need);
      memcpy(p + at, bytes, n);
      if (fix) {
        const uint64_t h = rtacc::fnv1a(p + 96, need - 96);
        memcpy(p + 88, &h, 8);
      }
      rt_accum_info g = {};
      return rt_adaptive_blob_info(p, need, &g);
    };
    CHECK(with(0, blob, 1, true) == RT_OK);  // the helper itself: nothing changed
    // a flipped byte in each region: header fields (the seed and the scene fingerprint are free), hash, n_t,
    // active, padding, sums, S2, S1
    const size_t at[] = {0, 9, 13, 16, 20, 72, 88, l.n_t + 5, l.active + 2, l.pad0, l.pad0 + 1, l.sums + 101,
                         l.s2 + 1001, l.s1 + 77, need - 1};
    for (size_t a : at) {
      const unsigned char flipped = blob[a] ^ 0x10;
      CHECK(with(a, &flipped, 1, false) == RT_ERR_ARG);
    }
    CHECK(with(0, "RTADAPT2", 8, false) == RT_ERR_ARG && with(0, "RTNOISE1", 8, false) == RT_ERR_ARG);
    const uint32_t two = 2, hundred = 100;
    CHECK(with(8, &two, 4, false) == RT_ERR_ARG && with(12, &hundred, 4, false) == RT_ERR_ARG);
    // the invariants, each with a matching hash: padding not zero
    const unsigned char one = 1;
    CHECK(with(l.pad0, &one, 1, true) == RT_ERR_ARG && with(l.pad0 + 1, &one, 1, true) == RT_ERR_ARG);
    // n_t < 0, n_t > fb_count, no tile at fb_count, a retired tile with n_t < 2, a flag that is neither 0 nor 1
    const int32_t minus = -1, eight = 8, six = 6, i1 = 1, i0 = 0;
    CHECK(with(l.n_t + 4, &minus, 4, true) == RT_ERR_ARG && with(l.n_t + 4, &eight, 4, true) == RT_ERR_ARG);
    {
      std::vector<unsigned char> v(blob, blob + need);
      memcpy(v.data() + l.n_t, &six, 4), memcpy(v.data() + l.n_t + 16, &six, 4);  // both tiles at 7 now at 6
      const uint64_t h = rtacc::fnv1a(v.data() + 96, need - 96);
      memcpy(v.data() + 88, &h, 8);
      CHECK(rt_adaptive_blob_info(v.data(), need, &got) == RT_ERR_ARG);
    }
    CHECK(with(l.n_t + 4, &i1, 4, true) == RT_ERR_ARG && with(l.n_t + 4, &i0, 4, true) == RT_ERR_ARG);
    CHECK(with(l.n_t + 12, &i1, 4, true) == RT_OK);  // an active tile may hold fewer than 2
    const unsigned char flag2 = 2;
    CHECK(with(l.active, &flag2, 1, true) == RT_ERR_ARG);
    // fb_count: beyond the cap, below a tile's n_t, 0 with tiles that are not at 0
    const int32_t over = 32769, full = 32768;
    CHECK(with(16 + 4 * 4, &over, 4, false) == RT_ERR_ARG && with(16 + 4 * 4, &six, 4, false) == RT_ERR_ARG);
    CHECK(with(16 + 4 * 4, &full, 4, false) == RT_ERR_ARG && with(16 + 4 * 4, &i0, 4, false) == RT_ERR_ARG);
    // n_values and the tiling
    const int64_t nvals[] = {0, -1, -3, INT64_MAX, (int64_t)1 << 62, info.n_values - 3, info.n_values + 3};
    for (int64_t v : nvals) CHECK(with(72, &v, 8, false) == RT_ERR_ARG);
    const int32_t vals[] = {0, -1, INT32_MAX, INT32_MIN};
    for (int field = 0; field < 12; ++field)
      for (int32_t v : vals) {
        const int rc = with(16 + 4 * field, &v, 4, false);
        CHECK(rc == RT_OK || rc == RT_ERR_ARG);
        if (field < 2 || field == 4) CHECK(rc == RT_ERR_ARG);  // width, height, fb_count
      }
    // pack in place (every array already where it goes), as rt_adaptive_save does
    CHECK(rt_adaptive_blob_pack(&info, reinterpret_cast<const int32_t*>(blob + l.n_t), blob + l.active,
                                reinterpret_cast<const float*>(blob + l.sums), reinterpret_cast<const uint32_t*>(blob + l.s1),
                                reinterpret_cast<const uint64_t*>(blob + l.s2), blob, need, nullptr) == RT_OK);
    CHECK(rt_adaptive_blob_info(blob, need, &got) == RT_OK);
  }
  // pack refuses what info would refuse
  rt_accum_info bad = info;
  bad.args.fb_count = 6;
  std::vector<unsigned char> bb(need);
  CHECK(rt_adaptive_blob_pack(&bad, n_t, active, sums.data(), s1.data(), s2.data(), bb.data(), need, nullptr) == RT_ERR_ARG);
  bad.args.fb_count = 8;
  CHECK(rt_adaptive_blob_pack(&bad, n_t, active, sums.data(), s1.data(), s2.data(), bb.data(), need, nullptr) == RT_ERR_ARG);
  // the empty state: fb_count = 0, every tile active at 0; it has no image and no measure
  rt_accum_info empty = info;
  empty.args.fb_count = 0;
  const int32_t zeros[TILES] = {};
  const uint8_t ones[TILES] = {1, 1, 1, 1, 1, 1};
  std::fill(sums.begin(), sums.end(), 0.0f), std::fill(s1.begin(), s1.end(), 0u), std::fill(s2.begin(), s2.end(), 0ull);
  CHECK(rt_adaptive_blob_pack(&empty, zeros, ones, sums.data(), s1.data(), s2.data(), bb.data(), need, nullptr) == RT_OK);
  rt_accum_info got = {};
  CHECK(rt_adaptive_blob_info(bb.data(), need, &got) == RT_OK && got.args.fb_count == 0);
  std::vector<uint8_t> img(nv);
  CHECK(rt_adaptive_blob_image(bb.data(), need, img.data()) == RT_ERR_STATE);
  CHECK(rt_adaptive_blob_measure(bb.data(), need, 1.0f, nullptr, nullptr, nullptr, nullptr) == RT_ERR_STATE);
  CHECK(rt_adaptive_blob_pack(&empty, zeros, active, sums.data(), s1.data(), s2.data(), bb.data(), need, nullptr) == RT_ERR_ARG);
  // a band tiling: H = 20 in bands of 4, every second band from the first -> 12 rows, 3 x 1 tiles
  rt_accum_info part = info;
  part.args.band_rows = 4, part.args.band_stride = 2;
  part.n_values = 12 * W * 3;
  part.args.fb_count = 5;
  const int32_t pn[3] = {5, 5, 3};
  const uint8_t pa[3] = {1, 1, 0};
  const rtacc::AdaptLayout pl = rtacc::adapt_layout((size_t)part.n_values, 3);
  std::vector<unsigned char> pb(pl.total);
  CHECK(pl.pad0 == 96 + 15 && pl.sums == 96 + 16);
  CHECK(rt_adaptive_blob_pack(&part, pn, pa, sums.data(), s1.data(), s2.data(), pb.data(), pb.size(), nullptr) == RT_OK);
  CHECK(rt_adaptive_blob_info(pb.data(), pb.size(), &got) == RT_OK && got.n_values == part.n_values);
  // the largest state: 32768 frame buffers, half at c = 255 and half at 0 in the first pixel, the others constant 255
  rt_accum_info big = info;
  big.args.fb_count = 32768;
  const int32_t bn[TILES] = {32768, 32768, 32768, 32768, 32768, 32768};
  for (size_t k = 0; k < nv; ++k) {
    const uint64_t n = k < 3 ? 16384 : 32768;
    s1[k] = (uint32_t)(n * 65025);
    s2[k] = n * 65025 * 65025;
  }
  CHECK(rt_adaptive_blob_pack(&big, bn, ones, sums.data(), s1.data(), s2.data(), bb.data(), need, nullptr) == RT_OK);
  std::vector<float> map((size_t)W * H);
  rt_adapt_report rep = {};
  CHECK(rt_adaptive_blob_measure(bb.data(), need, 0.25f, &rep, nullptr, nullptr, map.data()) == RT_OK);
  CHECK(map[0] > 0.4999f && map[0] < 0.5001f && map[1] == 0.0f && rep.pixels_above == 1 && rep.max_noise == map[0]);
  big.args.fb_count = 32769;
  CHECK(rt_adaptive_blob_pack(&big, bn, ones, sums.data(), s1.data(), s2.data(), bb.data(), need, nullptr) == RT_ERR_ARG);
  printf("check_adapt_blob ok\n");
  return 0;
}
