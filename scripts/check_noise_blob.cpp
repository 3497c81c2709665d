// check_noise_blob.cpp — the host-only noise-monitor functions (csrc/rt_noise_blob.cpp) run once in a
// stand-alone program, for a sanitizer build:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       scripts/check_noise_blob.cpp raytracing_gpu_amd/csrc/rt_noise_blob.cpp \
//       raytracing_gpu_amd/csrc/rt_accum_blob.cpp -o check_noise_blob && ./check_noise_blob
//
// A valid blob aligned and unaligned, every rejection of rt_noise_blob_info, header fields at 0, -1,
// INT32_MAX and INT32_MIN, the largest monitor (32768 frame buffers, c = 255 / 0).  Prints "ok" and
// returns 0, or names the failed check.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_hip.h"

#define CHECK(x)                                       \
  do {                                                 \
    if (!(x)) {                                        \
      printf("FAILED line %d: %s\n", __LINE__, #x);    \
      return 1;                                        \
    }                                                  \
  } while (0)

int main() {
  const int W = 17, H = 9, NFB = 5;
  rt_accum_info info = {};
  info.args = rt_render_args{W, H, 3, 2, NFB, 50, RT_CAM_PER_PIXEL, H, 0, 1, 0, 0, 77};
  info.n_values = (int64_t)W * H * 3;
  info.scene_fp = 0x123456789abcdef0ull;
  const size_t nv = (size_t)info.n_values;
  std::vector<uint32_t> s1(nv);
  std::vector<uint64_t> s2(nv);
  uint32_t x = 12345;
  for (size_t k = 0; k < nv; ++k) {  // NFB values of c per accumulator value from a small LCG
    for (int f = 0; f < NFB; ++f) {
      x = x * 1664525u + 1013904223u;
      const uint64_t c = (x >> 24) % 256, q = c * c;
      s1[k] += (uint32_t)q;
      s2[k] += q * q;
    }
  }
  size_t need = 0;
  CHECK(rt_noise_blob_pack(&info, nullptr, nullptr, nullptr, 0, &need) == RT_OK && need == 96 + 12 * nv);
  const size_t tiles = 2;
  for (int off = 0; off < 2; ++off) {  // the blob at an 8-byte aligned and at an odd address
    std::vector<unsigned char> store(need + 16);
    unsigned char* blob = store.data() + off;
    CHECK(rt_noise_blob_pack(&info, s1.data(), s2.data(), blob, need - 1, nullptr) == RT_ERR_ARG);
    CHECK(rt_noise_blob_pack(&info, s1.data(), s2.data(), blob, need, nullptr) == RT_OK);
    rt_accum_info got = {};
    CHECK(rt_noise_blob_info(blob, need, &got) == RT_OK);
    CHECK(memcmp(&got.args, &info.args, sizeof(info.args)) == 0 && got.n_values == info.n_values && got.scene_fp == info.scene_fp);
    rt_noise_report rep = {};
    std::vector<float> tmax(tiles), map((size_t)W * H);
    std::vector<int32_t> tabove(tiles);
    CHECK(rt_noise_blob_measure(blob, need, 1.0f, &rep, tmax.data(), tabove.data(), map.data()) == RT_OK);
    CHECK(rep.fbs == NFB && rep.tiles_x == 2 && rep.tiles_y == 1 && rep.pixels == W * H);
    CHECK(rep.pixels_above == tabove[0] + tabove[1] && rep.max_noise >= tmax[0] && rep.max_noise >= tmax[1]);
    CHECK(rt_noise_blob_measure(blob, need, 1.0f, nullptr, nullptr, nullptr, nullptr) == RT_OK);
    // rejections: truncation, size, magic, version, header size, checksum, n_values, tiling, fb_count
    CHECK(rt_noise_blob_info(blob, need - 1, &got) == RT_ERR_ARG);
    CHECK(rt_noise_blob_info(blob, 96, &got) == RT_ERR_ARG && rt_noise_blob_info(blob, 40, &got) == RT_ERR_ARG);
    CHECK(rt_noise_blob_info(blob, 0, &got) == RT_ERR_ARG && rt_noise_blob_info(nullptr, need, &got) == RT_ERR_ARG);
    CHECK(rt_noise_blob_info(blob, need + 1, &got) == RT_ERR_ARG);
    auto with = [&](size_t at, const void* bytes, size_t n) {
      std::vector<unsigned char> s2v(need + 16);
      memcpy(s2v.data() + off, blob, need);
      memcpy(s2v.data() + off + at, bytes, n);
      rt_accum_info g = {};
      return rt_noise_blob_info(s2v.data() + off, need, &g);
    };
    CHECK(with(0, "RTNOISE2", 8) == RT_ERR_ARG && with(0, "RTACCUM1", 8) == RT_ERR_ARG);
    const uint32_t two = 2, hundred = 100;
    CHECK(with(8, &two, 4) == RT_ERR_ARG && with(12, &hundred, 4) == RT_ERR_ARG);
    const unsigned char flipped = blob[96 + 101] ^ 0x10, flipped_last = blob[need - 1] ^ 1;
    CHECK(with(96 + 101, &flipped, 1) == RT_ERR_ARG && with(need - 1, &flipped_last, 1) == RT_ERR_ARG);
    const int32_t over = 32769;
    CHECK(with(16 + 4 * 4, &over, 4) == RT_ERR_ARG);
    const int32_t full = 32768;
    CHECK(with(16 + 4 * 4, &full, 4) == RT_OK);
    const int64_t nvals[] = {0, -1, -3, INT64_MAX, (int64_t)1 << 62, info.n_values - 3, info.n_values + 3};
    for (int64_t v : nvals) CHECK(with(72, &v, 8) == RT_ERR_ARG);
    const int32_t vals[] = {0, -1, INT32_MAX, INT32_MIN};
    int accepted = 0;
    for (int field = 0; field < 12; ++field)
      for (int32_t v : vals) {
        const int rc = with(16 + 4 * field, &v, 4);
        CHECK(rc == RT_OK || rc == RT_ERR_ARG);
        accepted += rc == RT_OK;
      }
    CHECK(accepted == 9 + 8);  // the combinations tests/test_noise_cpu.py lists, and stats / flags at INT32_MIN
    // one and zero frame buffers: a valid blob that cannot be measured
    rt_accum_info one = info;
    one.args.fb_count = 1;
    CHECK(rt_noise_blob_pack(&one, s1.data(), s2.data(), blob, need, nullptr) == RT_OK);
    CHECK(rt_noise_blob_measure(blob, need, 1.0f, &rep, nullptr, nullptr, nullptr) == RT_ERR_STATE);
    // pack in place (payload already where it goes), as rt_noise_save does
    CHECK(rt_noise_blob_pack(&info, s1.data(), s2.data(), blob, need, nullptr) == RT_OK);
    CHECK(rt_noise_blob_pack(&info, reinterpret_cast<const uint32_t*>(blob + 96 + 8 * nv),
                             reinterpret_cast<const uint64_t*>(blob + 96), blob, need, nullptr) == RT_OK);
    CHECK(rt_noise_blob_info(blob, need, &got) == RT_OK);
  }
  // partial tiling: H = 9 in bands of 4, every second band from the first -> 5 rows
  rt_accum_info part = info;
  part.args.band_rows = 4, part.args.band_stride = 2;
  part.n_values = 5 * W * 3;
  std::vector<unsigned char> pb(96 + 12 * (size_t)part.n_values);
  CHECK(rt_noise_blob_pack(&part, s1.data(), s2.data(), pb.data(), pb.size(), nullptr) == RT_OK);
  rt_accum_info got = {};
  CHECK(rt_noise_blob_info(pb.data(), pb.size(), &got) == RT_OK && got.n_values == part.n_values);
  part.n_values = info.n_values;
  CHECK(rt_noise_blob_pack(&part, s1.data(), s2.data(), nullptr, 0, &need) == RT_ERR_ARG);
  // the largest monitor: 32768 frame buffers, half at c = 255 and half at 0, the other pixels constant 255
  rt_accum_info big = info;
  big.args.fb_count = 32768;
  for (size_t k = 0; k < nv; ++k) {
    const uint64_t n = k < 3 ? 16384 : 32768;
    s1[k] = (uint32_t)(n * 65025);
    s2[k] = n * 65025 * 65025;
  }
  std::vector<unsigned char> bb(96 + 12 * nv);
  CHECK(rt_noise_blob_pack(&big, s1.data(), s2.data(), bb.data(), bb.size(), nullptr) == RT_OK);
  std::vector<float> map((size_t)W * H);
  rt_noise_report rep = {};
  CHECK(rt_noise_blob_measure(bb.data(), bb.size(), 0.25f, &rep, nullptr, nullptr, map.data()) == RT_OK);
  CHECK(map[0] > 0.4999f && map[0] < 0.5001f && map[1] == 0.0f && rep.pixels_above == 1 && rep.max_noise == map[0]);
  big.args.fb_count = 32769;
  CHECK(rt_noise_blob_pack(&big, s1.data(), s2.data(), bb.data(), bb.size(), nullptr) == RT_ERR_ARG);
  printf("ok\n");
  return 0;
}
