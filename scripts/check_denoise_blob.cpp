// check_denoise_blob.cpp -- the denoiser's host-only twin (csrc/rt_denoise_blob.cpp) in a stand-alone program,
// the one a sanitizer build runs: images smaller than the window, than a patch and than a noise tile, every
// patch radius, a monitor's side file and an adaptive checkpoint with mixed counts, the refusals.
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Iraytracing_gpu_amd/csrc scripts/check_denoise_blob.cpp \
//       raytracing_gpu_amd/csrc/rt_{accum,noise,adapt,denoise}_blob.cpp -o check_denoise_blob && ./check_denoise_blob
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_hip.h"

#define CHECK(x)                                                \
  do {                                                          \
    if (!(x)) {                                                 \
      printf("check_denoise_blob: line %d: %s\n", __LINE__, #x); \
      return 1;                                                 \
    }                                                           \
  } while (0)

int main() {
  const int cases[][4] = {{23, 19, 3, 1}, {40, 37, 10, 3}, {5, 3, 10, 3}, {1, 1, 10, 3}, {7, 2, 10, 0}, {2, 9, 4, 2}, {33, 17, 0, 3}};
  unsigned seed = 12345;
  auto next = [&]() { return (seed = seed * 1664525u + 1013904223u) >> 24; };  // 0..255
  for (const auto& z : cases) {
    const int W = z[0], H = z[1];
    rt_accum_info info = {};
    info.args.width = W;
    info.args.height = H;
    info.args.spp = 1;
    info.args.fb_count = 5;
    info.args.max_depth = 50;
    info.args.band_rows = H;
    info.args.band_stride = 1;
    info.n_values = (int64_t)W * H * 3;
    const size_t nv = (size_t)info.n_values;
    std::vector<uint32_t> s1(nv);
    std::vector<uint64_t> s2(nv);
    for (size_t k = 0; k < nv; ++k) {
      uint64_t a = 0, b = 0;
      for (int f = 0; f < 5; ++f) {
        const uint64_t c = k % 7 == 0 ? 255 : next();
        a += c * c;
        b += c * c * c * c;
      }
      s1[k] = (uint32_t)a;
      s2[k] = b;
    }
    size_t need = 0;
    CHECK(rt_noise_blob_pack(&info, nullptr, nullptr, nullptr, 0, &need) == RT_OK);
    std::vector<unsigned char> blob(need);
    CHECK(rt_noise_blob_pack(&info, s1.data(), s2.data(), blob.data(), need, nullptr) == RT_OK);
    rt_denoise_params p;
    rt_denoise_params_default(&p);
    p.search_radius = z[2];
    p.patch_radius = z[3];
    std::vector<uint8_t> out(nv, 0xAB), again(nv);
    std::vector<float> gain((size_t)W * H, -1.0f);
    CHECK(rt_denoise_monitor_blob(blob.data(), need, &p, out.data(), gain.data()) == RT_OK);
    CHECK(rt_denoise_monitor_blob(blob.data(), need, &p, again.data(), nullptr) == RT_OK && again == out);
    const float window = (float)((2 * z[2] + 1) * (2 * z[2] + 1));
    for (float g : gain) CHECK(g >= 1.0f && g <= window);
    // refusals: nothing written
    std::vector<uint8_t> untouched(nv, 0xAB);
    rt_denoise_params bad = p;
    bad.search_radius = 11;
    CHECK(rt_denoise_monitor_blob(blob.data(), need, &bad, untouched.data(), nullptr) == RT_ERR_ARG);
    bad = p;
    bad.eps = 0.0f;
    CHECK(rt_denoise_monitor_blob(blob.data(), need, &bad, untouched.data(), nullptr) == RT_ERR_ARG);
    CHECK(rt_denoise_monitor_blob(blob.data(), need - 1, &p, untouched.data(), nullptr) == RT_ERR_ARG);
    CHECK(rt_denoise_adaptive_blob(blob.data(), need, &p, untouched.data(), nullptr) == RT_ERR_ARG);
    for (uint8_t b : untouched) CHECK(b == 0xAB);
    // an adaptive checkpoint of the same moments with mixed counts
    const int tiles = ((W + 15) / 16) * ((H + 15) / 16);
    std::vector<int32_t> n_t((size_t)tiles);
    std::vector<uint8_t> active((size_t)tiles, 0);
    std::vector<float> sums(nv, 0.0f);
    for (int t = 0; t < tiles; ++t) n_t[(size_t)t] = t % 2 ? 5 : 9;
    info.args.fb_count = 9;
    CHECK(rt_adaptive_blob_pack(&info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &need) == RT_OK);
    blob.resize(need);
    CHECK(rt_adaptive_blob_pack(&info, n_t.data(), active.data(), sums.data(), s1.data(), s2.data(), blob.data(), need, nullptr) == RT_OK);
    CHECK(rt_denoise_adaptive_blob(blob.data(), need, &p, out.data(), gain.data()) == RT_OK);
    CHECK(rt_denoise_monitor_blob(blob.data(), need, &p, untouched.data(), nullptr) == RT_ERR_ARG);
  }
  puts("check_denoise_blob ok");
  return 0;
}
