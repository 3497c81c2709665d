// check_tile_list.cpp -- csrc/rt_tile_list.h on the CPU: tile_items_kernel's index arithmetic replayed
// over the records of rttile::records, many shapes and tile subsets.  Checks that every written position
// is inside the item list (the kernel's only store), that the positions are a permutation, that the items
// are exactly the (row, fb, column) triples of the listed tiles, and the tile-major order: a tile's pixels
// of one frame buffer in one run.  Stand-alone (own main); built by tests/test_adapt_cpu.py with g++, and
// run once by hand under -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -I raytracing_gpu_amd/csrc scripts/check_tile_list.cpp -o /tmp/ctl && /tmp/ctl
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "rt_tile_list.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      if (failures++ < 20) {            \
        fprintf(stderr, "FAIL %s: ", #cond); \
        fprintf(stderr, __VA_ARGS__);   \
        fprintf(stderr, "\n");          \
      }                                 \
    }                                   \
  } while (0)

void run(int rows, int width, int fb_count, const std::vector<int32_t>& tiles) {
  const int tiles_x = (width + 15) / 16;
  std::vector<rttile::Rec> rec;
  const unsigned long long n = rttile::records(tiles.data(), (int)tiles.size(), tiles_x, rows, width, fb_count, rec);
  unsigned long long want = 0;
  std::vector<uint8_t> listed((size_t)tiles_x * ((rows + 15) / 16), 0);
  for (int32_t t : tiles) {
    int tw, th;
    rttile::size(t, tiles_x, rows, width, tw, th);
    CHECK(tw >= 1 && tw <= 16 && th >= 1 && th <= 16, "tile %d size %d x %d", t, tw, th);
    want += (unsigned long long)tw * th * fb_count;
    listed[(size_t)t] = 1;
  }
  CHECK(n == want, "%d x %d x %d: %llu items, want %llu", rows, width, fb_count, n, want);
  CHECK(rec.size() == tiles.size(), "record count");
  const uint32_t kUnset = 0xFFFFFFFFu;
  std::vector<uint32_t> perm((size_t)n, kUnset);
  // tile_items_kernel: one workgroup per record, one lane per pixel
  for (const rttile::Rec& d : rec)
    for (int lane = 0; lane < 256; ++lane) {
      const int lx = lane & 15, ly = lane >> 4;
      const int col = (int)(d.id % (unsigned)tiles_x) * 16 + lx, row = (int)(d.id / (unsigned)tiles_x) * 16 + ly;
      if (col >= width || row >= rows) continue;
      const unsigned long long first = (unsigned long long)row * fb_count * width + col;
      const unsigned long long pos = (unsigned long long)d.base + (unsigned long long)ly * d.row_stride + lx;
      for (int f = 0; f < fb_count; ++f) {
        const unsigned long long p = pos + (unsigned long long)f * d.fb_stride;
        CHECK(p < n, "position %llu outside %llu items (tile %u)", p, n, d.id);
        if (p >= n) continue;
        CHECK(perm[(size_t)p] == kUnset, "position %llu written twice", p);
        perm[(size_t)p] = (uint32_t)(first + (unsigned long long)f * width);
      }
    }
  // the render kernels' decode: item -> (row position, fb, column)
  std::vector<uint8_t> seen((size_t)rows * fb_count * width, 0);
  for (unsigned long long p = 0; p < n; ++p) {
    const uint32_t item = perm[(size_t)p];
    CHECK(item != kUnset, "position %llu never written", p);
    if (item == kUnset) continue;
    const long long per_row = (long long)fb_count * width;
    const int q = (int)(item / per_row), f = (int)((item - (long long)q * per_row) / width),
              i = (int)(item - (long long)q * per_row - (long long)f * width);
    CHECK(q < rows && f < fb_count && i < width, "item %u decodes outside the image", item);
    CHECK(listed[(size_t)(q / 16) * tiles_x + i / 16], "item %u is in no listed tile", item);
    CHECK(!seen[item], "item %u twice", item);
    seen[item] = 1;
    if (p > 0 && perm[(size_t)p - 1] != kUnset) {  // a tile's pixels of one fb are one run
      const uint32_t prev = perm[(size_t)p - 1];
      const int pq = (int)(prev / per_row), pf = (int)((prev - (long long)pq * per_row) / width),
                pi = (int)(prev - (long long)pq * per_row - (long long)pf * width);
      const bool same_tile = pq / 16 == q / 16 && pi / 16 == i / 16;
      CHECK(!same_tile || pf <= f, "tile-major: fb order inside a tile at %llu", p);
      CHECK(!same_tile || pf != f || prev < item, "tile-major: pixel order inside a tile's fb at %llu", p);
    }
  }
}

}  // namespace

int main() {
  std::mt19937 rng(20240611);
  const int shapes[][2] = {{37, 70}, {48, 80}, {17, 70}, {1, 1}, {16, 16}, {17, 17}, {5, 300}, {300, 5}, {33, 31}};
  long long cases = 0;
  for (const auto& s : shapes)
    for (int fb_count : {1, 3, 10}) {
      const int rows = s[0], width = s[1];
      const int n_all = ((rows + 15) / 16) * ((width + 15) / 16);
      std::vector<int32_t> all((size_t)n_all);
      for (int t = 0; t < n_all; ++t) all[(size_t)t] = t;
      run(rows, width, fb_count, all);
      run(rows, width, fb_count, {n_all - 1});
      run(rows, width, fb_count, {0});
      for (int trial = 0; trial < 16; ++trial) {  // random subsets in random order
        std::vector<int32_t> pick = all;
        std::shuffle(pick.begin(), pick.end(), rng);
        pick.resize((size_t)(1 + rng() % (unsigned)n_all));
        run(rows, width, fb_count, pick);
        ++cases;
      }
      cases += 3;
    }
  // the largest list the ABI accepts: 2^31 items (records only; the list itself is not expanded)
  {
    const int rows = 32768, width = 32768, fb_count = 2;
    const int tiles_x = width / 16;
    std::vector<int32_t> all((size_t)tiles_x * (rows / 16));
    for (size_t t = 0; t < all.size(); ++t) all[t] = (int32_t)t;
    std::vector<rttile::Rec> rec;
    const unsigned long long n = rttile::records(all.data(), (int)all.size(), tiles_x, rows, width, fb_count, rec);
    CHECK(n == (1ull << 31), "2^31 items: %llu", n);
    const rttile::Rec& last = rec.back();
    const unsigned long long top = (unsigned long long)last.base + 15ull * last.row_stride + (unsigned long long)(fb_count - 1) * last.fb_stride + 15;
    CHECK(top == n - 1, "2^31 items: last position %llu", top);
  }
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("check_tile_list ok: %lld cases\n", cases);
  return 0;
}
