// rt_tile_list.h -- the item list of a launch over a set of noise tiles (rt_render_tiles, rt_adapt), host
// side: plain C++ without HIP, so that scripts/check_tile_list.cpp can run it on the CPU.
//
// "Noise tile" is the noise monitor's tile of rtacc::kNoiseTile = 16 x 16 pixels over (owned-row index,
// column), id = ty * tiles_x + tx -- never the 8 x 8 camera-ray tile of the render kernels.
#ifndef RT_TILE_LIST_H
#define RT_TILE_LIST_H

#include <algorithm>
#include <cstdint>
#include <vector>

namespace rttile {

constexpr int kTile = 16;  // = rtacc::kNoiseTile

// One listed tile for tile_items_kernel (read there as a uint4): pixel (ly, lx) of the tile in frame
// buffer f goes to position base + ly * row_stride + f * fb_stride + lx of the item list.
struct Rec {
  uint32_t id, base, row_stride, fb_stride;
};
static_assert(sizeof(Rec) == 16, "tile_items_kernel reads a record as one uint4");

// Valid pixels of noise tile id: width x height of its part inside rows x width.
inline void size(int id, int tiles_x, int rows, int width, int& tw, int& th) {
  const int tx = id % tiles_x, ty = id / tiles_x;
  tw = std::min(kTile, width - tx * kTile);
  th = std::min(kTile, rows - ty * kTile);
}

// Item order of a tile launch, tile-major: the listed tiles one after another, inside a tile one frame
// buffer after another, inside that the tile's pixels row by row -- adjacent claims are neighbouring
// pixels of one frame buffer.  (Measured against ascending items, rt_render's own order restricted to the
// list)
//
// The records of the listed tiles (distinct ids inside the grid; fb_count x rows x width <= 2^31) and
// the item count: the positions the records describe are a permutation of 0 .. count - 1.
inline unsigned long long records(const int32_t* tiles, int n_tiles, int tiles_x, int rows, int width, int fb_count,
                                  std::vector<Rec>& rec) {
  rec.resize((size_t)n_tiles);
  unsigned long long pixels = 0;
  for (int k = 0; k < n_tiles; ++k) {
    int tw, th;
    size(tiles[k], tiles_x, rows, width, tw, th);
    rec[(size_t)k] = Rec{(uint32_t)tiles[k], (uint32_t)(pixels * fb_count), (uint32_t)tw, (uint32_t)(tw * th)};
    pixels += (unsigned long long)tw * th;
  }
  return pixels * (unsigned long long)fb_count;
}

}  // namespace rttile

#endif  // RT_TILE_LIST_H
