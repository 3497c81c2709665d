// rt_progressive.hip -- what is built on rt_render rather than inside it: the progressive accumulator
// (rt_accum), its noise monitor (rt_noise), launches over a set of noise tiles (rt_render_tiles) and the
// adaptive accumulator (rt_adapt) of include/rt_hip.h, kernels and host code.  It reaches the render side
// (rt_kernels.hip) through rt_ctx_internal.h and the public rt_render / rt_render_init only; no device
// code is called across the two files.  The denoiser's entry points on rt_noise and rt_adapt are here too; its
// kernels are rt_denoise.hip's.  Both own their device memory through rt_devbuf.h (DevBuf, Staged).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_accum_blob.h"
#include "rt_ctx_internal.h"
#include "rt_denoise.h"
#include "rt_denoise_math.h"
#include "rt_devbuf.h"
#include "rt_guide.h"
#include "rt_quant.h"
#include "rt_tile_list.h"

namespace {

// The fold of one frame-buffer value v into its accumulator value, stated once for every kernel that
// folds: c = quant(v); a += float(c*c) / (255*255) -- resolve_kernel's operations on its acc -- and, with
// MOMENTS, the integer moments S1 += c^2 (u32), S2 += c^4 (u64).  The byte identity of the three
// accumulators' sums and moments is this function being the only one.
template <bool MOMENTS>
__device__ __forceinline__ void fold1(float v, float& a, uint32_t& m1, unsigned long long& m2) {
  const int c = quant(v);
  a += (float)(c * c) / (255.0f * 255.0f);
  if (MOMENTS) {
    const uint32_t q = (uint32_t)(c * c);
    m1 += q;
    m2 += (unsigned long long)q * q;
  }
}
// fold1 on the 4 consecutive values of a lane (the S2 quad in two 16-byte pairs), written out in the order
// accum_add_stats_kernel<true> was measured with: four calls of fold1 compile to another schedule.
template <bool MOMENTS>
__device__ __forceinline__ void fold4(const float4 v, float4& a, uint4& m1, ulonglong2& m2a, ulonglong2& m2b) {
  const int cx = quant(v.x), cy = quant(v.y), cz = quant(v.z), cw = quant(v.w);
  a.x += (float)(cx * cx) / (255.0f * 255.0f);
  a.y += (float)(cy * cy) / (255.0f * 255.0f);
  a.z += (float)(cz * cz) / (255.0f * 255.0f);
  a.w += (float)(cw * cw) / (255.0f * 255.0f);
  if (MOMENTS) {
    const uint32_t qx = (uint32_t)(cx * cx), qy = (uint32_t)(cy * cy), qz = (uint32_t)(cz * cz), qw = (uint32_t)(cw * cw);
    m1.x += qx;
    m1.y += qy;
    m1.z += qz;
    m1.w += qw;
    m2a.x += (unsigned long long)qx * qx;
    m2a.y += (unsigned long long)qy * qy;
    m2b.x += (unsigned long long)qz * qz;
    m2b.y += (unsigned long long)qw * qw;
  }
}

// The body of accum_add_kernel (MOMENTS = false: s1, s2 are not touched) and accum_add_stats_kernel.
// A pure stream: a lane owns 4 consecutive elements.  VEC (per_fb % 4 == 0, fb and sums -- with
// MOMENTS s1 and s2 too -- 16-byte aligned, so every frame buffer's start f*per_fb is too): one 16-byte
// load per frame buffer, one 16-byte load and store of the sums (and of the S1 quad, two 16-byte pairs
// for S2), consecutive lanes on consecutive 16 bytes; elements past the last whole group of 4, and
// everything when !VEC (odd per_fb, an offset fb pointer), go one by one.
template <bool VEC, bool MOMENTS>
__device__ __forceinline__ void accum_add_body(const float* __restrict__ fb, float* __restrict__ sums,
                                               uint32_t* __restrict__ s1, unsigned long long* __restrict__ s2,
                                               long long per_fb, int nfb) {
  const long long k0 = 4 * ((long long)blockIdx.x * kBlock + threadIdx.x);
  if (k0 >= per_fb) return;
  if (VEC && k0 + 4 <= per_fb) {
    float4 a = *reinterpret_cast<const float4*>(sums + k0);
    uint4 m1 = {};
    ulonglong2 m2a = {}, m2b = {};
    if (MOMENTS) {
      m1 = *reinterpret_cast<const uint4*>(s1 + k0);
      m2a = *reinterpret_cast<const ulonglong2*>(s2 + k0);
      m2b = *reinterpret_cast<const ulonglong2*>(s2 + k0 + 2);
    }
#pragma unroll 4
    for (int f = 0; f < nfb; ++f)
      fold4<MOMENTS>(*reinterpret_cast<const float4*>(fb + (long long)f * per_fb + k0), a, m1, m2a, m2b);
    *reinterpret_cast<float4*>(sums + k0) = a;
    if (MOMENTS) {
      *reinterpret_cast<uint4*>(s1 + k0) = m1;
      *reinterpret_cast<ulonglong2*>(s2 + k0) = m2a;
      *reinterpret_cast<ulonglong2*>(s2 + k0 + 2) = m2b;
    }
    return;
  }
  const long long k1 = k0 + 4 < per_fb ? k0 + 4 : per_fb;
  for (long long k = k0; k < k1; ++k) {
    float a = sums[k];
    uint32_t m1 = MOMENTS ? s1[k] : 0;
    unsigned long long m2 = MOMENTS ? s2[k] : 0;
    for (int f = 0; f < nfb; ++f) fold1<MOMENTS>(fb[(long long)f * per_fb + k], a, m1, m2);
    sums[k] = a;
    if (MOMENTS) {
      s1[k] = m1;
      s2[k] = m2;
    }
  }
}

// Progressive accumulator (rt_accum): resolve_kernel's sum kept in memory between launches, so that
// it can be cut after any frame buffer.  Element k: a = sums[k]; a += float(c*c) / (255*255) for
// c = quant(fb[f][k]), f = 0..nfb-1 in order; sums[k] = a -- the same float operations in the same
// order as resolve_kernel's acc (the sums start at 0.0f as acc does).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void accum_add_kernel(const float* __restrict__ fb, float* __restrict__ sums,
                                                          long long per_fb, int nfb) {
  accum_add_body<VEC, false>(fb, sums, nullptr, nullptr, per_fb, nfb);
}

// accum_add_kernel with a noise monitor attached (rt_noise, include/rt_hip.h): the same single pass
// over the frame buffers, the float sums updated by the same float operations in the same order
// (byte-identical sums), and per value the integer moments S1 += c^2 (u32), S2 += c^4 (u64).  A fold
// is refused before launch when the monitor would pass 32768 frame buffers, so S1 <= 2^15 x 65025
// < 2^31 and S2 <= 2^15 x 65025^2 < 2^47 never wrap.  Traffic per value: 4 nfb bytes in, 8 + 8 + 16
// bytes of state.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void accum_add_stats_kernel(const float* __restrict__ fb, float* __restrict__ sums,
                                                                uint32_t* __restrict__ s1, unsigned long long* __restrict__ s2,
                                                                long long per_fb, int nfb) {
  accum_add_body<VEC, true>(fb, sums, s1, s2, per_fb, nfb);
}

// The noise of the n frame buffers a monitor has seen (definitions in include/rt_hip.h).  One
// 256-lane workgroup per tile of 16 x 16 pixels over (owned-row index, column), one lane per pixel;
// a wave holds 4 tile rows of 16 pixels.  Per pixel, over its channels j, in unsigned 64-bit
// integers (n <= 32768: n S2 and S1^2 <= 4.6e18 each, the three-channel sum <= 1.4e19 < 2^64; every
// term n S2 - S1^2 >= 0 by Cauchy-Schwarz):  D = sum_j (n S2_j - S1_j^2),  S = sum_j S1_j;  then in
// double, in this order:  a = D / (3.0 n n (n - 1) 4228250625.0),  m = max(S / (3.0 n 65025.0), 2^-16),
// noise = float(128.0 sqrt(a / m)) >= 0.  Lanes outside a partial tile hold noise 0 and are not
// counted.  Outputs: map[row][col] (may be null); per tile the maximum (shuffles within the wave, LDS
// across the four) and the count of pixels with noise > threshold (ballot + popcount).  The image-wide
// maximum and count come from the tile arrays in noise_reduce_kernel (one atomic per tile on one
// address serialises: 32 400 tiles at 3840 x 2159 took longer than reading the moments).  No float is
// summed anywhere: every output is independent of the order of reduction.
// (the per-pixel formula and the tile reduction are functions of their own: the adaptive accumulator's
// adapt_measure_kernel runs the same device code with a per-tile n)
__device__ __forceinline__ float pixel_noise(const uint32_t* __restrict__ s1, const unsigned long long* __restrict__ s2,
                                             long long px, int n) {
  unsigned long long D = 0, S = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const unsigned long long m1 = s1[3 * px + j], m2 = s2[3 * px + j];
    D += (unsigned long long)n * m2 - m1 * m1;
    S += m1;
  }
  const double dn = (double)n, dn1 = (double)(n - 1);
  const double a = (double)D / (3.0 * dn * dn * dn1 * 4228250625.0);
  double m = (double)S / (3.0 * dn * 65025.0);
  if (m < 0x1p-16) m = 0x1p-16;
  return (float)(128.0 * __builtin_sqrt(a / m));
}
// A 256-lane workgroup's maximum of noise and count of lanes with noise > threshold, into tile_max[tile]
// and tile_above[tile] (wave_max, wave_above: 4 LDS words each).
__device__ __forceinline__ void noise_tile_reduce(bool valid, float noise, float threshold, float* wave_max, int* wave_above,
                                                  int tile, float* __restrict__ tile_max, int32_t* __restrict__ tile_above) {
  const int lane = threadIdx.x;
  const unsigned long long hot = __ballot(valid && noise > threshold);
  float mx = noise;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  const int wave = lane >> 6;
  if ((lane & 63) == 0) {
    wave_max[wave] = mx;
    wave_above[wave] = __popcll(hot);
  }
  __syncthreads();
  if (lane == 0) {
    const float t = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
    const int cnt = wave_above[0] + wave_above[1] + wave_above[2] + wave_above[3];
    tile_max[tile] = t;
    tile_above[tile] = cnt;
  }
}
__global__ __launch_bounds__(256) void noise_measure_kernel(const uint32_t* __restrict__ s1,
                                                            const unsigned long long* __restrict__ s2, int n, int rows,
                                                            int width, float threshold, float* __restrict__ map,
                                                            float* __restrict__ tile_max, int32_t* __restrict__ tile_above) {
  __shared__ float wave_max[4];
  __shared__ int wave_above[4];
  const int lane = threadIdx.x;
  const int col = blockIdx.x * 16 + (lane & 15), row = blockIdx.y * 16 + (lane >> 4);
  const bool valid = col < width && row < rows;
  float noise = 0.0f;
  if (valid) {
    const long long px = (long long)row * width + col;
    noise = pixel_noise(s1, s2, px, n);
    if (map) map[px] = noise;
  }
  noise_tile_reduce(valid, noise, threshold, wave_max, wave_above, blockIdx.y * gridDim.x + blockIdx.x, tile_max,
                    tile_above);
}

// Image-wide maximum (as the bit pattern of the non-negative float, in the low word of totals[1]) and
// count (totals[0]) from noise_measure_kernel's tile arrays: one 256-lane workgroup strides over the
// tiles; a maximum and an integer sum, so the order does not matter.
__global__ __launch_bounds__(256) void noise_reduce_kernel(const float* __restrict__ tile_max,
                                                           const int32_t* __restrict__ tile_above, int tiles,
                                                           unsigned long long* __restrict__ totals) {
  __shared__ float wave_max[4];
  __shared__ unsigned long long wave_above[4];
  const int lane = threadIdx.x;
  float mx = 0.0f;
  unsigned long long cnt = 0;
  for (int t = lane; t < tiles; t += 256) {
    mx = fmaxf(mx, tile_max[t]);
    cnt += (unsigned long long)tile_above[t];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, d));
    cnt += __shfl_xor(cnt, d);
  }
  if ((lane & 63) == 0) {
    wave_max[lane >> 6] = mx;
    wave_above[lane >> 6] = cnt;
  }
  __syncthreads();
  if (lane == 0) {
    totals[0] = wave_above[0] + wave_above[1] + wave_above[2] + wave_above[3];
    totals[1] = __float_as_uint(fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3])));
  }
}

// The image of the nfb frame buffers folded into sums: resolve_kernel's last line.  VEC (sums 16-byte,
// out 4-byte aligned): 4 sums in, 4 bytes out per lane.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void accum_image_kernel(const float* __restrict__ sums, uint8_t* __restrict__ out,
                                                            long long n, int nfb) {
  const long long k0 = 4 * ((long long)blockIdx.x * kBlock + threadIdx.x);
  if (k0 >= n) return;
  const float d = (float)nfb;
  if (VEC && k0 + 4 <= n) {
    const float4 a = *reinterpret_cast<const float4*>(sums + k0);
    const uint32_t q = (uint32_t)quant(a.x / d) | (uint32_t)quant(a.y / d) << 8 | (uint32_t)quant(a.z / d) << 16 |
                       (uint32_t)quant(a.w / d) << 24;
    *reinterpret_cast<uint32_t*>(out + k0) = q;
    return;
  }
  const long long k1 = k0 + 4 < n ? k0 + 4 : n;
  for (long long k = k0; k < k1; ++k) out[k] = (uint8_t)quant(sums[k] / d);
}

// ---- launches over a set of noise tiles (rt_render_tiles) and the adaptive accumulator (rt_adapt)
// "Noise tile" here is always the noise monitor's tile of 16 x 16 pixels over (owned-row index, column)
// (rtacc::kNoiseTile), never the 8 x 8 camera-ray tile of kTileShift.
//
// The item list of a launch over the listed noise tiles: RenderParams::perm for the render kernels, which
// decode item = q * fb_count * W + f * W + i (row position q, frame buffer f, column i).  One 256-lane
// workgroup per listed tile, one lane per pixel; ntile[k] = {tile id, base, row stride, fb stride}: pixel
// (ly, lx) of the tile in frame buffer f goes to position base + ly * row stride + f * fb stride + lx.  The
// host (rttile::records) chooses the strides -- tile-major, a tile's pixels of one fb in adjacent claims --
// and guarantees that the positions are a permutation of 0 .. n_items - 1.
__global__ __launch_bounds__(256) void tile_items_kernel(const uint4* __restrict__ ntile, int tiles_x, int rows, int width,
                                                         int fb_count, uint32_t* __restrict__ perm) {
  const uint4 d = ntile[blockIdx.x];
  const int lane = threadIdx.x, lx = lane & 15, ly = lane >> 4;
  const int col = (int)(d.x % (unsigned)tiles_x) * 16 + lx, row = (int)(d.x / (unsigned)tiles_x) * 16 + ly;
  if (col >= width || row >= rows) return;
  const unsigned long long first = (unsigned long long)row * fb_count * width + col;
  const unsigned long long pos = (unsigned long long)d.y + (unsigned long long)ly * d.z + lx;
  for (int f = 0; f < fb_count; ++f) perm[pos + (unsigned long long)f * d.w] = (uint32_t)(first + (unsigned long long)f * width);
}

// rt_adapt: the nfb frame buffers at fb folded into the listed (active) noise tiles' values: the float sum
// by accum_add_kernel's operations in its order, S1 and S2 as accum_add_stats_kernel keeps them.  One
// workgroup per listed tile: the traffic is the active tiles', not the image's.  A tile row is 16 pixels =
// 48 consecutive values; the 256 lanes take the tile's 768 values in three passes, consecutive lanes on
// consecutive values of a row (one lane per pixel, three values 12 bytes apart, measured 127.7 us at
// 1200 x 800 x 10 fb against this layout's 48.6 us).
__global__ __launch_bounds__(256) void adapt_fold_kernel(const uint4* __restrict__ ntile, int tiles_x, int rows, int width,
                                                         const float* __restrict__ fb, long long per_fb, int nfb,
                                                         float* __restrict__ sums, uint32_t* __restrict__ s1,
                                                         unsigned long long* __restrict__ s2) {
  const unsigned id = ntile[blockIdx.x].x;
  const int row0 = (int)(id / (unsigned)tiles_x) * 16, v0 = (int)(id % (unsigned)tiles_x) * 48;  // first row, first value of a row
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    const int v = pass * 256 + (int)threadIdx.x;
    const int row = row0 + v / 48, vx = v0 + v % 48;
    if (row >= rows || vx >= 3 * width) continue;
    const long long k = (long long)row * width * 3 + vx;
    float a = sums[k];
    uint32_t m1 = s1[k];
    unsigned long long m2 = s2[k];
    for (int f = 0; f < nfb; ++f) fold1<true>(fb[(long long)f * per_fb + k], a, m1, m2);
    sums[k] = a;
    s1[k] = m1;
    s2[k] = m2;
  }
}

// rt_adapt: noise_measure_kernel over listed noise tiles (list null: over every tile, tile = blockIdx.x),
// each with its own n = tile_n[tile] >= 2; same per-pixel code, same tile reduction.
__global__ __launch_bounds__(256) void adapt_measure_kernel(const uint4* __restrict__ ntile, const int32_t* __restrict__ tile_n,
                                                            const uint32_t* __restrict__ s1,
                                                            const unsigned long long* __restrict__ s2, int tiles_x, int rows,
                                                            int width, float threshold, float* __restrict__ map,
                                                            float* __restrict__ tile_max, int32_t* __restrict__ tile_above) {
  __shared__ float wave_max[4];
  __shared__ int wave_above[4];
  const int tile = ntile ? (int)ntile[blockIdx.x].x : (int)blockIdx.x;
  const int lane = threadIdx.x;
  const int col = (tile % tiles_x) * 16 + (lane & 15), row = (tile / tiles_x) * 16 + (lane >> 4);
  const bool valid = col < width && row < rows;
  float noise = 0.0f;
  if (valid) {
    const long long px = (long long)row * width + col;
    noise = pixel_noise(s1, s2, px, tile_n[tile]);
    if (map) map[px] = noise;
  }
  noise_tile_reduce(valid, noise, threshold, wave_max, wave_above, tile, tile_max, tile_above);
}

// rt_adapt: accum_image_kernel with the divisor of the pixel's noise tile, out = quant(sum / n_t); one lane
// per pixel.
__global__ __launch_bounds__(kBlock) void adapt_image_kernel(const float* __restrict__ sums, const int32_t* __restrict__ tile_n,
                                                            int tiles_x, int rows, int width, uint8_t* __restrict__ out) {
  const long long px = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (px >= (long long)rows * width) return;
  const int row = (int)(px / width), col = (int)(px - (long long)row * width);
  const float d = (float)tile_n[(row >> 4) * tiles_x + (col >> 4)];
#pragma unroll
  for (int j = 0; j < 3; ++j) out[3 * px + j] = (uint8_t)quant(sums[3 * px + j] / d);
}

// ====================================================================== host side: shared plumbing
using namespace rtctx;

bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
hipStream_t stream_of(const rt_ctx* c) { return view(c).stream; }

// The device time between two points of a stream.
class Timer {
 public:
  Timer() = default;
  Timer(const Timer&) = delete;
  Timer& operator=(const Timer&) = delete;
  ~Timer() {
    for (hipEvent_t e : ev_)
      if (e) (void)hipEventDestroy(e);
  }
  bool create() { return hipEventCreate(&ev_[0]) == hipSuccess && hipEventCreate(&ev_[1]) == hipSuccess; }
  hipError_t start(hipStream_t stream) { return hipEventRecord(ev_[0], stream); }
  hipError_t stop(hipStream_t stream) {
    const hipError_t e = hipEventRecord(ev_[1], stream);
    if (e == hipSuccess) recorded_ = true;
    return e;
  }
  // 0 until a start / stop pair has been recorded
  float ms() const {
    float ms = 0.0f;
    if (!recorded_ || hipEventElapsedTime(&ms, ev_[0], ev_[1]) != hipSuccess) return 0.0f;
    return ms;
  }

 private:
  hipEvent_t ev_[2] = {nullptr, nullptr};
  bool recorded_ = false;
};

// The noise tiles of rows x width pixels: 16 x 16 pixels over (owned-row index, column), id = ty * tiles_x + tx.
static_assert(rttile::kTile == rtacc::kNoiseTile, "tile launches use the noise monitor's tiles");
struct TileGrid {
  int rows = 0, width = 0, tiles_x = 0, tiles_y = 0;
  TileGrid() = default;
  TileGrid(int rows_, int width_)
      : rows(rows_), width(width_), tiles_x((int)(((long long)width_ + rtacc::kNoiseTile - 1) / rtacc::kNoiseTile)),
        tiles_y((int)(((long long)rows_ + rtacc::kNoiseTile - 1) / rtacc::kNoiseTile)) {}
  long long count() const { return (long long)tiles_x * tiles_y; }
  long long pixels() const { return (long long)rows * width; }
  bool ids_fit() const { return count() <= INT32_MAX; }                  // a tile id is an int32
  bool launch_2d_fits() const { return tiles_y <= 65535 && ids_fit(); }  // tiles_y as gridDim.y
  void size(int id, int& tw, int& th) const { rttile::size(id, tiles_x, rows, width, tw, th); }
};

// The integer moments of c^2 per accumulator value and the per-tile outputs of a measure over them: what
// rt_noise and rt_adapt both keep.
struct Moments {
  TileGrid grid;
  DevBuf<uint32_t> s1;            // [pixels x 3] sum of c^2
  DevBuf<unsigned long long> s2;  // [pixels x 3] sum of c^4
  DevBuf<float> tile_max;         // [tiles] measure outputs: maxima, counts
  DevBuf<int32_t> tile_above;
  bool alloc(const TileGrid& g) {
    grid = g;
    const size_t nv = (size_t)g.pixels() * 3, tiles = (size_t)g.count();
    return s1.alloc(nv) && s2.alloc(nv) && tile_max.alloc(tiles) && tile_above.alloc(tiles);
  }
  bool clear(hipStream_t stream) { return s1.clear(stream) && s2.clear(stream); }  // every moment 0
};

// What rt_accum and rt_adapt are both made of: draw() cut after any frame buffer -- the float sums of
// average_images (color.h:57-170) stay on the device between calls, the frame buffers of one chunk at a
// time go through `scratch`.
struct AccumCore {
  rt_ctx* ctx = nullptr;
  rt_render_args args{};  // fb_count = frame buffers folded in (rt_adapt: rendered for the tiles still active, max n_t)
  int32_t chunk = 1;
  long long per_fb = 0;  // owned_rows x width x 3
  long long scene_gen = 0;
  DevBuf<float> sums;     // [per_fb]
  DevBuf<float> scratch;  // [chunk][per_fb], allocated by the first add
  DevBuf<uint8_t> img;    // [per_fb], allocated by the first image into host memory
  Timer add_timer;        // around the last fold launch
};

// What rt_accum_create and rt_adapt_create check alike, in this order, after their own null checks and
// before their own limits; *rows: the rows a's tiling owns.
int create_check(rt_ctx* c, const rt_render_args* a, int32_t chunk_fbs, int* rows) {
  if (!a) return fail(c, RT_ERR_ARG, "null args");
  rt_render_args one = *a;
  one.fb_count = 1;
  const int rc = validate_args(c, &one);
  if (rc) return rc;
  if (chunk_fbs < 1) return fail(c, RT_ERR_ARG, "chunk_fbs < 1");
  if (a->fb_first > INT32_MAX - chunk_fbs) return fail(c, RT_ERR_ARG, "fb range overflows");
  *rows = rt_owned_rows(a, nullptr);
  if (*rows <= 0) return fail(c, RT_ERR_ARG, "no rows owned");
  return RT_OK;
}
void core_init(AccumCore& k, rt_ctx* c, const rt_render_args* a, int32_t chunk_fbs, int rows) {
  k.ctx = c;
  k.args = *a;
  k.args.fb_count = 0;
  k.chunk = chunk_fbs;
  k.per_fb = (long long)rows * a->width * 3;
  k.scene_gen = view(c).scene_gen;
}

// A fold of count further frame buffers, checked before anything is rendered or written; room: how many
// the noise moments folded with them still take (rtacc::kNoiseMaxFbs in all; INT32_MAX without moments).
int fold_check(const AccumCore& k, int32_t count, int32_t room) {
  rt_ctx* c = k.ctx;
  if (count < 1) return fail(c, RT_ERR_ARG, "count < 1");
  if (count > INT32_MAX - k.args.fb_first - k.args.fb_count) return fail(c, RT_ERR_ARG, "fb range overflows");
  if (count > room) return fail(c, RT_ERR_ARG, "noise monitor: more than 32768 frame buffers");
  return RT_OK;
}
// ... that are to be rendered: the scene must be the one of creation.
int add_check(const AccumCore& k, int32_t count, int32_t room) {
  const int rc = fold_check(k, count, room);
  if (rc) return rc;
  if (k.scene_gen != view(k.ctx).scene_gen)
    return fail(k.ctx, RT_ERR_STATE, "scene uploaded again since the accumulator was created");
  return RT_OK;
}

void add_counters(rt_counters& t, const rt_counters& x) {
  t.segments += x.segments;
  t.node_tests += x.node_tests;
  t.prim_tests += x.prim_tests;
  t.samples += x.samples;
  t.fallbacks += x.fallbacks;
}

// count frame buffers from k's next one on, at most k.chunk at a time: step(r, n, &cnt) renders the n frame
// buffers of r into k.scratch and folds them, which moves k.args.fb_count on by n; all queued on the
// context's stream in order.  total: the steps' counters, summed.
template <class Step>
int add_chunks(AccumCore& k, int32_t count, rt_counters& total, Step step) {
  for (int32_t left = count; left > 0;) {
    const int32_t n = std::min(left, k.chunk);
    rt_render_args r = k.args;
    r.fb_first = k.args.fb_first + k.args.fb_count;
    r.fb_count = n;
    rt_counters cnt = {};
    const int rc = step(r, n, &cnt);
    if (rc) return rc;
    add_counters(total, cnt);
    left -= n;
  }
  return RT_OK;
}

// rt_accum_image and rt_adapt_image: the checks; the image in device memory -- out itself, or for a host
// out k.img, allocated on first use (nomem: that failure's text); launch(img) queues the kernel that writes
// it; then the wait, for a host out after the copy, rows flipped for png_order.
template <class Launch>
int image_out(AccumCore& k, uint8_t* out, int32_t png_order, const char* nomem, Launch launch) {
  rt_ctx* c = k.ctx;
  if (!out) return fail(c, RT_ERR_ARG, "null image");
  if (png_order != 0 && png_order != 1) return fail(c, RT_ERR_ARG, "bad png_order");
  const rt_render_args& a = k.args;
  const View v = view(c);
  HIPCHK(c, hipSetDevice(v.device));
  const bool out_dev = device_ptr(out);
  if (png_order && k.per_fb != (long long)a.width * a.height * 3)
    return fail(c, RT_ERR_ARG, "png_order needs the whole-image tiling");
  if (png_order && out_dev) return fail(c, RT_ERR_ARG, "png_order needs a host image");
  if (a.fb_count < 1) return fail(c, RT_ERR_STATE, "no frame buffer accumulated yet");
  if (!out_dev && !k.img && !k.img.alloc((size_t)k.per_fb)) return fail(c, RT_ERR_NOMEM, nomem);
  uint8_t* img = out_dev ? out : k.img.get();
  const int rc = launch(img);
  if (rc) return rc;
  std::vector<uint8_t> tmp(png_order ? (size_t)k.per_fb : 0);
  if (!out_dev) HIPCHK(c, hipMemcpyAsync(png_order ? tmp.data() : out, img, (size_t)k.per_fb, hipMemcpyDeviceToHost, v.stream));
  HIPCHK(c, hipStreamSynchronize(v.stream));
  const size_t row = (size_t)a.width * 3;
  if (png_order)
    for (int j = 0; j < a.height; ++j) memcpy(out + (size_t)(a.height - 1 - j) * row, tmp.data() + j * row, row);
  return RT_OK;
}

// rt_denoise_monitor and rt_denoise_adaptive: the checks (every one before anything is written), then
// rt_denoise.hip's prepare pass and filter over the moments m -- every pixel at n frame buffers, or with
// tile_n_dev at its noise tile's -- into image_out's image, and the gain beside it under the same conventions.
// The (M, V) scratch lives for the call only.
int denoise_out(AccumCore& k, const Moments& m, const int32_t* tile_n_dev, int n, Timer& timer, const rt_denoise_params* params,
                uint8_t* out, float* gain, int32_t png_order, const rtdn::GuideView* guide = nullptr) {
  rt_ctx* c = k.ctx;
  rt_denoise_params p;
  if (params) p = *params;
  else rt_denoise_params_default(&p);
  if (!rtdn::params_ok(&p)) return fail(c, RT_ERR_ARG, "denoise: parameters out of range");
  if (k.per_fb != (long long)k.args.width * k.args.height * 3) return fail(c, RT_ERR_ARG, "denoise needs the whole-image tiling");
  if (!m.grid.launch_2d_fits()) return fail(c, RT_ERR_ARG, "denoise: too many tiles");
  HIPCHK(c, hipSetDevice(view(c).device));
  if (gain && png_order == 1 && device_ptr(gain)) return fail(c, RT_ERR_ARG, "png_order needs a host gain");
  const size_t pixels = (size_t)m.grid.pixels();
  DevBuf<float2> mv;
  DevBuf<float> gain_tmp;  // a host gain is staged through device memory
  std::vector<float> gain_rows;
  const bool gain_host = gain && !device_ptr(gain);
  const int rc = image_out(k, out, png_order, "hipMalloc denoised image", [&](uint8_t* img) {
    const hipStream_t stream = stream_of(c);
    if (!mv.alloc(pixels * 3) || (gain_host && !gain_tmp.alloc(pixels))) return fail(c, RT_ERR_NOMEM, "hipMalloc denoise scratch");
    float* gain_dev = gain_host ? gain_tmp.get() : gain;
    HIPCHK(c, timer.start(stream));
    HIPCHK(c, rtdn::launch(stream, m.s1.get(), m.s2.get(), tile_n_dev, n, m.grid.rows, m.grid.width, p, mv.get(), img, gain_dev, guide));
    HIPCHK(c, timer.stop(stream));
    if (gain_host) {
      if (png_order) gain_rows.resize(pixels);
      HIPCHK(c, hipMemcpyAsync(png_order ? gain_rows.data() : gain, gain_dev, pixels * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    return (int)RT_OK;
  });
  if (hipStreamSynchronize(stream_of(c)) != hipSuccess && !rc) return fail(c, RT_ERR_HIP, "denoise kernels");  // before mv is freed
  if (rc) return rc;
  if (gain_host && png_order) {
    const size_t w = (size_t)m.grid.width, h = (size_t)m.grid.rows;
    for (size_t j = 0; j < h; ++j) memcpy(gain + (h - 1 - j) * w, gain_rows.data() + j * w, w * sizeof(float));
  }
  return RT_OK;
}

// rt_guide_denoise_monitor and rt_guide_denoise_adaptive: the guide's planes as the filter's view of them, after
// the checks that are the guided call's own -- the gains, then that g has rendered planes of k's image size, on
// k's device, of the scene with fingerprint scene_fp.
int guide_view(AccumCore& k, uint64_t scene_fp, const rt_guide* g, const rt_guide_params* gparams, rtdn::GuideView* gv) {
  rt_ctx* c = k.ctx;
  if (gparams) gv->gains = *gparams;
  else rt_guide_params_default(&gv->gains);
  if (!rtdn::guide_params_ok(&gv->gains)) return fail(c, RT_ERR_ARG, "guided denoise: gains out of range");
  const rtguide::View v = rtguide::view(g);
  if (!v.width) return fail(c, RT_ERR_STATE, "guided denoise: the guide has rendered no planes");
  if (v.width != k.args.width || v.height != k.args.height) return fail(c, RT_ERR_STATE, "guided denoise: the guide's planes have another size");
  if (v.scene_fp != scene_fp) return fail(c, RT_ERR_STATE, "guided denoise: the guide belongs to another scene");
  if (v.device != view(c).device) return fail(c, RT_ERR_STATE, "guided denoise: the guide lives on another device");
  gv->normal = v.normal, gv->albedo = v.albedo, gv->depth = v.depth;
  return RT_OK;
}

}  // namespace

// ---------------------------------------------------------------------- progressive accumulator
struct RT_INTERNAL rt_accum : AccumCore {
  uint64_t scene_fp = 0;
  Timer image_timer;          // around the last image launch
  rt_noise* noise = nullptr;  // the attached monitor (not owned: rt_noise_destroy frees it)
};

// Noise monitor of an accumulator (include/rt_hip.h): the integer moments of c^2 per accumulator value.
struct RT_INTERNAL rt_noise {
  rt_accum* acc = nullptr;  // null once the accumulator is destroyed (detached: calls are RT_ERR_STATE)
  int device = 0;
  int32_t fbs = 0;  // frame buffers folded in, at most rtacc::kNoiseMaxFbs
  Moments m;
  DevBuf<unsigned long long> totals;  // totals[0] = pixels above (image-wide), low word of totals[1] = max bits
  Timer timer;                        // around the last measure and its reduction
  Timer denoise_timer;                // around the last denoise's kernels
};

namespace {

// Frame buffers acc's monitor still takes (fold_check's room).
int32_t noise_room(const rt_accum* acc) { return acc->noise ? rtacc::kNoiseMaxFbs - acc->noise->fbs : INT32_MAX; }

// sums += the count frame buffers at fb_dev (fold_check passed), queued on the context's stream.
int accum_fold(rt_accum* acc, const float* fb_dev, int count) {
  rt_ctx* c = acc->ctx;
  const hipStream_t stream = stream_of(c);
  const long long per_fb = acc->per_fb;
  const unsigned blocks = (unsigned)(((per_fb + 3) / 4 + kBlock - 1) / kBlock);
  rt_noise* nm = acc->noise;
  float* sums = acc->sums.get();
  uint32_t* s1 = nm ? nm->m.s1.get() : nullptr;
  unsigned long long* s2 = nm ? nm->m.s2.get() : nullptr;
  HIPCHK(c, acc->add_timer.start(stream));
  const bool vec = per_fb % 4 == 0 && aligned_to(fb_dev, 16) && aligned_to(sums, 16);
  if (nm && vec && aligned_to(s1, 16) && aligned_to(s2, 16))
    hipLaunchKernelGGL(accum_add_stats_kernel<true>, dim3(blocks), dim3(kBlock), 0, stream, fb_dev, sums, s1, s2, per_fb, count);
  else if (nm)
    hipLaunchKernelGGL(accum_add_stats_kernel<false>, dim3(blocks), dim3(kBlock), 0, stream, fb_dev, sums, s1, s2, per_fb, count);
  else if (vec)
    hipLaunchKernelGGL(accum_add_kernel<true>, dim3(blocks), dim3(kBlock), 0, stream, fb_dev, sums, per_fb, count);
  else
    hipLaunchKernelGGL(accum_add_kernel<false>, dim3(blocks), dim3(kBlock), 0, stream, fb_dev, sums, per_fb, count);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, acc->add_timer.stop(stream));
  acc->args.fb_count += count;
  if (nm) nm->fbs += count;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_accum_create(rt_ctx* c, const rt_render_args* a, int32_t chunk_fbs, rt_accum** out) {
  if (!c) return RT_ERR_ARG;
  if (!out) return fail(c, RT_ERR_ARG, "null accumulator pointer");
  *out = nullptr;
  int rows = 0;
  const int rc = create_check(c, a, chunk_fbs, &rows);
  if (rc) return rc;
  const View v = view(c);
  if (!v.have_scene) return fail(c, RT_ERR_STATE, "no scene uploaded");
  HIPCHK(c, hipSetDevice(v.device));
  std::unique_ptr<rt_accum> acc(new rt_accum);
  core_init(*acc, c, a, chunk_fbs, rows);
  acc->scene_fp = v.scene_fp;
  if (!acc->add_timer.create() || !acc->image_timer.create()) return fail(c, RT_ERR_HIP, "hipEventCreate");
  if (!acc->sums.alloc((size_t)acc->per_fb)) return fail(c, RT_ERR_NOMEM, "hipMalloc accumulator sums");
  if (!acc->sums.clear(v.stream)) return fail(c, RT_ERR_HIP, "clear accumulator sums");
  *out = acc.release();
  return RT_OK;
}

int rt_accum_destroy(rt_accum* acc) {
  if (!acc) return RT_ERR_ARG;
  const View v = view(acc->ctx);
  (void)hipSetDevice(v.device);
  (void)hipStreamSynchronize(v.stream);
  if (acc->noise) acc->noise->acc = nullptr;  // detached: the monitor's calls fail from here on
  delete acc;
  return RT_OK;
}

int rt_accum_add(rt_accum* acc, int32_t count, rt_counters* counters) {
  if (!acc) return RT_ERR_ARG;
  rt_ctx* c = acc->ctx;
  int rc = add_check(*acc, count, noise_room(acc));
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(view(c).device));
  if ((rc = ensure_states(c, acc->args.width, acc->args.height, acc->args.seed))) return rc;
  if (!acc->scratch && !acc->scratch.alloc((size_t)acc->chunk * acc->per_fb))
    return fail(c, RT_ERR_NOMEM, "hipMalloc accumulator frame buffers");
  rt_counters total = {};
  rc = add_chunks(*acc, count, total, [&](const rt_render_args& r, int32_t n, rt_counters* cnt) {
    const int e = rt_render(c, &r, acc->scratch.get(), cnt);
    return e ? e : accum_fold(acc, acc->scratch.get(), n);  // ordered before the next chunk's render on the stream
  });
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(stream_of(c)));
  if (counters) *counters = total;
  return RT_OK;
}

int rt_accum_add_fbs(rt_accum* acc, const float* fb, int32_t count) {
  if (!acc) return RT_ERR_ARG;
  rt_ctx* c = acc->ctx;
  if (!fb) return fail(c, RT_ERR_ARG, "null fb");
  int rc = fold_check(*acc, count, noise_room(acc));
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(view(c).device));
  const Staged<float> st(fb, (size_t)count * acc->per_fb);  // a host frame buffer is staged through device memory, as rt_resolve does
  if (!st.ok()) return fail(c, RT_ERR_NOMEM, "hipMalloc frame buffer staging");
  if (st.host() && hipMemcpy(st.dev(), fb, st.bytes(), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(c, RT_ERR_HIP, "copy frame buffer to device");
  if (!rc) rc = accum_fold(acc, st.dev(), count);
  if (hipStreamSynchronize(stream_of(c)) != hipSuccess && !rc) rc = fail(c, RT_ERR_HIP, "accumulate kernel");
  return rc;
}

int rt_accum_image(rt_accum* acc, uint8_t* out, int32_t png_order) {
  if (!acc) return RT_ERR_ARG;
  return image_out(*acc, out, png_order, "hipMalloc accumulator image", [&](uint8_t* img) {
    rt_ctx* c = acc->ctx;
    const hipStream_t stream = stream_of(c);
    const float* sums = acc->sums.get();
    const unsigned blocks = (unsigned)(((acc->per_fb + 3) / 4 + kBlock - 1) / kBlock);
    HIPCHK(c, acc->image_timer.start(stream));
    if (aligned_to(sums, 16) && aligned_to(img, 4))
      hipLaunchKernelGGL(accum_image_kernel<true>, dim3(blocks), dim3(kBlock), 0, stream, sums, img, acc->per_fb, acc->args.fb_count);
    else
      hipLaunchKernelGGL(accum_image_kernel<false>, dim3(blocks), dim3(kBlock), 0, stream, sums, img, acc->per_fb, acc->args.fb_count);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, acc->image_timer.stop(stream));
    return (int)RT_OK;
  });
}

int rt_accum_get_info(const rt_accum* acc, rt_accum_info* info) {
  if (!acc) return RT_ERR_ARG;
  if (!info) return fail(acc->ctx, RT_ERR_ARG, "null info");
  info->args = acc->args;
  info->n_values = acc->per_fb;
  info->scene_fp = acc->scene_fp;
  return RT_OK;
}

float rt_accum_last_add_ms(const rt_accum* acc) { return acc ? acc->add_timer.ms() : 0.0f; }
float rt_accum_last_image_ms(const rt_accum* acc) { return acc ? acc->image_timer.ms() : 0.0f; }

int rt_accum_save(rt_accum* acc, void* blob, size_t cap, size_t* need) {
  if (!acc) return RT_ERR_ARG;
  rt_ctx* c = acc->ctx;
  const size_t total = rtacc::kHeaderBytes + acc->sums.bytes();
  if (need) *need = total;
  if (!blob && cap == 0) return RT_OK;  // size query
  if (!blob || cap < total) return fail(c, RT_ERR_ARG, "checkpoint buffer too small");
  const View v = view(c);
  HIPCHK(c, hipSetDevice(v.device));
  // the sums land in the blob's payload, then the header is packed around them
  float* payload = reinterpret_cast<float*>(static_cast<unsigned char*>(blob) + rtacc::kHeaderBytes);
  HIPCHK(c, hipMemcpyAsync(payload, acc->sums.get(), acc->sums.bytes(), hipMemcpyDeviceToHost, v.stream));
  HIPCHK(c, hipStreamSynchronize(v.stream));
  rt_accum_info info;
  rt_accum_get_info(acc, &info);
  if (rt_accum_blob_pack(&info, payload, blob, cap, nullptr)) return fail(c, RT_ERR_ARG, "pack checkpoint");
  return RT_OK;
}

int rt_accum_load(rt_ctx* c, const void* blob, size_t n, int32_t chunk_fbs, rt_accum** out) {
  if (!c) return RT_ERR_ARG;
  if (!out) return fail(c, RT_ERR_ARG, "null accumulator pointer");
  *out = nullptr;
  rt_accum_info info;
  if (rt_accum_blob_info(blob, n, &info)) return fail(c, RT_ERR_ARG, "malformed checkpoint");
  const View v = view(c);
  if (!v.have_scene) return fail(c, RT_ERR_STATE, "no scene uploaded");
  if (info.scene_fp != v.scene_fp) return fail(c, RT_ERR_STATE, "checkpoint belongs to another scene");
  if (info.args.fb_first > INT32_MAX - info.args.fb_count) return fail(c, RT_ERR_ARG, "malformed checkpoint");
  rt_accum* acc = nullptr;
  int rc = rt_accum_create(c, &info.args, chunk_fbs, &acc);
  if (rc) return rc;
  if (acc->per_fb != info.n_values) rc = fail(c, RT_ERR_ARG, "malformed checkpoint");
  const unsigned char* payload = static_cast<const unsigned char*>(blob) + rtacc::kHeaderBytes;
  if (!rc && (hipMemcpyAsync(acc->sums.get(), payload, acc->sums.bytes(), hipMemcpyHostToDevice, v.stream) != hipSuccess ||
              hipStreamSynchronize(v.stream) != hipSuccess))
    rc = fail(c, RT_ERR_HIP, "copy checkpoint sums to device");
  if (rc) {
    rt_accum_destroy(acc);
    return rc;
  }
  acc->args.fb_count = info.args.fb_count;
  *out = acc;
  return RT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------- noise monitor
namespace {

// A monitor attached to acc with every moment 0 (queued on the context's stream).
int noise_new(rt_accum* acc, rt_noise** out) {
  rt_ctx* c = acc->ctx;
  const TileGrid g((int)(acc->per_fb / (3LL * acc->args.width)), acc->args.width);
  if (!g.launch_2d_fits()) return fail(c, RT_ERR_ARG, "noise monitor: too many tiles");
  const View v = view(c);
  HIPCHK(c, hipSetDevice(v.device));
  std::unique_ptr<rt_noise> nm(new rt_noise);
  nm->device = v.device;
  if (!nm->m.alloc(g) || !nm->totals.alloc(2)) return fail(c, RT_ERR_NOMEM, "hipMalloc noise monitor");
  if (!nm->timer.create() || !nm->denoise_timer.create() || !nm->m.clear(v.stream)) return fail(c, RT_ERR_HIP, "set up noise monitor");
  nm->acc = acc;
  acc->noise = *out = nm.release();
  return RT_OK;
}

// noise_measure_kernel over the whole monitor, then the reduction of its tile arrays, queued on the
// context's stream; map_dev may be null.
int noise_run(rt_noise* nm, float threshold, float* map_dev) {
  rt_ctx* c = nm->acc->ctx;
  const hipStream_t stream = stream_of(c);
  const Moments& m = nm->m;
  HIPCHK(c, nm->timer.start(stream));
  hipLaunchKernelGGL(noise_measure_kernel, dim3(m.grid.tiles_x, m.grid.tiles_y), dim3(256), 0, stream, m.s1.get(), m.s2.get(),
                     nm->fbs, m.grid.rows, m.grid.width, threshold, map_dev, m.tile_max.get(), m.tile_above.get());
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(noise_reduce_kernel, dim3(1), dim3(256), 0, stream, m.tile_max.get(), m.tile_above.get(),
                     (int)m.grid.count(), nm->totals.get());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, nm->timer.stop(stream));
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_noise_create(rt_accum* acc, rt_noise** out) {
  if (!acc) return RT_ERR_ARG;
  rt_ctx* c = acc->ctx;
  if (!out) return fail(c, RT_ERR_ARG, "null monitor pointer");
  *out = nullptr;
  if (acc->noise) return fail(c, RT_ERR_STATE, "the accumulator has a noise monitor already");
  if (acc->args.fb_count != 0) return fail(c, RT_ERR_STATE, "a noise monitor sees every frame buffer or none: the accumulator is not empty");
  return noise_new(acc, out);
}

int rt_noise_destroy(rt_noise* nm) {
  if (!nm) return RT_ERR_ARG;
  (void)hipSetDevice(nm->device);
  if (nm->acc) {
    (void)hipStreamSynchronize(stream_of(nm->acc->ctx));
    nm->acc->noise = nullptr;  // the accumulator goes on with accum_add_kernel
  }
  delete nm;
  return RT_OK;
}

int rt_noise_measure(rt_noise* nm, float threshold, rt_noise_report* rep, float* tile_max, int32_t* tile_above) {
  if (!nm) return RT_ERR_ARG;
  if (!nm->acc) return RT_ERR_STATE;  // detached
  rt_ctx* c = nm->acc->ctx;
  if (nm->fbs < 2) return fail(c, RT_ERR_STATE, "noise needs at least 2 frame buffers");
  const View v = view(c);
  HIPCHK(c, hipSetDevice(v.device));
  const int rc = noise_run(nm, threshold, nullptr);
  if (rc) return rc;
  const Moments& m = nm->m;
  unsigned long long totals[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(totals, nm->totals.get(), sizeof(totals), hipMemcpyDeviceToHost, v.stream));
  if (tile_max) HIPCHK(c, hipMemcpyAsync(tile_max, m.tile_max.get(), m.tile_max.bytes(), hipMemcpyDeviceToHost, v.stream));
  if (tile_above) HIPCHK(c, hipMemcpyAsync(tile_above, m.tile_above.get(), m.tile_above.bytes(), hipMemcpyDeviceToHost, v.stream));
  HIPCHK(c, hipStreamSynchronize(v.stream));
  if (rep) {
    rep->fbs = nm->fbs;
    rep->tiles_x = m.grid.tiles_x;
    rep->tiles_y = m.grid.tiles_y;
    rep->pad = 0;
    rep->pixels = m.grid.pixels();
    rep->pixels_above = (int64_t)totals[0];
    rep->threshold = threshold;
    const uint32_t bits = (uint32_t)totals[1];
    memcpy(&rep->max_noise, &bits, sizeof(bits));
  }
  return RT_OK;
}

int rt_noise_map(rt_noise* nm, float* out) {
  if (!nm) return RT_ERR_ARG;
  if (!nm->acc) return RT_ERR_STATE;  // detached
  rt_ctx* c = nm->acc->ctx;
  if (!out) return fail(c, RT_ERR_ARG, "null map");
  if (nm->fbs < 2) return fail(c, RT_ERR_STATE, "noise needs at least 2 frame buffers");
  const View v = view(c);
  HIPCHK(c, hipSetDevice(v.device));
  const Staged<float> st(out, (size_t)nm->m.grid.pixels());  // a host map is staged through device memory
  if (!st.ok()) return fail(c, RT_ERR_NOMEM, "hipMalloc noise map");
  int rc = noise_run(nm, 0.0f, st.dev());
  if (!rc && st.host() && hipMemcpyAsync(out, st.dev(), st.bytes(), hipMemcpyDeviceToHost, v.stream) != hipSuccess)
    rc = fail(c, RT_ERR_HIP, "copy noise map");
  if (hipStreamSynchronize(v.stream) != hipSuccess && !rc) rc = fail(c, RT_ERR_HIP, "noise measure kernel");
  return rc;
}

float rt_noise_last_measure_ms(const rt_noise* nm) { return nm ? nm->timer.ms() : 0.0f; }

int rt_denoise_monitor(rt_noise* nm, const rt_denoise_params* params, uint8_t* out, float* gain, int32_t png_order) {
  if (!nm) return RT_ERR_ARG;
  if (!nm->acc) return RT_ERR_STATE;  // detached
  if (nm->fbs < 2) return fail(nm->acc->ctx, RT_ERR_STATE, "denoise needs at least 2 frame buffers");
  return denoise_out(*nm->acc, nm->m, nullptr, nm->fbs, nm->denoise_timer, params, out, gain, png_order);
}
float rt_denoise_monitor_last_ms(const rt_noise* nm) { return nm ? nm->denoise_timer.ms() : 0.0f; }

int rt_guide_denoise_monitor(rt_noise* nm, rt_guide* g, const rt_denoise_params* params, const rt_guide_params* gparams,
                             uint8_t* out, float* gain, int32_t png_order) {
  if (!nm || !g) return RT_ERR_ARG;
  if (!nm->acc) return RT_ERR_STATE;  // detached
  rtdn::GuideView gv;
  const int rc = guide_view(*nm->acc, nm->acc->scene_fp, g, gparams, &gv);
  if (rc) return rc;
  if (nm->fbs < 2) return fail(nm->acc->ctx, RT_ERR_STATE, "denoise needs at least 2 frame buffers");
  return denoise_out(*nm->acc, nm->m, nullptr, nm->fbs, nm->denoise_timer, params, out, gain, png_order, &gv);
}

int rt_noise_save(rt_noise* nm, void* blob, size_t cap, size_t* need) {
  if (!nm) return RT_ERR_ARG;
  if (!nm->acc) return RT_ERR_STATE;  // detached
  rt_ctx* c = nm->acc->ctx;
  const Moments& m = nm->m;
  const size_t total = rtacc::kHeaderBytes + m.s2.bytes() + m.s1.bytes();
  if (need) *need = total;
  if (!blob && cap == 0) return RT_OK;  // size query
  if (!blob || cap < total) return fail(c, RT_ERR_ARG, "noise blob buffer too small");
  const View v = view(c);
  HIPCHK(c, hipSetDevice(v.device));
  // the moments land in the blob's payload, then the header is packed around them
  unsigned char* p2 = static_cast<unsigned char*>(blob) + rtacc::kHeaderBytes;
  unsigned char* p1 = p2 + m.s2.bytes();
  HIPCHK(c, hipMemcpyAsync(p2, m.s2.get(), m.s2.bytes(), hipMemcpyDeviceToHost, v.stream));
  HIPCHK(c, hipMemcpyAsync(p1, m.s1.get(), m.s1.bytes(), hipMemcpyDeviceToHost, v.stream));
  HIPCHK(c, hipStreamSynchronize(v.stream));
  rt_accum_info info;
  rt_accum_get_info(nm->acc, &info);
  info.args.fb_count = nm->fbs;
  if (rt_noise_blob_pack(&info, reinterpret_cast<const uint32_t*>(p1), reinterpret_cast<const uint64_t*>(p2), blob, cap, nullptr))
    return fail(c, RT_ERR_ARG, "pack noise blob");
  return RT_OK;
}

int rt_noise_load(rt_accum* acc, const void* blob, size_t n, rt_noise** out) {
  if (!acc) return RT_ERR_ARG;
  rt_ctx* c = acc->ctx;
  if (!out) return fail(c, RT_ERR_ARG, "null monitor pointer");
  *out = nullptr;
  rt_accum_info info, have;
  if (rt_noise_blob_info(blob, n, &info)) return fail(c, RT_ERR_ARG, "malformed noise blob");
  if (acc->noise) return fail(c, RT_ERR_STATE, "the accumulator has a noise monitor already");
  rt_accum_get_info(acc, &have);
  const rt_render_args &a = info.args, &b = have.args;
  if (a.width != b.width || a.height != b.height || a.spp != b.spp || a.fb_first != b.fb_first || a.fb_count != b.fb_count ||
      a.max_depth != b.max_depth || a.cam_mode != b.cam_mode || a.band_rows != b.band_rows || a.band_first != b.band_first ||
      a.band_stride != b.band_stride || a.stats != b.stats || a.flags != b.flags || a.seed != b.seed ||
      info.n_values != have.n_values || info.scene_fp != have.scene_fp)
    return fail(c, RT_ERR_STATE, "noise blob belongs to another accumulator state");
  rt_noise* nm = nullptr;
  int rc = noise_new(acc, &nm);
  if (rc) return rc;
  const hipStream_t stream = stream_of(c);
  const Moments& m = nm->m;
  const unsigned char* p2 = static_cast<const unsigned char*>(blob) + rtacc::kHeaderBytes;
  const unsigned char* p1 = p2 + m.s2.bytes();
  if (hipMemcpyAsync(m.s2.get(), p2, m.s2.bytes(), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(m.s1.get(), p1, m.s1.bytes(), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess) {
    rt_noise_destroy(nm);
    return fail(c, RT_ERR_HIP, "copy noise moments to device");
  }
  nm->fbs = info.args.fb_count;
  *out = nm;
  return RT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------- tile launches, adaptive accumulator
// rt_render over a set of the noise monitor's tiles (16 x 16 pixels over (owned-row index, column)), and
// the accumulator that stops rendering a tile once its own noise estimate is low enough (include/rt_hip.h).
struct RT_INTERNAL rt_adapt : AccumCore {
  uint64_t scene_fp = 0;
  Moments m;
  DevBuf<uint32_t> perm;              // [chunk x owned pixels] item list of a tile launch, allocated with scratch
  DevBuf<uint4> ntile;                // [tiles] the active noise tiles' list (tile_items_kernel's records)
  DevBuf<int32_t> tile_n;             // [tiles] n_t
  std::vector<int32_t> n_t;           // host copy of tile_n (kept alive for its upload)
  std::vector<int32_t> active;        // ids of the active tiles, ascending
  std::vector<rttile::Rec> ntile_host;  // what ntile holds (kept alive for its upload)
  std::vector<float> h_max;           // host copies of the measure outputs; once have_measure, the retired
  std::vector<int32_t> h_above;       // tiles' entries are current at threshold `measured` (theirs change only
                                      // once a reopen, which measures every tile, has made them active again)
  float measured = 0.0f;
  bool have_measure = false;
  Timer retire_timer;   // around the last retire's measure kernel
  Timer denoise_timer;  // around the last denoise's kernels
};

namespace {

// The records uploaded to ntile_dev and expanded into perm_dev (both large enough), queued on the stream;
// rec must stay alive until the stream has been synchronised (render_dev does).
int tile_items(rt_ctx* c, const std::vector<rttile::Rec>& rec, const TileGrid& g, int fb_count, uint4* ntile_dev,
               uint32_t* perm_dev) {
  const hipStream_t stream = stream_of(c);
  HIPCHK(c, hipMemcpyAsync(ntile_dev, rec.data(), rec.size() * sizeof(uint4), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(tile_items_kernel, dim3((unsigned)rec.size()), dim3(256), 0, stream, ntile_dev, g.tiles_x, g.rows, g.width,
                     fb_count, perm_dev);
  HIPCHK(c, hipGetLastError());
  return RT_OK;
}

// adapt_measure_kernel over the active tiles (all = false; the retired tiles' entries are re-measured too
// when they hold the counts of another threshold) or every tile, then the tile arrays to the host:
// afterwards h_max / h_above are current for every tile at `threshold`.  map_dev may be null.
int adapt_measure(rt_adapt* ad, float threshold, bool all, float* map_dev, bool timed) {
  rt_ctx* c = ad->ctx;
  const hipStream_t stream = stream_of(c);
  const Moments& m = ad->m;
  if (!ad->have_measure || memcmp(&ad->measured, &threshold, sizeof(float)) != 0) all = true;  // counts of another threshold
  const unsigned blocks = all ? (unsigned)m.grid.count() : (unsigned)ad->active.size();
  if (timed) HIPCHK(c, ad->retire_timer.start(stream));
  if (blocks > 0) {
    hipLaunchKernelGGL(adapt_measure_kernel, dim3(blocks), dim3(256), 0, stream, all ? (const uint4*)nullptr : ad->ntile.get(),
                       ad->tile_n.get(), m.s1.get(), m.s2.get(), m.grid.tiles_x, m.grid.rows, m.grid.width, threshold, map_dev,
                       m.tile_max.get(), m.tile_above.get());
    HIPCHK(c, hipGetLastError());
  }
  if (timed) HIPCHK(c, ad->retire_timer.stop(stream));
  HIPCHK(c, hipMemcpyAsync(ad->h_max.data(), m.tile_max.get(), m.tile_max.bytes(), hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipMemcpyAsync(ad->h_above.data(), m.tile_above.get(), m.tile_above.bytes(), hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipStreamSynchronize(stream));
  ad->measured = threshold;
  ad->have_measure = true;
  return RT_OK;
}

// The tiles within Chebyshev distance r >= 0 of a listed tile, over the tile grid (owned-row index, column):
// flags[id] = 1.  A box is a row interval of column intervals: two passes of prefix counts, O(tiles).
std::vector<uint8_t> dilated(const TileGrid& g, const std::vector<int32_t>& listed, int r) {
  const int tx = g.tiles_x, ty = g.tiles_y;
  std::vector<uint8_t> f((size_t)g.count(), 0), h(f.size(), 0), out(f.size(), 0);
  for (int32_t t : listed) f[(size_t)t] = 1;
  std::vector<int32_t> pre((size_t)std::max(tx, ty) + 1, 0);
  for (int y = 0; y < ty; ++y) {  // h: a listed tile within r columns in the same row
    for (int x = 0; x < tx; ++x) pre[(size_t)x + 1] = pre[(size_t)x] + f[(size_t)y * tx + x];
    for (int x = 0; x < tx; ++x) {
      const int lo = x - std::min(r, x), hi = (int)std::min<long long>(tx - 1, (long long)x + r);
      h[(size_t)y * tx + x] = pre[(size_t)hi + 1] - pre[(size_t)lo] > 0;
    }
  }
  for (int x = 0; x < tx; ++x) {  // out: an h within r rows in the same column
    for (int y = 0; y < ty; ++y) pre[(size_t)y + 1] = pre[(size_t)y] + h[(size_t)y * tx + x];
    for (int y = 0; y < ty; ++y) {
      const int lo = y - std::min(r, y), hi = (int)std::min<long long>(ty - 1, (long long)y + r);
      out[(size_t)y * tx + x] = pre[(size_t)hi + 1] - pre[(size_t)lo] > 0;
    }
  }
  return out;
}

void adapt_report(const rt_adapt* ad, float threshold, rt_adapt_report* rep) {
  const TileGrid& g = ad->m.grid;
  rep->fbs = ad->args.fb_count;
  rep->tiles_x = g.tiles_x;
  rep->tiles_y = g.tiles_y;
  rep->tiles_active = (int32_t)ad->active.size();
  rep->pixels = g.pixels();
  rep->pixels_active = 0;
  rep->pixel_fbs = 0;
  rep->pixels_above = 0;
  rep->threshold = threshold;
  float mx = 0.0f;
  for (size_t t = 0; t < (size_t)g.count(); ++t) {
    int tw, th;
    g.size((int)t, tw, th);
    rep->pixel_fbs += (int64_t)tw * th * ad->n_t[t];
    rep->pixels_above += ad->h_above[t];
    mx = std::max(mx, ad->h_max[t]);
  }
  for (int32_t t : ad->active) {
    int tw, th;
    g.size(t, tw, th);
    rep->pixels_active += (int64_t)tw * th;
  }
  rep->max_noise = mx;
}

}  // namespace

extern "C" {

int rt_render_tiles(rt_ctx* c, const rt_render_args* a, const int32_t* tiles, int32_t n_tiles, float* fb,
                    rt_counters* counters) {
  if (!c) return RT_ERR_ARG;
  int rc = validate_args(c, a);
  if (rc) return rc;
  if (!fb) return fail(c, RT_ERR_ARG, "null fb");
  if (!tiles || n_tiles <= 0) return fail(c, RT_ERR_ARG, "empty tile list");
  const int rows = rt_owned_rows(a, nullptr);
  if (rows <= 0) return fail(c, RT_ERR_ARG, "no rows owned");
  const long long items = (long long)a->fb_count * rows * a->width;
  if (items > (1LL << 31)) return fail(c, RT_ERR_ARG, "tile launch: more than 2^31 items (fb_count x owned rows x width)");
  const TileGrid g(rows, a->width);
  const long long n_all = g.count();
  if (n_tiles > n_all) return fail(c, RT_ERR_ARG, "tile list: a repeated tile id");
  std::vector<uint8_t> seen((size_t)n_all, 0);
  for (int k = 0; k < n_tiles; ++k) {
    if (tiles[k] < 0 || tiles[k] >= n_all) return fail(c, RT_ERR_ARG, "tile list: id out of range");
    if (seen[(size_t)tiles[k]]) return fail(c, RT_ERR_ARG, "tile list: a repeated tile id");
    seen[(size_t)tiles[k]] = 1;
  }
  const View v = view(c);
  if (!v.have_scene) return fail(c, RT_ERR_STATE, "no scene uploaded");
  if (!states_are(c, a->width, a->height, a->seed)) return fail(c, RT_ERR_STATE, "rt_render_init not called for this size/seed");
  HIPCHK(c, hipSetDevice(v.device));
  std::vector<rttile::Rec> rec;
  TileLaunch tl{nullptr, rttile::records(tiles, n_tiles, g.tiles_x, rows, a->width, a->fb_count, rec)};
  DevBuf<uint4> ntile;
  DevBuf<uint32_t> perm;
  const Staged<float> st(fb, (size_t)items * 3);  // a host fb is staged in and out: the floats outside the listed tiles stay
  if (!ntile.alloc(rec.size()) || !perm.alloc((size_t)tl.n_items) || !st.ok()) rc = fail(c, RT_ERR_NOMEM, "hipMalloc tile launch");
  if (!rc && st.host() && hipMemcpy(st.dev(), fb, st.bytes(), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(c, RT_ERR_HIP, "copy frame buffer to device");
  if (!rc) rc = tile_items(c, rec, g, a->fb_count, ntile.get(), perm.get());
  tl.perm = perm.get();
  if (!rc) rc = render_dev(c, a, st.dev(), counters, &tl);
  if (hipStreamSynchronize(v.stream) != hipSuccess && !rc) rc = fail(c, RT_ERR_HIP, "tile launch");
  if (!rc && st.host() && hipMemcpy(fb, st.dev(), st.bytes(), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(c, RT_ERR_HIP, "copy frame buffer to host");
  return rc;
}

int rt_adapt_destroy(rt_adapt* ad) {
  if (!ad) return RT_ERR_ARG;
  const View v = view(ad->ctx);
  (void)hipSetDevice(v.device);
  (void)hipStreamSynchronize(v.stream);
  delete ad;
  return RT_OK;
}

int rt_adapt_create(rt_ctx* c, const rt_render_args* a, int32_t chunk_fbs, rt_adapt** out) {
  if (!c) return RT_ERR_ARG;
  if (!out) return fail(c, RT_ERR_ARG, "null adaptive accumulator pointer");
  *out = nullptr;
  int rows = 0;
  const int rc = create_check(c, a, chunk_fbs, &rows);
  if (rc) return rc;
  if ((long long)chunk_fbs * rows * a->width > (1LL << 31)) return fail(c, RT_ERR_ARG, "chunk_fbs x owned rows x width > 2^31");
  const TileGrid g(rows, a->width);
  if (!g.ids_fit()) return fail(c, RT_ERR_ARG, "adaptive accumulator: too many tiles");
  const View v = view(c);
  if (!v.have_scene) return fail(c, RT_ERR_STATE, "no scene uploaded");
  HIPCHK(c, hipSetDevice(v.device));
  std::unique_ptr<rt_adapt> ad(new rt_adapt);
  core_init(*ad, c, a, chunk_fbs, rows);
  ad->scene_fp = v.scene_fp;
  const size_t tiles = (size_t)g.count();
  ad->n_t.assign(tiles, 0);
  ad->h_max.assign(tiles, 0.0f);
  ad->h_above.assign(tiles, 0);
  ad->active.resize(tiles);
  for (size_t t = 0; t < tiles; ++t) ad->active[t] = (int32_t)t;
  if (!ad->sums.alloc((size_t)ad->per_fb) || !ad->m.alloc(g) || !ad->ntile.alloc(tiles) || !ad->tile_n.alloc(tiles))
    return fail(c, RT_ERR_NOMEM, "hipMalloc adaptive accumulator");
  if (!ad->add_timer.create() || !ad->retire_timer.create() || !ad->denoise_timer.create() || !ad->sums.clear(v.stream) || !ad->m.clear(v.stream) ||
      !ad->tile_n.clear(v.stream) || !ad->m.tile_max.clear(v.stream) || !ad->m.tile_above.clear(v.stream))
    return fail(c, RT_ERR_HIP, "set up adaptive accumulator");
  *out = ad.release();
  return RT_OK;
}

int rt_adaptive_add(rt_adapt* ad, int32_t count, int32_t limit, rt_counters* counters) {
  if (!ad) return RT_ERR_ARG;
  rt_ctx* c = ad->ctx;
  const rt_render_args& a = ad->args;
  if (count < 1) return fail(c, RT_ERR_ARG, "count < 1");
  if (limit < 1) return fail(c, RT_ERR_ARG, "limit < 1");
  // the tiles that receive something, grouped by n_t (what a tile receives is a function of its n_t), the
  // groups in ascending n_t, a group's tiles in ascending id; checked before anything is rendered
  std::vector<std::pair<int32_t, int32_t>> by_n;  // (n_t, id)
  for (int32_t t : ad->active) {
    const int32_t n = ad->n_t[(size_t)t];
    if (n >= limit) continue;  // at the limit: receives nothing, stays active
    const int32_t give = std::min(count, limit - n);
    if (give > rtacc::kNoiseMaxFbs - n) return fail(c, RT_ERR_ARG, "noise monitor: more than 32768 frame buffers");
    if (a.fb_first > INT32_MAX - n - give) return fail(c, RT_ERR_ARG, "fb range overflows");
    by_n.emplace_back(n, t);
  }
  if (ad->scene_gen != view(c).scene_gen) return fail(c, RT_ERR_STATE, "scene uploaded again since the accumulator was created");
  rt_counters total = {};
  if (by_n.empty()) {  // every tile has retired or is at the limit: nothing is rendered
    if (counters) *counters = total;
    return RT_OK;
  }
  std::sort(by_n.begin(), by_n.end());
  const hipStream_t stream = stream_of(c);
  HIPCHK(c, hipSetDevice(view(c).device));
  int rc = ensure_states(c, a.width, a.height, a.seed);
  if (rc) return rc;
  const TileGrid& g = ad->m.grid;
  if (!ad->scratch) {
    const size_t px = (size_t)ad->chunk * g.pixels();
    DevBuf<float> scratch;  // both or neither
    if (!scratch.alloc(px * 3) || !ad->perm.alloc(px)) return fail(c, RT_ERR_NOMEM, "hipMalloc adaptive frame buffers");
    ad->scratch = std::move(scratch);
  }
  std::vector<int32_t> group;
  for (size_t k0 = 0; k0 < by_n.size();) {
    const int32_t n0 = by_n[k0].first, give = std::min(count, limit - n0);
    group.clear();
    for (; k0 < by_n.size() && by_n[k0].first == n0; ++k0) group.push_back(by_n[k0].second);
    // the group's frame buffers fb_first + n0 .., at most chunk per launch: the tile launch, then the fold
    // over the same list, ordered on the stream before the next launch writes the scratch
    for (int32_t done = 0; done < give;) {
      const int32_t n = std::min(give - done, ad->chunk);
      rt_render_args r = a;
      r.fb_first = a.fb_first + n0 + done;
      r.fb_count = n;
      rt_counters cnt = {};
      TileLaunch tl{ad->perm.get(), rttile::records(group.data(), (int)group.size(), g.tiles_x, g.rows, g.width, n, ad->ntile_host)};
      rc = tile_items(c, ad->ntile_host, g, n, ad->ntile.get(), ad->perm.get());
      if (!rc) rc = render_dev(c, &r, ad->scratch.get(), &cnt, &tl);
      if (rc) return rc;
      HIPCHK(c, ad->add_timer.start(stream));
      hipLaunchKernelGGL(adapt_fold_kernel, dim3((unsigned)group.size()), dim3(256), 0, stream, ad->ntile.get(), g.tiles_x, g.rows,
                         g.width, ad->scratch.get(), ad->per_fb, n, ad->sums.get(), ad->m.s1.get(), ad->m.s2.get());
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, ad->add_timer.stop(stream));
      add_counters(total, cnt);
      done += n;
      for (int32_t t : group) ad->n_t[(size_t)t] = n0 + done;  // what the sums hold, also when a later launch fails
      ad->args.fb_count = std::max(ad->args.fb_count, n0 + done);
    }
  }
  HIPCHK(c, hipMemcpyAsync(ad->tile_n.get(), ad->n_t.data(), ad->tile_n.bytes(), hipMemcpyHostToDevice, stream));
  HIPCHK(c, hipStreamSynchronize(stream));
  if (counters) *counters = total;
  return RT_OK;
}

int rt_adapt_add(rt_adapt* ad, int32_t count, rt_counters* counters) {
  if (!ad) return RT_ERR_ARG;
  const int rc = add_check(*ad, count, rtacc::kNoiseMaxFbs - ad->args.fb_count);
  return rc ? rc : rt_adaptive_add(ad, count, rtacc::kNoiseMaxFbs, counters);
}

int rt_adaptive_retire(rt_adapt* ad, float threshold, int32_t max_above, int32_t dilate, rt_adapt_report* rep) {
  if (!ad) return RT_ERR_ARG;
  rt_ctx* c = ad->ctx;
  if (max_above < 0) return fail(c, RT_ERR_ARG, "max_above < 0");
  if (dilate < 0) return fail(c, RT_ERR_ARG, "dilate < 0");
  if (ad->args.fb_count < 2) return fail(c, RT_ERR_STATE, "noise needs at least 2 frame buffers");
  HIPCHK(c, hipSetDevice(view(c).device));
  // the active list on the device: the measure kernel reads the records' ids only
  const TileGrid& g = ad->m.grid;
  rttile::records(ad->active.data(), (int)ad->active.size(), g.tiles_x, g.rows, g.width, 1, ad->ntile_host);
  HIPCHK(c, hipMemcpyAsync(ad->ntile.get(), ad->ntile_host.data(), ad->ntile_host.size() * sizeof(uint4), hipMemcpyHostToDevice,
                           stream_of(c)));
  const int rc = adapt_measure(ad, threshold, false, nullptr, true);
  if (rc) return rc;
  std::vector<int32_t> keep;  // the failing active tiles
  for (int32_t t : ad->active)
    if (ad->h_above[(size_t)t] > max_above) keep.push_back(t);
  if (dilate > 0) {  // ... and the active tiles within `dilate` of one
    const std::vector<uint8_t> near = dilated(g, keep, dilate);
    keep.clear();
    for (int32_t t : ad->active)
      if (near[(size_t)t]) keep.push_back(t);
  }
  ad->active.swap(keep);  // n_t of the others stays where it is
  if (rep) adapt_report(ad, threshold, rep);
  return RT_OK;
}

int rt_adapt_retire(rt_adapt* ad, float threshold, int32_t max_above, rt_adapt_report* rep) {
  return rt_adaptive_retire(ad, threshold, max_above, 0, rep);
}

int rt_adaptive_reopen(rt_adapt* ad, float threshold, int32_t max_above, int32_t dilate, rt_adapt_report* rep) {
  if (!ad) return RT_ERR_ARG;
  rt_ctx* c = ad->ctx;
  if (max_above < 0) return fail(c, RT_ERR_ARG, "max_above < 0");
  if (dilate < 0) return fail(c, RT_ERR_ARG, "dilate < 0");
  if (ad->args.fb_count < 2) return fail(c, RT_ERR_STATE, "noise needs at least 2 frame buffers");
  HIPCHK(c, hipSetDevice(view(c).device));
  const int rc = adapt_measure(ad, threshold, true, nullptr, false);  // every tile, each at its own n_t
  if (rc) return rc;
  const TileGrid& g = ad->m.grid;
  std::vector<int32_t> failing;
  for (int32_t t = 0; t < (int32_t)g.count(); ++t)
    if (ad->h_above[(size_t)t] > max_above) failing.push_back(t);
  std::vector<uint8_t> on = dilated(g, failing, dilate);
  for (int32_t t : ad->active) on[(size_t)t] = 1;  // never retires a tile
  ad->active.clear();
  for (int32_t t = 0; t < (int32_t)g.count(); ++t)
    if (on[(size_t)t]) ad->active.push_back(t);
  if (rep) adapt_report(ad, threshold, rep);
  return RT_OK;
}

int rt_adaptive_active(rt_adapt* ad, uint8_t* flags) {
  if (!ad) return RT_ERR_ARG;
  if (!flags) return fail(ad->ctx, RT_ERR_ARG, "null flags");
  std::fill(flags, flags + ad->n_t.size(), (uint8_t)0);
  for (int32_t t : ad->active) flags[(size_t)t] = 1;
  return RT_OK;
}

int rt_adaptive_save(rt_adapt* ad, void* blob, size_t cap, size_t* need) {
  if (!ad) return RT_ERR_ARG;
  rt_ctx* c = ad->ctx;
  const size_t tiles = ad->n_t.size();
  const rtacc::AdaptLayout l = rtacc::adapt_layout((size_t)ad->per_fb, tiles);
  if (need) *need = l.total;
  if (!blob && cap == 0) return RT_OK;  // size query
  if (!blob || cap < l.total) return fail(c, RT_ERR_ARG, "checkpoint buffer too small");
  const View v = view(c);
  HIPCHK(c, hipSetDevice(v.device));
  // every array lands in the blob's payload, then the header is packed around them
  unsigned char* p = static_cast<unsigned char*>(blob);
  memcpy(p + l.n_t, ad->n_t.data(), 4 * tiles);
  rt_adaptive_active(ad, p + l.active);
  const Moments& m = ad->m;
  HIPCHK(c, hipMemcpyAsync(p + l.sums, ad->sums.get(), ad->sums.bytes(), hipMemcpyDeviceToHost, v.stream));
  HIPCHK(c, hipMemcpyAsync(p + l.s2, m.s2.get(), m.s2.bytes(), hipMemcpyDeviceToHost, v.stream));
  HIPCHK(c, hipMemcpyAsync(p + l.s1, m.s1.get(), m.s1.bytes(), hipMemcpyDeviceToHost, v.stream));
  HIPCHK(c, hipStreamSynchronize(v.stream));
  rt_accum_info info;
  info.args = ad->args;
  info.n_values = ad->per_fb;
  info.scene_fp = ad->scene_fp;
  if (rt_adaptive_blob_pack(&info, reinterpret_cast<const int32_t*>(p + l.n_t), p + l.active,
                            reinterpret_cast<const float*>(p + l.sums), reinterpret_cast<const uint32_t*>(p + l.s1),
                            reinterpret_cast<const uint64_t*>(p + l.s2), blob, cap, nullptr))
    return fail(c, RT_ERR_ARG, "pack adaptive checkpoint");
  return RT_OK;
}

int rt_adaptive_load(rt_ctx* c, const void* blob, size_t n, int32_t chunk_fbs, rt_adapt** out) {
  if (!c) return RT_ERR_ARG;
  if (!out) return fail(c, RT_ERR_ARG, "null adaptive accumulator pointer");
  *out = nullptr;
  rt_accum_info info;
  if (rt_adaptive_blob_info(blob, n, &info)) return fail(c, RT_ERR_ARG, "malformed adaptive checkpoint");
  const View v = view(c);
  if (!v.have_scene) return fail(c, RT_ERR_STATE, "no scene uploaded");
  if (info.scene_fp != v.scene_fp) return fail(c, RT_ERR_STATE, "checkpoint belongs to another scene");
  if (info.args.fb_first > INT32_MAX - info.args.fb_count) return fail(c, RT_ERR_ARG, "malformed adaptive checkpoint");
  rt_adapt* ad = nullptr;
  int rc = rt_adapt_create(c, &info.args, chunk_fbs, &ad);
  if (rc) return rc;
  const size_t tiles = ad->n_t.size();
  const rtacc::AdaptLayout l = rtacc::adapt_layout((size_t)info.n_values, tiles);
  if (ad->per_fb != info.n_values || l.total != n) rc = fail(c, RT_ERR_ARG, "malformed adaptive checkpoint");
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  if (!rc) {
    memcpy(ad->n_t.data(), p + l.n_t, 4 * tiles);
    ad->active.clear();
    for (size_t t = 0; t < tiles; ++t)
      if (p[l.active + t]) ad->active.push_back((int32_t)t);
    const Moments& m = ad->m;
    if (hipMemcpyAsync(ad->sums.get(), p + l.sums, ad->sums.bytes(), hipMemcpyHostToDevice, v.stream) != hipSuccess ||
        hipMemcpyAsync(m.s2.get(), p + l.s2, m.s2.bytes(), hipMemcpyHostToDevice, v.stream) != hipSuccess ||
        hipMemcpyAsync(m.s1.get(), p + l.s1, m.s1.bytes(), hipMemcpyHostToDevice, v.stream) != hipSuccess ||
        hipMemcpyAsync(ad->tile_n.get(), ad->n_t.data(), ad->tile_n.bytes(), hipMemcpyHostToDevice, v.stream) != hipSuccess ||
        hipStreamSynchronize(v.stream) != hipSuccess)
      rc = fail(c, RT_ERR_HIP, "copy adaptive checkpoint to device");
  }
  if (rc) {
    rt_adapt_destroy(ad);
    return rc;
  }
  ad->args.fb_count = info.args.fb_count;  // the first measure runs over every tile (have_measure is false)
  *out = ad;
  return RT_OK;
}

int rt_adapt_get_report(rt_adapt* ad, float threshold, rt_adapt_report* rep) {
  if (!ad) return RT_ERR_ARG;
  rt_ctx* c = ad->ctx;
  if (!rep) return fail(c, RT_ERR_ARG, "null report");
  if (ad->args.fb_count < 2) return fail(c, RT_ERR_STATE, "noise needs at least 2 frame buffers");
  HIPCHK(c, hipSetDevice(view(c).device));
  const int rc = adapt_measure(ad, threshold, true, nullptr, false);
  if (rc) return rc;
  adapt_report(ad, threshold, rep);
  return RT_OK;
}

int rt_adapt_counts(rt_adapt* ad, int32_t* tile_fbs) {
  if (!ad) return RT_ERR_ARG;
  if (!tile_fbs) return fail(ad->ctx, RT_ERR_ARG, "null counts");
  std::copy(ad->n_t.begin(), ad->n_t.end(), tile_fbs);
  return RT_OK;
}

int rt_adapt_noise_map(rt_adapt* ad, float* out) {
  if (!ad) return RT_ERR_ARG;
  rt_ctx* c = ad->ctx;
  if (!out) return fail(c, RT_ERR_ARG, "null map");
  if (ad->args.fb_count < 2) return fail(c, RT_ERR_STATE, "noise needs at least 2 frame buffers");
  HIPCHK(c, hipSetDevice(view(c).device));
  const Staged<float> st(out, (size_t)ad->m.grid.pixels());  // a host map is staged through device memory
  if (!st.ok()) return fail(c, RT_ERR_NOMEM, "hipMalloc noise map");
  int rc = adapt_measure(ad, ad->have_measure ? ad->measured : 0.0f, true, st.dev(), false);
  if (!rc && st.host() && hipMemcpy(out, st.dev(), st.bytes(), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(c, RT_ERR_HIP, "copy noise map");
  return rc;
}

int rt_adapt_image(rt_adapt* ad, uint8_t* out, int32_t png_order) {
  if (!ad) return RT_ERR_ARG;
  return image_out(*ad, out, png_order, "hipMalloc adaptive image", [&](uint8_t* img) {
    const TileGrid& g = ad->m.grid;
    hipLaunchKernelGGL(adapt_image_kernel, dim3((unsigned)((g.pixels() + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       stream_of(ad->ctx), ad->sums.get(), ad->tile_n.get(), g.tiles_x, g.rows, g.width, img);
    HIPCHK(ad->ctx, hipGetLastError());
    return (int)RT_OK;
  });
}

int rt_denoise_adaptive(rt_adapt* ad, const rt_denoise_params* params, uint8_t* out, float* gain, int32_t png_order) {
  if (!ad) return RT_ERR_ARG;
  for (int32_t n : ad->n_t)  // V divides by n_t - 1
    if (n < 2) return fail(ad->ctx, RT_ERR_STATE, "denoise needs at least 2 frame buffers in every tile");
  return denoise_out(*ad, ad->m, ad->tile_n.get(), 0, ad->denoise_timer, params, out, gain, png_order);
}
float rt_denoise_adaptive_last_ms(const rt_adapt* ad) { return ad ? ad->denoise_timer.ms() : 0.0f; }

int rt_guide_denoise_adaptive(rt_adapt* ad, rt_guide* g, const rt_denoise_params* params, const rt_guide_params* gparams,
                              uint8_t* out, float* gain, int32_t png_order) {
  if (!ad || !g) return RT_ERR_ARG;
  rtdn::GuideView gv;
  const int rc = guide_view(*ad, ad->scene_fp, g, gparams, &gv);
  if (rc) return rc;
  for (int32_t n : ad->n_t)  // V divides by n_t - 1
    if (n < 2) return fail(ad->ctx, RT_ERR_STATE, "denoise needs at least 2 frame buffers in every tile");
  return denoise_out(*ad, ad->m, ad->tile_n.get(), 0, ad->denoise_timer, params, out, gain, png_order, &gv);
}

float rt_adapt_last_add_ms(const rt_adapt* ad) { return ad ? ad->add_timer.ms() : 0.0f; }
float rt_adapt_last_retire_ms(const rt_adapt* ad) { return ad ? ad->retire_timer.ms() : 0.0f; }

}  // extern "C"
