// rt_denoise_blob.cpp -- the host-only twin of the denoiser (rt_denoise_monitor_blob, rt_denoise_adaptive_blob
// of include/rt_hip.h): a noise monitor's side file or an adaptive checkpoint filtered without a context or a
// GPU.  Plain C++ with no HIP include; a stand-alone program links this file with rt_accum_blob.cpp,
// rt_noise_blob.cpp and rt_adapt_blob.cpp.
//
// The arithmetic of a term and a weight is rt_denoise_math.h's, which the device kernels (rt_denoise.hip)
// compile too; every sum across pixels is an integer sum, so the order taken here (one search offset at a
// time over the whole image, the patch sums from a summed-area table) gives the device's bytes.
#include <cstring>
#include <vector>

#include "rt_accum_blob.h"
#include "rt_denoise_math.h"

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the payload is read as little-endian integers");

namespace {

// p1 / p2: the blob's S1 (u32) and S2 (u64) arrays, possibly unaligned; tile_n: n_t per noise tile (u8 pointer to
// i32, possibly unaligned), or null with n for every pixel.  guide: the feature planes of the guided denoise, or null.
int denoise_host(int64_t rows, int64_t width, const unsigned char* p1, const unsigned char* p2, const unsigned char* tile_n,
                 int32_t n, const rt_denoise_params* prm, const rtdn::GuideView* guide, uint8_t* out, float* gain) {
  const int64_t px_count = rows * width, tiles_x = (width + rtacc::kNoiseTile - 1) / rtacc::kNoiseTile;
  std::vector<float> M((size_t)px_count * 3), V((size_t)px_count * 3);
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t x = 0; x < width; ++x) {
      int32_t np = n;
      if (tile_n) memcpy(&np, tile_n + 4 * ((r / rtacc::kNoiseTile) * tiles_x + x / rtacc::kNoiseTile), 4);
      for (int j = 0; j < 3; ++j) {
        const int64_t k = 3 * (r * width + x) + j;
        uint32_t s1;
        uint64_t s2;
        memcpy(&s1, p1 + 4 * k, 4);
        memcpy(&s2, p2 + 8 * k, 8);
        rtdn::prepare(s1, s2, np, &M[(size_t)k], &V[(size_t)k]);
      }
    }
  const int R = prm->search_radius, f = prm->patch_radius;
  const float kk = prm->k * prm->k, alpha = prm->alpha, eps = prm->eps;
  std::vector<uint64_t> num((size_t)px_count * 3, 0), den((size_t)px_count, 0);
  std::vector<int64_t> sat((size_t)((rows + 1) * (width + 1)), 0);  // sat[y + 1][x + 1] = sum of T over [0..y] x [0..x]
  const int64_t sw = width + 1;
  for (int oy = -R; oy <= R; ++oy)
    for (int ox = -R; ox <= R; ++ox) {
      if ((oy < 0 ? -oy : oy) >= rows || (ox < 0 ? -ox : ox) >= width) continue;  // no pixel has q inside
      for (int64_t y = 0; y < rows; ++y) {
        int64_t run = 0;
        for (int64_t x = 0; x < width; ++x) {
          const int64_t by = y + oy, bx = x + ox;
          if (by >= 0 && by < rows && bx >= 0 && bx < width) {
            const size_t a = (size_t)(3 * (y * width + x)), b = (size_t)(3 * (by * width + bx));
            for (int j = 0; j < 3; ++j) run += rtdn::term(M[a + j], V[a + j], M[b + j], V[b + j], alpha, kk, eps);
          }
          sat[(size_t)((y + 1) * sw + x + 1)] = sat[(size_t)(y * sw + x + 1)] + run;
        }
      }
      for (int64_t y = 0; y < rows; ++y) {
        const int64_t qy = y + oy;
        if (qy < 0 || qy >= rows) continue;
        const int64_t ylo = oy < 0 ? qy : y, yhi = oy < 0 ? y : qy;  // the patch rows u with y + u and qy + u inside
        const int64_t y0 = y + (-f > -ylo ? -f : -ylo), y1 = y + (f < rows - 1 - yhi ? f : rows - 1 - yhi);
        for (int64_t x = 0; x < width; ++x) {
          const int64_t qx = x + ox;
          if (qx < 0 || qx >= width) continue;
          const int64_t xlo = ox < 0 ? qx : x, xhi = ox < 0 ? x : qx;
          const int64_t x0 = x + (-f > -xlo ? -f : -xlo), x1 = x + (f < width - 1 - xhi ? f : width - 1 - xhi);
          const int64_t P = sat[(size_t)((y1 + 1) * sw + x1 + 1)] - sat[(size_t)(y0 * sw + x1 + 1)] -
                            sat[(size_t)((y1 + 1) * sw + x0)] + sat[(size_t)(y0 * sw + x0)];
          const int32_t cnt = 3 * rtdn::patch_span((int32_t)x, ox, f, (int32_t)width) * rtdn::patch_span((int32_t)y, oy, f, (int32_t)rows);
          const size_t p = (size_t)(y * width + x), q = (size_t)(qy * width + qx);
          uint64_t W;
          if (guide && (oy | ox) != 0) {
            rtdn::Feature fp, fq;
            for (int j = 0; j < 3; ++j) {
              fp.n[j] = guide->normal[3 * p + j], fp.a[j] = guide->albedo[3 * p + j];
              fq.n[j] = guide->normal[3 * q + j], fq.a[j] = guide->albedo[3 * q + j];
            }
            fp.z = guide->depth[p], fq.z = guide->depth[q];
            W = rtdn::weight((int32_t)P, cnt, rtdn::feature_x(fp, fq, guide->gains));
          } else {
            W = rtdn::weight((int32_t)P, cnt);
          }
          for (int j = 0; j < 3; ++j) num[3 * p + j] += W * rtdn::q_of(M[3 * q + j]);
          den[p] += W;
        }
      }
    }
  for (int64_t p = 0; p < px_count; ++p) {
    for (int j = 0; j < 3; ++j) out[3 * p + j] = (uint8_t)rtacc::host_quant(rtdn::linear(num[(size_t)(3 * p + j)], den[(size_t)p]));
    if (gain) gain[p] = rtdn::gain(den[(size_t)p]);
  }
  return RT_OK;
}

// What both entry points check after their blob: the whole-image tiling, the parameters, the image pointer, and
// with planes their gains, pointers and size.
int denoise_check(const rt_accum_info& i, const rt_denoise_params* prm, const rtdn::GuideView* guide, int32_t plane_width,
                  int32_t plane_height, const uint8_t* out) {
  if (!out || !rtdn::params_ok(prm)) return RT_ERR_ARG;
  if (i.n_values != (int64_t)i.args.width * i.args.height * 3) return RT_ERR_ARG;  // a band tiling
  if (guide && (!rtdn::guide_params_ok(&guide->gains) || !guide->normal || !guide->albedo || !guide->depth ||
                plane_width != i.args.width || plane_height != i.args.height))
    return RT_ERR_ARG;
  return RT_OK;
}

}  // namespace

namespace rtdn {

int monitor_blob(const void* blob, size_t n, const rt_denoise_params* prm, const GuideView* guide, int32_t plane_width,
                 int32_t plane_height, uint8_t* out, float* gain) {
  rt_accum_info i;
  rt_denoise_params defaults;
  if (!prm) rt_denoise_params_default(&defaults), prm = &defaults;
  int rc = rt_noise_blob_info(blob, n, &i);
  if (rc) return rc;
  if ((rc = denoise_check(i, prm, guide, plane_width, plane_height, out))) return rc;
  if (i.args.fb_count < 2) return RT_ERR_STATE;
  const unsigned char* p2 = static_cast<const unsigned char*>(blob) + rtacc::kHeaderBytes;
  const unsigned char* p1 = p2 + (size_t)i.n_values * sizeof(uint64_t);
  return denoise_host(i.args.height, i.args.width, p1, p2, nullptr, i.args.fb_count, prm, guide, out, gain);
}

int adaptive_blob(const void* blob, size_t n, const rt_denoise_params* prm, const GuideView* guide, int32_t plane_width,
                  int32_t plane_height, uint8_t* out, float* gain) {
  rt_accum_info i;
  rt_denoise_params defaults;
  if (!prm) rt_denoise_params_default(&defaults), prm = &defaults;
  int rc = rt_adaptive_blob_info(blob, n, &i);
  if (rc) return rc;
  if ((rc = denoise_check(i, prm, guide, plane_width, plane_height, out))) return rc;
  const int64_t tiles_x = (i.args.width + rtacc::kNoiseTile - 1) / rtacc::kNoiseTile;
  const int64_t tiles_y = (i.args.height + rtacc::kNoiseTile - 1) / rtacc::kNoiseTile;
  const rtacc::AdaptLayout l = rtacc::adapt_layout((size_t)i.n_values, (size_t)(tiles_x * tiles_y));
  const unsigned char* p = static_cast<const unsigned char*>(blob);
  for (int64_t t = 0; t < tiles_x * tiles_y; ++t) {  // V divides by n_t - 1
    int32_t nt;
    memcpy(&nt, p + l.n_t + 4 * t, 4);
    if (nt < 2) return RT_ERR_STATE;
  }
  return denoise_host(i.args.height, i.args.width, p + l.s1, p + l.s2, p + l.n_t, 0, prm, guide, out, gain);
}

}  // namespace rtdn

extern "C" {

void rt_denoise_params_default(rt_denoise_params* p) {
  if (!p) return;
  p->search_radius = 10;
  p->patch_radius = 3;
  p->k = 0.45f;
  p->alpha = 1.0f;
  p->eps = 1.0f;
  p->pad = 0;
}

int rt_denoise_monitor_blob(const void* blob, size_t n, const rt_denoise_params* prm, uint8_t* out, float* gain) {
  return rtdn::monitor_blob(blob, n, prm, nullptr, 0, 0, out, gain);
}

int rt_denoise_adaptive_blob(const void* blob, size_t n, const rt_denoise_params* prm, uint8_t* out, float* gain) {
  return rtdn::adaptive_blob(blob, n, prm, nullptr, 0, 0, out, gain);
}

}  // extern "C"
