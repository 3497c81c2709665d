// rt_denoise.hip -- the device half of the variance-guided NL-means denoiser (include/rt_hip.h, "denoiser"):
// a prepare pass from the integer moments to (M, V) per value, and the LDS-tiled filter.  The arithmetic of a
// term and of a weight is rt_denoise_math.h's, which the host twin (rt_denoise_blob.cpp) compiles too; every
// sum across pixels is an integer sum, so the reordering below (one search offset at a time, separable patch
// sums) changes no bit.  rt_progressive.hip, which owns rt_noise and rt_adapt, calls rtdn::launch.
#include <hip/hip_runtime.h>

#include "../../include/rt_hip.h"
#include "rt_denoise.h"
#include "rt_denoise_math.h"
#include "rt_quant.h"

namespace {

// The filter's output tile, one lane per pixel.  Measured at 3840 x 2159 with the default radii (10, 3), and
// with (5, 2): 16 x 16 22.3 / 4.99 ms, 32 x 8 24.9 / 5.13, 64 x 8 20.5 / 4.98, 32 x 16 19.7 / 4.32,
// 32 x 32 18.6 / 4.28: the larger the tile, the smaller the share of the patch border in D.
constexpr int kTileW = 32, kTileH = 32;

// (S1, S2, n) -> (M, V), 8 bytes per value; n = tile_n[noise tile of the pixel] (the adaptive accumulator's
// n_t) when tile_n is not null, the monitor's count otherwise.
__global__ __launch_bounds__(kBlock) void denoise_prepare_kernel(const uint32_t* __restrict__ s1,
                                                                const unsigned long long* __restrict__ s2,
                                                                const int32_t* __restrict__ tile_n, int n, int width,
                                                                long long n_values, float2* __restrict__ mv) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n_values) return;
  if (tile_n) {
    const long long px = k / 3;
    const int row = (int)(px / width), col = (int)(px - (long long)row * width);
    n = tile_n[(row >> 4) * ((width + 15) >> 4) + (col >> 4)];
  }
  float M, V;
  rtdn::prepare(s1[k], s2[k], n, &M, &V);
  mv[k] = make_float2(M, V);
}

// The filter.  One workgroup of TW x TH lanes per output tile of TW x TH pixels at (y0, x0).  LDS holds
//   M[3], V[3]  six planes of (TH + 2 (R + F)) rows of HS = TW + 2 (R + F) floats: the tile with a halo of R + F
//               pixels, planar so that consecutive lanes read consecutive dwords; pixels outside the image hold 0
//               and are masked.  32 x 32 at the largest radii: 58 x 58 x 24 B = 80.7 KB, one workgroup per CU
//   D           SH x SW int32, SW = TW + 2 F, SH = TH + 2 F: per pixel a of the tile and its patch border, the three
//               channels' terms T(a, a + o, .) of the current search offset o summed, 0 unless a and a + o are
//               inside the image
//   H           SH x TW int32: D summed along x over the patch width
// For each of the (2R + 1)^2 offsets: every lane computes D for up to kSlotsD pixels a (two for every shape
// measured but 32 x 8; their M and V stay in registers over all offsets), barrier, H from D, barrier, then its own pixel's patch sum P from 2F + 1 rows of
// H, the weight, and Num += W Q_q, Den += W in registers.  The next offset's D is written after the barrier
// that follows the last read of D, and its H after the barrier that follows the last read of H: two barriers
// per offset.  Zeros in D stand for the patch offsets the definition leaves out, and cnt counts the others.
// GUIDED (the guided denoise): the lane's own seven feature values stay in registers over all offsets and the
// partner's are read from global memory per offset (the planes are not staged: LDS is full at the largest
// radii); the weight takes the feature term.  The unguided instances compile none of it.
template <int F, int TW, int TH, bool GUIDED>
__global__ __launch_bounds__(TW * TH) void denoise_filter_kernel(const float2* __restrict__ mv, int rows, int width, int R,
                                                             float alpha, float kk, float eps, uint8_t* __restrict__ out,
                                                             float* __restrict__ gain, const rtdn::GuideView guide) {
  constexpr int SW = TW + 2 * F, SH = TH + 2 * F, NT = TW * TH;
  constexpr int kSlotsD = (SW * SH + NT - 1) / NT, kSlotsH = (SH * TW + NT - 1) / NT;
  extern __shared__ float lds[];
  const int HS = TW + 2 * (R + F), plane = HS * (TH + 2 * (R + F));
  int* const D = reinterpret_cast<int*>(lds + 6 * plane);
  int* const H = D + SW * SH;
  const int tid = threadIdx.x, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;

  for (int i = tid; i < plane; i += NT) {
    const int hy = i / HS, hx = i - hy * HS;
    const int gy = y0 - (R + F) + hy, gx = x0 - (R + F) + hx;
    const bool in = gy >= 0 && gy < rows && gx >= 0 && gx < width;
    const long long k = 3 * ((long long)gy * width + gx);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float2 v = in ? mv[k + j] : make_float2(0.0f, 0.0f);
      lds[j * plane + i] = v.x;
      lds[(3 + j) * plane + i] = v.y;
    }
  }
  __syncthreads();

  // the lane's pixels a for D: index tid + NT s of the SH x SW region
  int a_at[kSlotsD];  // position of a in a plane
  bool a_in[kSlotsD];
  int a_gy[kSlotsD], a_gx[kSlotsD];
  float Ma[kSlotsD][3], Va[kSlotsD][3];
#pragma unroll
  for (int s = 0; s < kSlotsD; ++s) {
    const int i = tid + NT * s, ay = i / SW, ax = i - ay * SW;
    a_gy[s] = y0 - F + ay;
    a_gx[s] = x0 - F + ax;
    a_in[s] = i < SW * SH && a_gy[s] >= 0 && a_gy[s] < rows && a_gx[s] >= 0 && a_gx[s] < width;
    a_at[s] = i < SW * SH ? (ay + R) * HS + ax + R : 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Ma[s][j] = lds[j * plane + a_at[s]];
      Va[s][j] = lds[(3 + j) * plane + a_at[s]];
    }
  }
  const int ly = tid / TW, lx = tid % TW, py = y0 + ly, px = x0 + lx;
  const bool p_in = py < rows && px < width;
  const int p_at = (ly + R + F) * HS + lx + R + F;
  unsigned long long num[3] = {0, 0, 0}, den = 0;
  rtdn::Feature fp = {};
  if (GUIDED && p_in) {
    const long long p = (long long)py * width + px;
#pragma unroll
    for (int j = 0; j < 3; ++j) fp.n[j] = guide.normal[3 * p + j], fp.a[j] = guide.albedo[3 * p + j];
    fp.z = guide.depth[p];
  }

  for (int oy = -R; oy <= R; ++oy)
    for (int ox = -R; ox <= R; ++ox) {
      const int shift = oy * HS + ox;
#pragma unroll
      for (int s = 0; s < kSlotsD; ++s) {
        const int i = tid + NT * s;
        if (i < SW * SH) {
          const int by = a_gy[s] + oy, bx = a_gx[s] + ox;
          int t = 0;
          if (a_in[s] && by >= 0 && by < rows && bx >= 0 && bx < width) {
            const int b_at = a_at[s] + shift;
#pragma unroll
            for (int j = 0; j < 3; ++j)
              t += rtdn::term(Ma[s][j], Va[s][j], lds[j * plane + b_at], lds[(3 + j) * plane + b_at], alpha, kk, eps);
          }
          D[i] = t;
        }
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < kSlotsH; ++s) {
        const int i = tid + NT * s;
        if (i < SH * TW) {
          const int r = i / TW, c = i % TW;
          int h = 0;
#pragma unroll
          for (int u = 0; u <= 2 * F; ++u) h += D[r * SW + c + u];
          H[i] = h;
        }
      }
      __syncthreads();
      const int qy = py + oy, qx = px + ox;
      if (p_in && qy >= 0 && qy < rows && qx >= 0 && qx < width) {
        int P = 0;
#pragma unroll
        for (int u = 0; u <= 2 * F; ++u) P += H[(ly + u) * TW + lx];
        const int cnt = 3 * rtdn::patch_span(px, ox, F, width) * rtdn::patch_span(py, oy, F, rows);
        unsigned long long W;
        if (GUIDED && (oy | ox) != 0) {
          const long long q = (long long)qy * width + qx;
          rtdn::Feature fq;
#pragma unroll
          for (int j = 0; j < 3; ++j) fq.n[j] = guide.normal[3 * q + j], fq.a[j] = guide.albedo[3 * q + j];
          fq.z = guide.depth[q];
          W = rtdn::weight(P, cnt, rtdn::feature_x(fp, fq, guide.gains));
        } else {
          W = rtdn::weight(P, cnt);
        }
        const int q_at = p_at + shift;
#pragma unroll
        for (int j = 0; j < 3; ++j) num[j] += W * rtdn::q_of(lds[j * plane + q_at]);
        den += W;
      }
    }

  if (!p_in) return;
  const long long p = (long long)py * width + px;
#pragma unroll
  for (int j = 0; j < 3; ++j) out[3 * p + j] = (uint8_t)quant(rtdn::linear(num[j], den));
  if (gain) gain[p] = rtdn::gain(den);
}

template <int F, int TW, int TH, bool GUIDED>
hipError_t launch_filter(hipStream_t stream, const rt_denoise_params& p, const float2* mv, int rows, int width, uint8_t* out,
                         float* gain, const rtdn::GuideView& guide) {
  const size_t HW = TW + 2 * (size_t)(p.search_radius + F), HH = TH + 2 * (size_t)(p.search_radius + F);
  const size_t lds = (6 * HW * HH + (size_t)(TW + 2 * F) * (TH + 2 * F) + (size_t)(TH + 2 * F) * TW) * sizeof(float);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&denoise_filter_kernel<F, TW, TH, GUIDED>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)((width + TW - 1) / TW), (unsigned)((rows + TH - 1) / TH));
  hipLaunchKernelGGL((denoise_filter_kernel<F, TW, TH, GUIDED>), grid, dim3(TW * TH), lds, stream, mv, rows, width,
                     p.search_radius, p.alpha, p.k * p.k, p.eps, out, gain, guide);
  return hipGetLastError();
}
template <int TW, int TH, bool GUIDED>
hipError_t launch_filter_f(hipStream_t stream, const rt_denoise_params& p, const float2* mv, int rows, int width, uint8_t* out,
                           float* gain, const rtdn::GuideView& guide) {
  switch (p.patch_radius) {
    case 0: return launch_filter<0, TW, TH, GUIDED>(stream, p, mv, rows, width, out, gain, guide);
    case 1: return launch_filter<1, TW, TH, GUIDED>(stream, p, mv, rows, width, out, gain, guide);
    case 2: return launch_filter<2, TW, TH, GUIDED>(stream, p, mv, rows, width, out, gain, guide);
    default: return launch_filter<3, TW, TH, GUIDED>(stream, p, mv, rows, width, out, gain, guide);
  }
}

}  // namespace

namespace rtdn {

hipError_t launch(hipStream_t stream, const uint32_t* s1, const unsigned long long* s2, const int32_t* tile_n, int n, int rows,
                  int width, const rt_denoise_params& p, float2* mv, uint8_t* out, float* gain, const GuideView* guide) {
  const long long n_values = 3LL * rows * width;
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3((unsigned)((n_values + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, s1, s2,
                     tile_n, n, width, n_values, mv);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (guide) return launch_filter_f<kTileW, kTileH, true>(stream, p, mv, rows, width, out, gain, *guide);
  return launch_filter_f<kTileW, kTileH, false>(stream, p, mv, rows, width, out, gain, GuideView{});
}

}  // namespace rtdn
