// rt_denoise.h -- internal: what rt_progressive.hip (the owner of rt_noise and rt_adapt) calls of rt_denoise.hip.
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_hip.h"
#include "rt_denoise_math.h"

#pragma GCC visibility push(hidden)
namespace rtdn {

// The prepare pass and the filter, queued on stream: the moments s1, s2 of rows x width pixels (whole image,
// rows ascending) after n >= 2 frame buffers -- or, with tile_n, after tile_n[noise tile] >= 2 each -- filtered
// with p (checked by the caller) into out [rows][width][3] and gain [rows][width] (may be null), both device
// memory.  mv: scratch of rows x width x 3 float2.  guide (may be null): the feature planes of rows x width
// pixels in device memory and the gains (checked by the caller) of the guided denoise, which runs the filter's
// GUIDED instances; without it the launches are the unguided ones.
hipError_t launch(hipStream_t stream, const uint32_t* s1, const unsigned long long* s2, const int32_t* tile_n, int n, int rows,
                  int width, const rt_denoise_params& p, float2* mv, uint8_t* out, float* gain,
                  const GuideView* guide = nullptr);

}  // namespace rtdn
#pragma GCC visibility pop

#endif  // RT_DENOISE_H
