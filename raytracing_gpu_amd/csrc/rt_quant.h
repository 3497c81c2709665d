// rt_quant.h -- internal: the device code that rt_kernels.hip (resolve_kernel) and rt_progressive.hip
// (the accumulators' kernels) both compile.  The byte identity of rt_draw, rt_resolve and the
// accumulators' images rests on all of them quantising with this one function.
#ifndef RT_QUANT_H
#define RT_QUANT_H

#include <hip/hip_runtime.h>

constexpr int kBlock = 256;

// write_frame_buffer quantisation (color.h:40-44); NaN defined as 0.
static __device__ __forceinline__ int quant(float x) {
  const float r = __builtin_sqrtf(x);
  if (!(r == r)) return 0;
  const float c = r < 0.0f ? 0.0f : (r > 0.999f ? 0.999f : r);
  return (int)(256.0f * c);
}

#endif  // RT_QUANT_H
