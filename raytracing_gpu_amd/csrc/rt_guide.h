// rt_guide.h -- internal: what rt_progressive.hip (the guided denoise's entry points on rt_noise and rt_adapt)
// reads of a guide (rt_guide.hip).
#ifndef RT_GUIDE_H
#define RT_GUIDE_H

#include <stdint.h>

#include "../../include/rt_hip.h"

#pragma GCC visibility push(hidden)
namespace rtguide {

// The planes of the last rt_guide_render, in the memory of `device`; width = 0 before one.
struct View {
  int device;
  uint64_t scene_fp;  // rtacc::scene_fingerprint of the guide's scene
  int32_t width, height;
  const float *normal, *albedo, *depth;
};
View view(const rt_guide* g);

}  // namespace rtguide
#pragma GCC visibility pop

#endif  // RT_GUIDE_H
