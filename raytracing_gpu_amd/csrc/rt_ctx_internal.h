// rt_ctx_internal.h -- internal: what rt_progressive.hip (the accumulators, rt_render_tiles) uses of the
// render side.  Everything here is defined in rt_kernels.hip; struct rt_ctx itself stays private to that
// file.  Hidden visibility: the library exports what include/rt_hip.h declares and none of these.
// The owned device buffers of both files (DevBuf, Staged) are rt_devbuf.h, over device_ptr below.
// (The other internal interface of rt_kernels.hip is rt_scene_prep.h: the host-only scene preparation
// behind rt_scene_upload and the constants it shares with the kernels.)
#ifndef RT_CTX_INTERNAL_H
#define RT_CTX_INTERNAL_H

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/rt_hip.h"

// On the definition of a struct that rt_hip.h only names: its members and the templates over it stay inside too.
#define RT_INTERNAL __attribute__((visibility("hidden")))

#pragma GCC visibility push(hidden)
namespace rtctx {

// Records msg as the context's error text (rt_last_error) and returns code.
int fail(rt_ctx* c, int code, const std::string& msg);
// RT_OK for render arguments rt_render accepts.
int validate_args(rt_ctx* c, const rt_render_args* a);
// A pointer the GPU kernels may write directly: device (or managed) memory.
bool device_ptr(const void* p);

// A launch over a caller-built item list (rt_render_tiles): perm[0 .. n_items) are the items to render.
struct TileLaunch {
  const uint32_t* perm;
  unsigned long long n_items;
};
// rt_render into device memory, queued on the context's stream and waited for.
int render_dev(rt_ctx* c, const rt_render_args* a, float* fb_dev, rt_counters* counters, const TileLaunch* tl = nullptr);

// The RNG states are those of (width, height, seed); ensure_states runs rt_render_init when they are
// not, as rt_draw makes them (rendering leaves them as they are).
bool states_are(const rt_ctx* c, int width, int height, uint64_t seed);
int ensure_states(rt_ctx* c, int width, int height, uint64_t seed);

// What the accumulators read of a context, as of the call.
struct View {
  int device;
  hipStream_t stream;
  bool have_scene;
  long long scene_gen;  // counts rt_scene_upload calls
  uint64_t scene_fp;    // rtacc::scene_fingerprint of the uploaded scene
};
View view(const rt_ctx* c);

}  // namespace rtctx
#pragma GCC visibility pop

#define HIPCHK(ctx, call)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) return rtctx::fail(ctx, RT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

#endif  // RT_CTX_INTERNAL_H
