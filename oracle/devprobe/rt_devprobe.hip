// rt_devprobe.hip -- test infrastructure: the arithmetic that the project's host and device code share
// (csrc/rt_detmath.h, rt_xorwow.h, rt_quant.h, rt_denoise_math.h), one value at a time.
//
// Built with the flags of librt_hip.so (raytracing_gpu_amd/_build.py, build_devprobe) into
// oracle/_build/librt_devprobe.so; oracle/devprobe.py is the ctypes wrapper.  Each family is one functor
// over an index; `*_dev` copies the operands to the device, runs the functor in a bounds-guarded kernel and
// copies the results back, `*_host` runs the same functor in a loop compiled by hipcc's host pass and touches
// no GPU.  Every entry takes host pointers and returns the HIP status (0 for a host twin).  Floats travel as
// bit patterns.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "rt_devprobe_fns.h"
#include "rt_xorwow.h"
#include "rt_denoise_math.h"

// rt_quant.h states quant() for the device alone; the host twin reads the same text with the function marked
// for both sides.
#pragma push_macro("__device__")
#undef __device__
#define __device__ __attribute__((device)) __attribute__((host))
#include "rt_quant.h"
#pragma pop_macro("__device__")

#define DP_HD __host__ __device__ inline
#define DP_API extern "C" __attribute__((visibility("default")))

namespace {

// ------------------------------------------------------------------ the families
struct Unary {
  int fn;
  const uint32_t* x;
  uint32_t* y;
  DP_HD void operator()(size_t i) const {
    y[i] = fn == dp::FN_QUANT ? (uint32_t)quant(rtm::u2f(x[i])) : dp::det_unary(fn, x[i]);
  }
};
// x = first + i: a sweep of consecutive bit patterns without an operand array
struct UnaryRange {
  int fn;
  uint32_t first;
  uint32_t* y;
  DP_HD void operator()(size_t i) const {
    const uint32_t xb = first + (uint32_t)i;
    y[i] = fn == dp::FN_QUANT ? (uint32_t)quant(rtm::u2f(xb)) : dp::det_unary(fn, xb);
  }
};
struct Binary {
  const uint32_t *y, *x;
  uint32_t* out;
  DP_HD void operator()(size_t i) const { out[i] = dp::det_atan2(y[i], x[i]); }
};
struct Checker {
  const uint32_t *a, *b, *c;
  uint32_t* out;
  DP_HD void operator()(size_t i) const { out[i] = dp::det_checker(a[i], b[i], c[i]); }
};
struct SinNeg {
  const uint32_t* x;
  uint32_t* out;
  DP_HD void operator()(size_t i) const { out[i] = dp::det_sin_neg(x[i]); }
};
struct Xorwow {
  const uint32_t* st;  // [n][6]: d, v[0..4]
  uint32_t *word, *ubits, *after;
  DP_HD void operator()(size_t i) const {
    rtx::State s, t;
    s.d = st[6 * i];
    for (int k = 0; k < 5; ++k) s.v[k] = st[6 * i + 1 + k];
    t = s;
    word[i] = rtx::next(s);
    ubits[i] = rtm::f2u(rtx::uniform(t));
    after[6 * i] = s.d;
    for (int k = 0; k < 5; ++k) after[6 * i + 1 + k] = s.v[k];
  }
};
struct SeedState {
  const uint64_t* seed;
  uint32_t* out;  // [n][6]
  DP_HD void operator()(size_t i) const {
    const rtx::State s = rtx::seed_state(seed[i]);
    out[6 * i] = s.d;
    for (int k = 0; k < 5; ++k) out[6 * i + 1 + k] = s.v[k];
  }
};
struct DnPrepare {
  const uint32_t* s1;
  const uint64_t* s2;
  const int32_t* n;
  uint32_t *M, *V;
  DP_HD void operator()(size_t i) const {
    float m, v;
    rtdn::prepare(s1[i], s2[i], n[i], &m, &v);
    M[i] = rtm::f2u(m);
    V[i] = rtm::f2u(v);
  }
};
struct DnQof {
  const uint32_t* M;
  uint32_t* q;
  DP_HD void operator()(size_t i) const { q[i] = rtdn::q_of(rtm::u2f(M[i])); }
};
struct DnTerm {
  const uint32_t* op;  // [n][7]: Ma Va Mb Vb alpha kk eps
  int32_t* t;
  DP_HD void operator()(size_t i) const {
    const uint32_t* o = op + 7 * i;
    t[i] = rtdn::term(rtm::u2f(o[0]), rtm::u2f(o[1]), rtm::u2f(o[2]), rtm::u2f(o[3]), rtm::u2f(o[4]), rtm::u2f(o[5]),
                      rtm::u2f(o[6]));
  }
};
struct DnWeight {
  const int32_t *P, *cnt;
  const uint32_t* xf;  // null: the overload without a feature term
  uint32_t* w;
  DP_HD void operator()(size_t i) const { w[i] = xf ? rtdn::weight(P[i], cnt[i], rtm::u2f(xf[i])) : rtdn::weight(P[i], cnt[i]); }
};
struct DnFeatureX {
  const uint32_t *p, *q;  // [n][7]: n[3] a[3] z
  const uint32_t* g;      // [n][3]: normal, albedo, depth gain
  uint32_t* xf;
  DP_HD static rtdn::Feature load(const uint32_t* w) {
    rtdn::Feature f;
    for (int k = 0; k < 3; ++k) f.n[k] = rtm::u2f(w[k]), f.a[k] = rtm::u2f(w[3 + k]);
    f.z = rtm::u2f(w[6]);
    return f;
  }
  DP_HD void operator()(size_t i) const {
    rt_guide_params gp = {};
    gp.normal_gain = rtm::u2f(g[3 * i]);
    gp.albedo_gain = rtm::u2f(g[3 * i + 1]);
    gp.depth_gain = rtm::u2f(g[3 * i + 2]);
    xf[i] = rtm::f2u(rtdn::feature_x(load(p + 7 * i), load(q + 7 * i), gp));
  }
};
struct DnPatchSpan {
  const int32_t* a;  // [n][4]: p o f size
  int32_t* out;
  DP_HD void operator()(size_t i) const { out[i] = rtdn::patch_span(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]); }
};
struct DnLinearGain {
  const uint64_t *Num, *Den;
  uint32_t *lin, *gain;
  DP_HD void operator()(size_t i) const {
    lin[i] = rtm::f2u(rtdn::linear(Num[i], Den[i]));
    gain[i] = rtm::f2u(rtdn::gain(Den[i]));
  }
};

// ------------------------------------------------------------------ running a family
template <class F>
__global__ void each_kernel(size_t n, F f) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f(i);
}

template <class F>
int run_host(size_t n, const F& f) {
  for (size_t i = 0; i < n; ++i) f(i);
  return 0;
}

// Device copies of an entry's host arrays: in() uploads, out() is copied back by finish(); the first HIP
// error is kept and everything is freed either way.
class Dev {
 public:
  ~Dev() {
    for (void* p : all_) (void)hipFree(p);
  }
  template <class T>
  const T* in(const T* host, size_t count) {
    T* d = alloc<T>(count);
    if (d && count) note(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    return d;
  }
  template <class T>
  T* out(T* host, size_t count) {
    T* d = alloc<T>(count);
    if (d) outs_.push_back({host, d, count * sizeof(T)});
    return d;
  }
  template <class F>
  int run(size_t n, const F& f) {
    if (err_ == hipSuccess && n) {
      const size_t blocks = (n + 255) / 256;
      if (blocks > 0x7fffffffu) return (int)hipErrorInvalidValue;
      each_kernel<<<dim3((unsigned)blocks), dim3(256)>>>(n, f);
      note(hipGetLastError());
      note(hipDeviceSynchronize());
    }
    for (const Out& o : outs_)
      if (err_ == hipSuccess && o.bytes) note(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
    return (int)err_;
  }

 private:
  struct Out {
    void* host;
    void* dev;
    size_t bytes;
  };
  template <class T>
  T* alloc(size_t count) {
    void* p = nullptr;
    if (err_ == hipSuccess) note(hipMalloc(&p, count ? count * sizeof(T) : sizeof(T)));
    if (err_ != hipSuccess) return nullptr;
    all_.push_back(p);
    return (T*)p;
  }
  void note(hipError_t e) {
    if (err_ == hipSuccess) err_ = e;
  }
  hipError_t err_ = hipSuccess;
  std::vector<void*> all_;
  std::vector<Out> outs_;
};

}  // namespace

// ------------------------------------------------------------------ the entries
DP_API int devprobe_unary_host(int fn, const uint32_t* x, uint32_t* y, size_t n) { return run_host(n, Unary{fn, x, y}); }
DP_API int devprobe_unary_dev(int fn, const uint32_t* x, uint32_t* y, size_t n) {
  Dev d;
  const Unary f{fn, d.in(x, n), d.out(y, n)};
  return d.run(n, f);
}
DP_API int devprobe_unary_range_host(int fn, uint32_t first, uint32_t* y, size_t n) { return run_host(n, UnaryRange{fn, first, y}); }
DP_API int devprobe_unary_range_dev(int fn, uint32_t first, uint32_t* y, size_t n) {
  Dev d;
  const UnaryRange f{fn, first, d.out(y, n)};
  return d.run(n, f);
}

DP_API int devprobe_binary_host(const uint32_t* y, const uint32_t* x, uint32_t* out, size_t n) { return run_host(n, Binary{y, x, out}); }
DP_API int devprobe_binary_dev(const uint32_t* y, const uint32_t* x, uint32_t* out, size_t n) {
  Dev d;
  const Binary f{d.in(y, n), d.in(x, n), d.out(out, n)};
  return d.run(n, f);
}

DP_API int devprobe_checker_host(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t n) {
  return run_host(n, Checker{a, b, c, out});
}
DP_API int devprobe_checker_dev(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t n) {
  Dev d;
  const Checker f{d.in(a, n), d.in(b, n), d.in(c, n), d.out(out, n)};
  return d.run(n, f);
}
DP_API int devprobe_sin_neg_host(const uint32_t* x, uint32_t* out, size_t n) { return run_host(n, SinNeg{x, out}); }
DP_API int devprobe_sin_neg_dev(const uint32_t* x, uint32_t* out, size_t n) {
  Dev d;
  const SinNeg f{d.in(x, n), d.out(out, n)};
  return d.run(n, f);
}

DP_API int devprobe_xorwow_host(const uint32_t* st, uint32_t* word, uint32_t* ubits, uint32_t* after, size_t n) {
  return run_host(n, Xorwow{st, word, ubits, after});
}
DP_API int devprobe_xorwow_dev(const uint32_t* st, uint32_t* word, uint32_t* ubits, uint32_t* after, size_t n) {
  Dev d;
  const Xorwow f{d.in(st, 6 * n), d.out(word, n), d.out(ubits, n), d.out(after, 6 * n)};
  return d.run(n, f);
}
DP_API int devprobe_seed_state_host(const uint64_t* seed, uint32_t* out, size_t n) { return run_host(n, SeedState{seed, out}); }
DP_API int devprobe_seed_state_dev(const uint64_t* seed, uint32_t* out, size_t n) {
  Dev d;
  const SeedState f{d.in(seed, n), d.out(out, 6 * n)};
  return d.run(n, f);
}

DP_API int devprobe_dn_prepare_host(const uint32_t* s1, const uint64_t* s2, const int32_t* nn, uint32_t* M, uint32_t* V, size_t n) {
  return run_host(n, DnPrepare{s1, s2, nn, M, V});
}
DP_API int devprobe_dn_prepare_dev(const uint32_t* s1, const uint64_t* s2, const int32_t* nn, uint32_t* M, uint32_t* V, size_t n) {
  Dev d;
  const DnPrepare f{d.in(s1, n), d.in(s2, n), d.in(nn, n), d.out(M, n), d.out(V, n)};
  return d.run(n, f);
}
DP_API int devprobe_dn_q_of_host(const uint32_t* M, uint32_t* q, size_t n) { return run_host(n, DnQof{M, q}); }
DP_API int devprobe_dn_q_of_dev(const uint32_t* M, uint32_t* q, size_t n) {
  Dev d;
  const DnQof f{d.in(M, n), d.out(q, n)};
  return d.run(n, f);
}
DP_API int devprobe_dn_term_host(const uint32_t* op, int32_t* t, size_t n) { return run_host(n, DnTerm{op, t}); }
DP_API int devprobe_dn_term_dev(const uint32_t* op, int32_t* t, size_t n) {
  Dev d;
  const DnTerm f{d.in(op, 7 * n), d.out(t, n)};
  return d.run(n, f);
}
// xf null: weight(P, cnt); else weight(P, cnt, xf)
DP_API int devprobe_dn_weight_host(const int32_t* P, const int32_t* cnt, const uint32_t* xf, uint32_t* w, size_t n) {
  return run_host(n, DnWeight{P, cnt, xf, w});
}
DP_API int devprobe_dn_weight_dev(const int32_t* P, const int32_t* cnt, const uint32_t* xf, uint32_t* w, size_t n) {
  Dev d;
  const DnWeight f{d.in(P, n), d.in(cnt, n), xf ? d.in(xf, n) : nullptr, d.out(w, n)};
  return d.run(n, f);
}
DP_API int devprobe_dn_feature_x_host(const uint32_t* p, const uint32_t* q, const uint32_t* g, uint32_t* xf, size_t n) {
  return run_host(n, DnFeatureX{p, q, g, xf});
}
DP_API int devprobe_dn_feature_x_dev(const uint32_t* p, const uint32_t* q, const uint32_t* g, uint32_t* xf, size_t n) {
  Dev d;
  const DnFeatureX f{d.in(p, 7 * n), d.in(q, 7 * n), d.in(g, 3 * n), d.out(xf, n)};
  return d.run(n, f);
}
DP_API int devprobe_dn_patch_span_host(const int32_t* a, int32_t* out, size_t n) { return run_host(n, DnPatchSpan{a, out}); }
DP_API int devprobe_dn_patch_span_dev(const int32_t* a, int32_t* out, size_t n) {
  Dev d;
  const DnPatchSpan f{d.in(a, 4 * n), d.out(out, n)};
  return d.run(n, f);
}
DP_API int devprobe_dn_linear_gain_host(const uint64_t* Num, const uint64_t* Den, uint32_t* lin, uint32_t* gain, size_t n) {
  return run_host(n, DnLinearGain{Num, Den, lin, gain});
}
DP_API int devprobe_dn_linear_gain_dev(const uint64_t* Num, const uint64_t* Den, uint32_t* lin, uint32_t* gain, size_t n) {
  Dev d;
  const DnLinearGain f{d.in(Num, n), d.in(Den, n), d.out(lin, n), d.out(gain, n)};
  return d.run(n, f);
}
