// rt_devbuf.h -- internal: owned device memory for the host code of rt_kernels.hip and rt_progressive.hip.
// DevBuf<T> is the one place of the library that calls hipFree (the scene's upload list apart); Staged<T>
// stands a caller's host buffer in device memory for the length of a call.
#ifndef RT_DEVBUF_H
#define RT_DEVBUF_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

#include "rt_ctx_internal.h"

#pragma GCC visibility push(hidden)
namespace rtctx {

// Device memory of n elements, owned: freed with the object (its device must be current then, as in
// every rt_*_destroy and wherever a temporary one lives).  A failing hipFree is ignored: it can fail
// only after an earlier device error, which the next HIP call reports.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(n_, o.n_);
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  // n fresh elements in place of whatever was held; false, and the buffer empty, when the device has no room
  bool alloc(size_t n) {
    reset();
    if (hipMalloc((void**)&p_, n * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      p_ = nullptr;
      return false;
    }
    n_ = n;
    return true;
  }
  // Grow-only: room for n elements.  kept: n fitted and nothing moved; grown: freed and allocated again,
  // the contents gone; failed: no room on the device, the buffer left empty (size 0).
  enum Reserve { kept, grown, failed };
  Reserve reserve(size_t n) {
    if (n <= n_) return kept;
    return alloc(n) ? grown : failed;
  }
  // every byte 0, queued on stream
  bool clear(hipStream_t stream) { return hipMemsetAsync(p_, 0, bytes(), stream) == hipSuccess; }
  T* get() const { return p_; }
  size_t size() const { return n_; }  // elements
  size_t bytes() const { return n_ * sizeof(T); }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// A caller's pointer as memory the kernels may address: p itself, or for host memory a temporary device
// buffer of n elements (the copies in and out are the caller's: which are needed differs).
template <class T>
class Staged {
 public:
  Staged(const T* p, size_t n) : dev_(const_cast<T*>(p)) {
    if (!device_ptr(p)) dev_ = tmp_.alloc(n) ? tmp_.get() : nullptr;
  }
  bool ok() const { return dev_ != nullptr; }  // false: no room for the temporary buffer
  bool host() const { return (bool)tmp_; }
  T* dev() const { return dev_; }
  size_t bytes() const { return tmp_.bytes(); }  // of the temporary buffer

 private:
  DevBuf<T> tmp_;
  T* dev_;
};

}  // namespace rtctx
#pragma GCC visibility pop

#endif  // RT_DEVBUF_H
