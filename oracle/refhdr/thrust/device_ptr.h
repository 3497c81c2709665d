// TEST INFRASTRUCTURE: the little of thrust that common.h's upload_to_device templates name, over the
// host heap (oracle/refhdr/curand_kernel.h has the why).  Nothing on the render path uses it.
#pragma once
#include <stddef.h>
#include <stdlib.h>

namespace thrust {
template <class T>
struct device_ptr {
  T* p = nullptr;
  T& operator[](size_t i) const { return p[i]; }
  T* get() const { return p; }
};
template <class T>
device_ptr<T> device_malloc(size_t n) {
  device_ptr<T> d;
  d.p = static_cast<T*>(malloc(n * sizeof(T)));
  return d;
}
template <class It, class T>
void copy(It first, It last, device_ptr<T> out) {
  for (size_t i = 0; first != last; ++first, ++i) out.p[i] = *first;
}
}  // namespace thrust
