// curand_kernel.h -- TEST INFRASTRUCTURE: the shim that lets the reference's class headers compile as plain
// host C++ (oracle/refhdr/ref_headers.cpp, `make -C oracle ref`).  It stands in for CUDA's header of the
// same name, which vec3.h and common.h include first.  Everything here is this project's text.
//
// What it fixes (the definitions the host build cannot take from the reference):
//   * __device__ / __host__ / __global__ are defined away; cudaError_t and cudaDeviceReset exist for
//     common.h's check_cuda only.
//   * curandState is XORWOW over six words in rt_read_states order (d, v0..v4); curand_uniform is
//     x * 2^-32 + 2^-33 with separate roundings (pinned by tests/test_oracle_cpu.py).  curand_init is
//     declared for completeness: the class headers never call it, the caller hands states in.
//   * min(float, float), a CUDA global the host has not, is fminf (material.h:78).
//   * the transcendental calls are redirected to rt_detmath.h's det_* functions, the project's
//     definition of libdevice's results: sin (texture.h:38, hittable.h:80), sinf (texture.h:89), cos
//     (hittable.h:81), tan (camera.h:27), log (constant_medium.h:57), acosf / atan2f (sphere.h:25-26) and
//     pow(float, 5) (material.h:102).  Every other pow goes to the host's (and with -DREFHDR_HOST_POW, a
//     negative control of tests/test_refhdr_cpu.py, that one too).
//   * ceilf returns an int holding the same value: bvh.h:353 has it in a new-declarator, which host C++
//     rejects for a float; its other uses feed an int or powf(2, .).
// Nothing else is redirected: sqrt, fminf, fabsf, floorf, abs, the divisions and every double
// intermediate are what the host compiler makes of the reference's expressions.
#pragma once

#include <math.h>    // with <stdlib.h>: the float and double overloads in the global namespace, as CUDA has them
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <cmath>
#include <iostream>
#include <limits>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../raytracing_gpu_amd/csrc/rt_detmath.h"

#define __device__
#define __host__
#define __global__

typedef int cudaError_t;
inline int cudaDeviceReset() { return 0; }

struct curandState {
  uint32_t d, v[5];
};

namespace refhdr {
extern thread_local long long draws;  // curand_uniform calls on this thread (the build pins count them)
}

void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long offset, curandState* s);

inline float curand_uniform(curandState* s) {
  const uint32_t t = s->v[0] ^ (s->v[0] >> 2);
  s->v[0] = s->v[1];
  s->v[1] = s->v[2];
  s->v[2] = s->v[3];
  s->v[3] = s->v[4];
  s->v[4] = (s->v[4] ^ (s->v[4] << 4)) ^ (t ^ (t << 1));
  s->d += 362437u;
  ++refhdr::draws;
  const float two_m32 = 2.3283064e-10f;
  return (float)(s->v[4] + s->d) * two_m32 + two_m32 / 2.0f;
}

inline float min(float a, float b) { return fminf(a, b); }

namespace refhdr {
inline float t_sin(float x) { return rtm::det_sinf(x); }
inline float t_cos(float x) { return rtm::det_cosf(x); }
inline float t_tan(float x) { return rtm::det_tanf(x); }
inline float t_log(float x) { return rtm::det_logf(x); }
inline float t_acos(float x) { return rtm::det_acosf(x); }
inline float t_atan2(float y, float x) { return rtm::det_atan2f(y, x); }
#ifndef REFHDR_HOST_POW
inline float t_pow(float x, int n) { return n == 5 ? rtm::det_pow5f(x) : (float)::pow((double)x, n); }
#endif
template <class A, class B>
inline auto t_pow(A a, B b) -> decltype(::pow(a, b)) { return ::pow(a, b); }
inline int t_ceil(float x) { return (int)::ceilf(x); }
}  // namespace refhdr

#define sin(x) refhdr::t_sin(x)
#define sinf(x) refhdr::t_sin(x)
#define cos(x) refhdr::t_cos(x)
#define tan(x) refhdr::t_tan(x)
#define log(x) refhdr::t_log(x)
#define acosf(x) refhdr::t_acos(x)
#define atan2f(y, x) refhdr::t_atan2(y, x)
#define pow(a, b) refhdr::t_pow(a, b)
#define ceilf(x) refhdr::t_ceil(x)
