// rt_devprobe_fns.h -- test infrastructure: the functions of csrc/rt_detmath.h by number, one value at a time,
// for the three compilers that read the header (hipcc's device pass and host pass in rt_devprobe.hip, g++ in
// rt_devprobe_gxx.cpp).  Floats travel as their bit patterns so that a NaN's payload survives the trip.
#ifndef RT_DEVPROBE_FNS_H
#define RT_DEVPROBE_FNS_H

#include "rt_detmath.h"

namespace dp {

enum : int { FN_SIN = 0, FN_COS = 1, FN_TAN = 2, FN_LOG = 3, FN_POW5 = 4, FN_ACOS = 5, FN_QUANT = 6 };

// FN_SIN .. FN_ACOS (FN_QUANT is device code of rt_quant.h: rt_devprobe.hip alone has it).
RT_HD uint32_t det_unary(int fn, uint32_t xb) {
  const float x = rtm::u2f(xb);
  switch (fn) {
    case FN_SIN: return rtm::f2u(rtm::det_sinf(x));
    case FN_COS: return rtm::f2u(rtm::det_cosf(x));
    case FN_TAN: return rtm::f2u(rtm::det_tanf(x));
    case FN_LOG: return rtm::f2u(rtm::det_logf(x));
    case FN_POW5: return rtm::f2u(rtm::det_pow5f(x));
    case FN_ACOS: return rtm::f2u(rtm::det_acosf(x));
    default: return 0xdeadbeefu;
  }
}
RT_HD uint32_t det_atan2(uint32_t yb, uint32_t xb) { return rtm::f2u(rtm::det_atan2f(rtm::u2f(yb), rtm::u2f(xb))); }
RT_HD uint32_t det_checker(uint32_t a, uint32_t b, uint32_t c) {
  return rtm::checker_odd(rtm::u2f(a), rtm::u2f(b), rtm::u2f(c)) ? 1u : 0u;
}
// bit 0: sin_neg_fast's result, bit 1: its ok
RT_HD uint32_t det_sin_neg(uint32_t xb) {
  bool ok;
  const bool neg = rtm::sin_neg_fast(rtm::u2f(xb), ok);
  return (neg ? 1u : 0u) | (ok ? 2u : 0u);
}

}  // namespace dp

#endif  // RT_DEVPROBE_FNS_H
