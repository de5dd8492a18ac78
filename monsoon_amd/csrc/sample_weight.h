// The weight of a sampling decision's action (monsoon_rollout_sample, include/monsoon.h): weight24(x) is
// floor(exp(x) * 2**24) for x = (score - best) * inv_temperature <= 0, a uint32 in [0, 2**24], computed without a library
// exponential: range reduction by ln 2 in two parts, a degree-10 Taylor polynomial in Horner form, ldexp, floor.  Every
// operation is a plain *, +, -, floor or ldexp, each rounded once (the library is built with -ffp-contract=off, and no
// term may be contracted into an fma), so the device, host C++ and numpy (monsoon_amd/game_log.py sample_weights) agree
// bit for bit.  The weights are integers: their sum is exact and does not depend on the order of the summands, which is
// what lets a whole wavefront compute a decision's draw (kernels.h sample_pick).
// One text for the kernels and for the host check (tests/sample_weight_check.cpp).  No device intrinsics.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSB_SAMPLE_HD __host__ __device__
#else
#define MSB_SAMPLE_HD
#endif

namespace msb {

constexpr uint32_t SAMPLE_ONE = 1u << 24;   // weight24(0): the weight of the arg-max and of every action tied with it

// x <= 0 (the caller's x is a score minus the decision's best score, scaled); NaN, -inf and x < -32 weigh nothing.
MSB_SAMPLE_HD inline uint32_t weight24(const double x) {
  if (!(x >= -32.0)) return 0u;
  const double n = floor(x * 0x1.71547652b82fep+0 + 0.5);
  const double r = (x - n * 0x1.62e42feep-1) - n * 0x1.a39ef35793c76p-33;
  // c_k = the double nearest 1 / k!, k = 10 .. 0
  double p = 0x1.27e4fb7789f5cp-22;
  p = p * r + 0x1.71de3a556c734p-19;
  p = p * r + 0x1.a01a01a01a01ap-16;
  p = p * r + 0x1.a01a01a01a01ap-13;
  p = p * r + 0x1.6c16c16c16c17p-10;
  p = p * r + 0x1.1111111111111p-7;
  p = p * r + 0x1.5555555555555p-5;
  p = p * r + 0x1.5555555555555p-3;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  return (uint32_t)floor(ldexp(p, (int)n + 24));
}

}  // namespace msb
