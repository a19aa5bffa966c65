// The full-range log1p of the Student-t family (STK_STUDENT, include/stark_hip.h), written for host and
// device so that a host build can check it against long double (tests/test_host_student.py).  Branch-free.
//
//   st_log1p(w), w in [0, +inf]: the row term log1p(z^2 / nu) of student_t's density.  Outliers make w
//   large (z = 1e3 at nu = 1: w = 1e6), nu = 1e6 makes it tiny (w = z^2 / 1e6), so one function has to keep
//   relative accuracy at both ends; pd_log1p01 (predictive_math.h) covers [0, 1] only.
//     w <= sqrt(2) - 1:  log1p(w) = 2 atanh(s), s = w / (2 + w): pd_log1p01's lower arm; log1p(w) -> w.
//     else:              u = 1 + w rounded, lo = (1 + w) - u exactly (Fast2Sum on the larger of the two);
//                        u = m 2^k with m in [sqrt(1/2), sqrt(2)) by integer arithmetic on the high word
//                        (adding 0x3ff00000 - 0x3fe6a09e carries into the exponent exactly where the
//                        mantissa passes sqrt(2)); f = m - 1 is exact and
//                        log1p(w) = k ln 2 + 2 atanh(f / (2 + f)) + lo / u
//                        with ln 2 split in two (the high part has 32 bits: k LN2_HI is exact, |k| <= 1024)
//                        and lo / u from the unrefined reciprocal (the term is below 2^-53 absolute).
//   Either way |s| <= 0.1716 and the odd series to s^21 is exact to 6.4e-19, as in pd_log1p01; the quotient
//   is refined with its own remainder.  w = +inf gives +inf and a NaN stays NaN (the last select); a negative
//   w is not an argument (z^2 / nu >= 0).  Largest relative error found over the host check (tools/student_math_check.cpp): 2.9 x 2^-53.
#pragma once
#include "predictive_math.h"

namespace stk {

PD_FN double st_log1p(double w) {
  constexpr double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
  const bool small = w <= 0.41421356237309503;            // false for a NaN
  const bool gt1 = w > 1.0;
  const double u = 1.0 + w;
  const double lo = (gt1 ? 1.0 : w) - (u - (gt1 ? w : 1.0));
  const uint64_t ub = __builtin_bit_cast(uint64_t, u);
  uint32_t hu = (uint32_t)(ub >> 32) + (0x3ff00000u - 0x3fe6a09eu);
  const int k = (int)(hu >> 20) - 0x3ff;
  hu = (hu & 0x000fffffu) + 0x3fe6a09eu;
  const double m = __builtin_bit_cast(double, ((uint64_t)hu << 32) | (ub & 0xffffffffull));
  const double f = small ? w : m - 1.0;
  const double kd = (double)(small ? 0 : k);
  const double c = small ? 0.0 : lo * PD_RCP(u);
  const double num = f + f, den = f + 2.0;                // t = 2 s = num / den
  double ri = PD_RCP(den);
  ri = fma(ri, fma(-den, ri, 1.0), ri);
  double t = num * ri;
  t = fma(fma(-t, den, num), ri, t);
  const double s2 = 0.25 * (t * t);
  double p = 1.0 / 21.0;
  p = fma(p, s2, 1.0 / 19.0);
  p = fma(p, s2, 1.0 / 17.0);
  p = fma(p, s2, 1.0 / 15.0);
  p = fma(p, s2, 1.0 / 13.0);
  p = fma(p, s2, 1.0 / 11.0);
  p = fma(p, s2, 1.0 / 9.0);
  p = fma(p, s2, 1.0 / 7.0);
  p = fma(p, s2, 1.0 / 5.0);
  p = fma(p, s2, 1.0 / 3.0);
  const double l = fma(t * s2, p, t);
  const double r = fma(kd, LN2_HI, l + fma(kd, LN2_LO, c));
  return w < __builtin_huge_val() ? r : w;
}

}  // namespace stk
