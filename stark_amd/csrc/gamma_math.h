// The shape-only terms of the gamma family (STK_GAMMA, include/stark_hip.h), written __host__ __device__ so
// that k_sweep_reduce_gm and stk_gamma_shape_terms_host run the same code.
//
// With a = exp(u) the shape,
//   kappa(a)  = a log a - a - lgamma(a)        n kappa(a) is the part of lp that depends on the shape alone
//   kappa'(a) = log a - psi(a)   > 0           its derivative, which d lp / d u needs
// Neither is formed from lgamma(a) or digamma(a): at a = 1e8 kappa is about 8, what is left of terms of 1.8e9,
// and kappa' is 5e-9, what is left of two logarithms of 18.  Both are their Stirling remainders,
//   kappa(x)  = (log x - log 2 pi) / 2 - (1/(12 x) - 1/(360 x^3) + 1/(1260 x^5) - 1/(1680 x^7) + 1/(1188 x^9)
//                                         - 691/(360360 x^11))
//   kappa'(x) = 1/(2 x) + 1/(12 x^2) - 1/(120 x^4) + 1/(252 x^6) - 1/(240 x^8) + 1/(132 x^10) - 691/(32760 x^12)
// from x >= GM_STIRLING = 16 on (the first terms left out are 1/(156 x^13) < 1.5e-18 and 1/(12 x^14) < 1.2e-18
// there; in 1 / x, so x = 1e300 neither overflows nor loses anything), and below it the recurrences
//   kappa(x)  = kappa(x + 1)  + [1 - (x + 1) log1p(1 / x)]
//   kappa'(x) = kappa'(x + 1) + [1 / x - log1p(1 / x)]
// carried up to the first x + m >= 16 (at most 16 steps).  Every bracket of kappa' is positive, so kappa' is a
// sum of positive terms, each with a relative error of a few ulp however small x is (1 / x dominates: 1e300 at
// x = 1e-300); the brackets of kappa are O(1) or smaller with an absolute error of an ulp of 1 each, and at a tiny
// x the first is 1 - log(1 / x), the log a that kappa tends to.
// a = 0, a = inf and a NaN (exp(u) under- or overflowed) give NaN for both: lp is not finite there.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GM_FN __host__ __device__ inline
#else
#define GM_FN inline
#endif

namespace stk {

constexpr double GM_STIRLING = 16.0;   // the series start here

// out2[0] = kappa(a), out2[1] = kappa'(a)
GM_FN void gamma_shape_terms(double a, double* out2) {
  if (!(a > 0.0 && a < __builtin_huge_val())) {
    out2[0] = out2[1] = __builtin_nan("");
    return;
  }
  double k0 = 0.0, k1 = 0.0, x = a;
  while (x < GM_STIRLING) {
    const double ix = 1.0 / x;
    const double l = log1p(ix);
    k0 += 1.0 - (x + 1.0) * l;
    k1 += ix - l;
    x += 1.0;
  }
  const double r = 1.0 / x, r2 = r * r;
  const double B = r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0 - r2 * (1.0 / 1188.0 - r2 * (691.0 / 360360.0))))));
  const double A = r * (0.5 + r * (1.0 / 12.0 - r2 * (1.0 / 120.0 - r2 * (1.0 / 252.0 - r2 * (1.0 / 240.0 - r2 * (1.0 / 132.0 - r2 * (691.0 / 32760.0)))))));
  out2[0] = k0 + (0.5 * (log(x) - 1.8378770664093454836) - B);
  out2[1] = k1 + A;
}

}  // namespace stk
