// Elementary functions of the pointwise log-predictive sweep (predictive.hip), written for the fewest
// vector instructions per (row, draw) and kept apart so that a host build can check them against
// long double (tools/predictive_math_check.cpp).  All are branch-free.
//   pd_exp     e^x through the sweeps' 1024-entry table T_j = 2^(j/1024) (sweep_common.h): x is clamped to
//              [-800, 800], n = rint(x 1024/ln2) by the 1.5 2^52 trick, r = x - n ln2/1024 with ln2/1024
//              split in two (the high part has 32 significant bits, so n L_HI is exact for |n| < 2^21),
//              e^r by the sweeps' fitted degree-3 polynomial (|r| <= ln2/2048: relative error 9.4e-17),
//              times T_{n mod 1024}, times 2^{n div 1024} by ldexp, which overflows to +inf past 709.78
//              and underflows through the subnormals to 0 on its own.  A NaN x is clamped to -800 and
//              gives 0: callers that must keep the NaN restore it.  About 2 ulp.
//   pd_rcp     1 / u by v_rcp_f64 and two Newton steps (< 1 ulp for u in [1, 2]).
//   pd_log1p01 log1p(e) for e in [0, 1]: log1p(e) = 2 atanh(s), s = e / (2 + e); above sqrt(2) - 1 the
//              argument is halved first, log1p(e) = ln 2 + 2 atanh((e - 1) / (e + 3)), so |s| <= 0.1716
//              and the odd series to s^21 is exact to 6.4e-19.  The quotient is refined with its own
//              remainder, so a tiny e keeps its relative accuracy: log1p(e) -> e.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define PD_FN __device__ __forceinline__
#define PD_RCP(x) __builtin_amdgcn_rcp(x)
#define PD_LDEXP(x, k) __builtin_amdgcn_ldexp(x, k)
#elif defined(__HIPCC__)
#define PD_FN __host__ __device__ inline
#define PD_RCP(x) (1.0 / (x))
#define PD_LDEXP(x, k) ldexp(x, k)
#else
#define PD_FN inline
#define PD_RCP(x) ((double)(float)(1.0 / (x)))   /* the host check starts from a 24-bit estimate */
#define PD_LDEXP(x, k) ldexp(x, k)
#endif

namespace stk {

PD_FN double pd_exp(double x, const double* tab) {
  constexpr double MAGIC = 6755399441055744.0;            // 1.5 * 2^52
  constexpr double INV_L = 1477.3197218702985;            // 1024 / ln 2
  constexpr double L_HI = 0.00067690154332922248;         // ln 2 / 1024, 32 significant bits
  constexpr double L_LO = 1.8634911419777064e-13;         // ln 2 / 1024 - L_HI
  constexpr double C2 = 0.5000000039583942, C3 = 0.16666666713444417;   // e^r on |r| <= ln2/2048 (fit)
  double a = x > -800.0 ? x : -800.0;                     // NaN -> -800
  a = a < 800.0 ? a : 800.0;
  const double sn = fma(a, INV_L, MAGIC);
  const int ni = (int)(uint32_t)__builtin_bit_cast(uint64_t, sn);
  const double n = sn - MAGIC;
  const double r = fma(-n, L_LO, fma(-n, L_HI, a));
  const double p = fma(fma(fma(C3, r, C2), r, 1.0), r, 1.0);
  return PD_LDEXP(tab[ni & 1023] * p, ni >> 10);
}

PD_FN double pd_rcp(double u) {
  double ri = PD_RCP(u);
  ri = fma(ri, fma(-u, ri, 1.0), ri);
  return fma(ri, fma(-u, ri, 1.0), ri);
}

PD_FN double pd_log1p01(double e) {
  const bool big = e > 0.41421356237309503;
  const double num = big ? (e - 1.0) + (e - 1.0) : e + e, den = big ? e + 3.0 : e + 2.0;   // t = 2 s = num / den
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
  return big ? 0.69314718055994531 + l : l;
}

}  // namespace stk
