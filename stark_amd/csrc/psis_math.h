// Per-row arithmetic of the PSIS-LOO sweep (loo.hip), given a row's S log importance ratios lr_s = -ll_s
// SORTED ascending and not yet shifted: the tail length, the Zhang-Stephens fit of the generalised
// Pareto tail with the loo package's prior, the smoothed tail, and the three logsumexps (the
// definitions are in include/stark_hip.h).  Kept apart so that a host build can check it against
// long double (tools/psis_math_check.cpp).
//
// The pieces are what one lane of the kernel evaluates: psis_theta / psis_kbar / psis_profile for grid
// point j, psis_weight for its weight, psis_smooth for tail value j.  Every sum inside a piece runs in
// index order.  psis_row composes them serially (the host check; the kernel composes the same pieces
// with one lane per grid point and per tail value, and sums the S-long logsumexps lane-strided, so its
// bits differ from psis_row's in the last places only).
//
// The fit's inner loop is M log1p per grid point: ps_log1p is its own (ps_log: frexp, the mantissa moved to
// [sqrt 1/2, sqrt 2), log m = 2 atanh((m - 1) / (m + 1)) by predictive_math.h's odd series to s^21, plus
// e ln 2 with ln 2 split in two; log1p(z) = log(u) + (z - (u - 1)) / u with u = 1 + z; about 1 ulp, a third
// of the library's instructions; anything but a positive finite u goes to the library).  The weights'
// and the S-long sums' exp is predictive_math.h's table exp; the other exp / log / expm1 (a few per lane)
// are the library's.
#pragma once
#include "predictive_math.h"

#if defined(__HIPCC__)
#define PS_HD __host__ __device__ inline   /* the integer geometry: the launcher calls it on the host */
#else
#define PS_HD inline
#endif

namespace stk {

constexpr int PSIS_SMAX = 1024;   // draws per row at most (the row matrix must fit the LDS)
constexpr int PSIS_MMAX = 96;     // tail values at most: ceil(3 sqrt(1024))
constexpr int PSIS_GMAX = 39;     // grid points at most: 30 + floor(sqrt(96))

// M = ceil(min(0.2 S, 3 sqrt S)) in integers: ceil(S / 5) and the least b with b^2 >= 9 S
PS_HD int psis_tail_len(int S) {
  const int a = (S + 4) / 5;
  int b = 0;
  while (b * b < 9 * S) ++b;
  return a < b ? a : b;
}
PS_HD int psis_grid(int M) {      // 30 + floor(sqrt M)
  int r = 0;
  while ((r + 1) * (r + 1) <= M) ++r;
  return 30 + r;
}
PS_HD int psis_xstar_index(int M) { return (M + 2) / 4; }   // floor(M / 4 + 0.5), 1-based

PD_FN double ps_log(double u) {
  if (!(u > 0.0 && u < __builtin_huge_val())) return log(u);   // 0, negative, +inf, NaN: the library's answer
  int e;
  double m = frexp(u, &e);                                // [1/2, 1)
  const bool lo = m < 0.70710678118654752;
  m = lo ? m + m : m;                                     // [sqrt 1/2, sqrt 2)
  e = lo ? e - 1 : e;
  const double num = (m - 1.0) + (m - 1.0), den = m + 1.0;   // t = 2 s = num / den, m - 1 exact
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
  constexpr double LN2_HI = 0.6931471803691238, LN2_LO = 1.9082149293851713e-10;   // the high part: 32 significant bits
  const double de = (double)e;
  return fma(de, LN2_HI, l) + de * LN2_LO;
}
PD_FN double ps_log1p(double z) {
  const double u = 1.0 + z;
  const double c = z - (u - 1.0);                          // what the rounding of u lost
  const double l = ps_log(u);
  return (u > 0.0 && u < __builtin_huge_val()) ? fma(c, pd_rcp(u), l) : l;
}

// grid point j = 1 .. Mg
PD_FN double psis_theta(int j, int Mg, double xN, double xstar) {
  return 1.0 / xN + (1.0 - sqrt((double)Mg / ((double)j - 0.5))) / 3.0 / xstar;
}
// mean_i log1p(-theta x_i), in index order
PD_FN double psis_kbar(double theta, const double* x, int M) {
  double s = 0.0;
  for (int i = 0; i < M; ++i) s += ps_log1p(-theta * x[i]);
  return s / (double)M;
}
PD_FN double psis_profile(double theta, double k, int M) { return (double)M * (log(-theta / k) - k - 1.0); }
// 1 / sum_i exp(l_i - l_j): an overflow of the sum gives 0
PD_FN double psis_weight(const double* l, int Mg, int j, const double* tab) {
  double s = 0.0;
  for (int i = 0; i < Mg; ++i) {
    const double dl = l[i] - l[j];
    const double e = pd_exp(dl, tab);
    s += dl != dl ? dl : e;                                // pd_exp turns a NaN into 0: put it back
  }
  return 1.0 / s;
}
PD_FN double psis_khat(double k, int M) { return (k * (double)M + 5.0) / ((double)M + 10.0); }
// smoothed (shifted) tail value j = 1 .. M
PD_FN double psis_smooth(int j, int M, double sigma, double khat, double ecut) {
  const double p = ((double)j - 0.5) / (double)M;
  return log(sigma * expm1(-khat * log1p(-p)) / khat + ecut);
}

// The shifted log weight of sorted position k before normalisation: min(. , 0) of the smoothed tail
// value (sm, when the row is smoothed and k lies in the tail) or of lr_k - max.
PD_FN double psis_lw(const double* v, int k, int S, int M, bool smoothed, const double* sm) {
  const double a = (smoothed && k >= S - M) ? sm[k - (S - M)] : v[k] - v[S - 1];
  return a < 0.0 ? a : 0.0;       // a NaN becomes 0 here; a NaN row never reaches this (the flag)
}

// A whole row, serially.  v [S]: the sorted, unshifted, FINITE lr; tab: the 1024-entry exp table;
// work: PSIS_MMAX + 2 * PSIS_GMAX doubles.  out: elpd_loo, khat, lppd, p_loo.
PD_FN void psis_row(const double* v, int S, const double* tab, double* work, double out[4]) {
  const double inf = __builtin_huge_val();
  const int M = psis_tail_len(S);
  double khat = inf;
  bool smoothed = false;
  double* x = work;               // the exceedances, then the smoothed tail
  double* l = work + PSIS_MMAX;
  double* tw = l + PSIS_GMAX;
  const double mx = v[S - 1];
  if (M >= 5 && (v[S - 1] - mx) - (v[S - M] - mx) > 0.0) {
    const double ecut = exp(v[S - M - 1] - mx);
    for (int i = 0; i < M; ++i) x[i] = exp(v[S - M + i] - mx) - ecut;
    const int Mg = psis_grid(M);
    const double xN = x[M - 1], xstar = x[psis_xstar_index(M) - 1];
    for (int j = 1; j <= Mg; ++j) {
      const double th = psis_theta(j, Mg, xN, xstar);
      l[j - 1] = psis_profile(th, psis_kbar(th, x, M), M);
    }
    for (int j = 1; j <= Mg; ++j) tw[j - 1] = psis_theta(j, Mg, xN, xstar) * psis_weight(l, Mg, j - 1, tab);
    double that = 0.0;
    for (int j = 0; j < Mg; ++j) that += tw[j];
    const double k = psis_kbar(that, x, M), sigma = -k / that;
    khat = psis_khat(k, M);
    if (khat - khat == 0.0) {     // finite
      smoothed = true;
      for (int j = 1; j <= M; ++j) x[j - 1] = psis_smooth(j, M, sigma, khat, ecut);
    }
  }
  // logsumexp of lw, of ll + lw and of ll = -v: the maxima, then the sums
  double m1 = -inf, m2 = -inf;
  for (int k = 0; k < S; ++k) {
    const double lw = psis_lw(v, k, S, M, smoothed, x), b = lw - v[k];
    m1 = lw > m1 ? lw : m1;
    m2 = b > m2 ? b : m2;
  }
  const double m3 = -v[0];
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int k = 0; k < S; ++k) {
    const double lw = psis_lw(v, k, S, M, smoothed, x);
    s1 += pd_exp(lw - m1, tab);
    s2 += pd_exp((lw - v[k]) - m2, tab);
    s3 += pd_exp(-v[k] - m3, tab);
  }
  const double elpd = (m2 + log(s2)) - (m1 + log(s1));
  const double lppd = m3 + log(s3) - log((double)S);
  out[0] = elpd;
  out[1] = khat;
  out[2] = lppd;
  out[3] = lppd - elpd;
}

}  // namespace stk
