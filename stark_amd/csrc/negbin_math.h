// The phi-only terms of the negative-binomial family (STK_NEGBIN, include/stark_hip.h), written
// __host__ __device__ so that k_sweep_reduce_nb and stk_negbin_phi_terms_host run the same code.
//
// With phi = exp(v) and T_j = #{i : y_i > j} (the shard's tail counts),
//   A1(phi) = sum_i sum_{j < y_i} log1p(j / phi)      = sum_j T_j log1p(j / phi)
//   A2(phi) = phi sum_i [psi(y_i + phi) - psi(phi)]   = sum_j T_j phi / (phi + j)
// depend on the shard's count histogram alone.  The table holds T_j for j < ncap = min(max y, NB_CAP);
// the part of a count y > NB_CAP past the cap, sum_{j = NB_CAP}^{y - 1}, is evaluated directly, once
// per distinct value (the table keeps the value and its multiplicity), from the asymptotic series of
// lgamma and digamma, which start at x = NB_CAP + phi >= 1024 here and so need no recurrence:
//   lgamma(x) = (x - 1/2) ln x - x + ln(2 pi)/2 + B(x),   B(x) = 1/(12 x) - 1/(360 x^3) + 1/(1260 x^5)
//   psi(x)    = ln x + A(x),   A(x) = -1/(2 x) - 1/(12 x^2) + 1/(120 x^4) - 1/(252 x^6)
// (next terms 1/(1680 x^7) < 5e-25 and 1/(240 x^8) < 4e-27 at x = 1024).  Differences are formed
// analytically, not by subtracting two large values: with x0 = NB_CAP + phi, x1 = y + phi, M = y - NB_CAP
// and L(k) = ln((k + phi) / phi),
//   sum_{j = NB_CAP}^{y - 1} log1p(j / phi) = lgamma(x1) - lgamma(x0) - M v
//                                           = (x1 - 1/2) L(y) - (x0 - 1/2) L(NB_CAP) - M + B(x1) - B(x0)
//   phi [psi(x1) - psi(x0)]                 = phi [log1p(M / x0) + A(x1) - A(x0)]
// (the v terms cancel exactly: x1 - x0 = M).  L(k) = log1p(k / phi), or ln(k + phi) - v where k / phi
// passes 1e10, so a tiny phi neither overflows the quotient nor turns the sum into +inf.
// phi = 0 or inf (exp(v) under- or overflowed) is the caller's to refuse: lp is NaN there.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NB_FN __host__ __device__ inline
#else
#define NB_FN inline
#endif

namespace stk {

constexpr int NB_CAP = 1024;     // tail counts are kept for j < NB_CAP

// What a negative-binomial shard adds to its ShardDev: derived data, built once at model creation.
// (The gamma family, STK_GAMMA, keeps its shard's one derived number in the same entry: tab points at a single
// double, L = sum_i log y_i, ncap = nbig = 0, and pr_a1, pr_b are the shape's gamma prior.)
struct NbShardDev {
  const double* tab;   // [ncap] T_j, then [nbig][2]: (value, multiplicity) of the distinct counts > NB_CAP
  int ncap;            // min(max y, NB_CAP)
  int nbig;
  double pr_a1, pr_b;  // phi ~ gamma(a, b): a - 1 and b (0, 0: flat, which is gamma(1, 0))
};

// L(k) = ln((k + phi) / phi), k >= 0
NB_FN double nb_log_ratio(double k, double phi, double v) {
  const double r = k / phi;
  return r > 1e10 ? log(k + phi) - v : log1p(r);
}

// Table entry j with tail count T: its terms of A1 and A2.
NB_FN void nb_tail_term(double j, double T, double phi, double v, double* a1, double* a2) {
  *a1 = T * nb_log_ratio(j, phi, v);
  *a2 = T * (phi / (phi + j));
}

// A distinct count y > NB_CAP of multiplicity m: the part of its sums past the cap.
NB_FN void nb_big_term(double y, double m, double phi, double v, double* a1, double* a2) {
  const double x0 = (double)NB_CAP + phi, x1 = y + phi, M = y - (double)NB_CAP;
  const double i0 = 1.0 / x0, i1 = 1.0 / x1, s0 = i0 * i0, s1 = i1 * i1;
  const double B0 = (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0) * s0) * s0) * i0;
  const double B1 = (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0) * s1) * s1) * i1;
  const double A0 = -(0.5 + (1.0 / 12.0 - (1.0 / 120.0 - (1.0 / 252.0) * s0) * s0) * i0) * i0;
  const double A1 = -(0.5 + (1.0 / 12.0 - (1.0 / 120.0 - (1.0 / 252.0) * s1) * s1) * i1) * i1;
  const double L0 = nb_log_ratio((double)NB_CAP, phi, v), L1 = nb_log_ratio(y, phi, v);
  *a1 = m * (((x1 - 0.5) * L1 - (x0 - 0.5) * L0 - M) + (B1 - B0));
  *a2 = m * (phi * (log1p(M * i0) + (A1 - A0)));
}

// Entry e of the whole table (tails, then the large counts), for a caller that splits the entries.
NB_FN void nb_entry_term(const double* tab, int ncap, int e, double phi, double v, double* a1, double* a2) {
  if (e < ncap) nb_tail_term((double)e, tab[e], phi, v, a1, a2);
  else nb_big_term(tab[ncap + 2 * (e - ncap)], tab[ncap + 2 * (e - ncap) + 1], phi, v, a1, a2);
}

}  // namespace stk
