// The posterior predictive replicate y_rep of one (row, draw): a pure function of (seed, stream, row, draw,
// eta, u), ONE definition for k_yrep (ppc.hip) and its host twin (stk_yrep_host).
//
//   counter  call j of element (row i, draw s):  {(uint32) i, (uint32)(i >> 32) | s << 8, stream << 12 | j, TAG_YREP}
//            i: the row's index in its shard, i < 2^40; s: the draw's GLOBAL index, s < 2^24; stream < 2^20 (the
//            shard's global index, as TAG_LAPLACE and TAG_BOOT have it); j < 4096.  U = u53(r.a), V = u53(r.b).
//            One call per element, never shared between rows.
//   logistic g = 1 / (1 + e^-eta) as draw_ll forms it (table exp, refined reciprocal);  y_rep = 1 if U < g else 0
//   linear   z = sqrt(-2 log U) cos(2 pi V) (call 0);  y_rep = eta + e^u z
//   poisson  mu = e^eta (table exp, a NaN put back)
//            mu < 10          inversion of U by upward search: k = 0, p = e^-mu, c = p; while U > c: k += 1,
//                             p *= mu / k, c += p; stopped at k = 128 whatever c is (P(Poisson(10) > 128) < 1e-90:
//                             the stop only catches a c that rounding leaves below U, probability ~1e-16)
//            10 <= mu < 2^30  Hormann's transformed rejection (PTRS, 1993; the constants numpy's legacy generator
//                             uses); attempt j takes (U, V) of call j; after 64 rejected attempts y_rep =
//                             floor(mu + 1/2) (the acceptance rate is above 0.75: 64 rejections have probability
//                             below 1e-38).  At mu = 2^30 the acceptance test's -mu + k log mu - lgamma(k + 1) has
//                             terms of 2.2e10 and so resolves 4e-6 against a left side of order 1.
//            2^30 <= mu < inf y_rep = max(0, floor(mu + sqrt(mu) z + 1/2)), z as for linear: the normal
//                             approximation with the continuity correction.  It has the mean of Poisson(mu) and
//                             the variance mu + 1/12 (relative error below 8e-11); its distribution function
//                             differs from Poisson(mu)'s by the skewness term of the Edgeworth expansion, at most
//                             (1 / (6 sqrt(2 pi mu))) max |1 - x^2| phi(x) sqrt(2 pi) < 0.07 / sqrt(mu) <= 2.1e-6.
//   A non-finite eta, e^u or mu gives NaN, never a finite number.  Every loop has a compile-time bound.
//
// `mg`, where it is not null, receives the smallest relative gap of any comparison that decided the value: for
// a < b, |a - b| / max(|a|, |b|); for a floor, the distance of its argument to the nearest integer over
// max(1, mu); for the PTRS acceptance test, |lhs - rhs| over the largest term of either side (at least 1).
// An element whose gap is below 1e-10 may come out differently from an eta that differs in the last bits.
#pragma once
#include <math.h>
#include <stdint.h>
#include "philox.h"
#include "predictive_math.h"

namespace stk {

constexpr uint32_t YREP_MAX_STREAM = 1u << 20;      // stream is 20 bits of the counter
constexpr int64_t YREP_MAX_DRAWS = (int64_t)1 << 24;   // s is 24
constexpr int YREP_SEARCH = 128;                    // steps of the inversion's search
constexpr int YREP_ATTEMPTS = 64;                   // PTRS attempts
constexpr double YREP_PTRS_MIN = 10.0, YREP_NORMAL_MIN = 1073741824.0;

struct YrepKey { uint64_t seed; uint32_t c0, c1, c2; };
STK_HD YrepKey yrep_key(uint64_t seed, uint32_t stream, int64_t row, uint32_t s) {
  const uint64_t i = (uint64_t)row;
  return {seed, (uint32_t)i, (uint32_t)(i >> 32) | (s << 8), stream << 12};
}
STK_HD void yrep_uv(const YrepKey& k, uint32_t j, double& U, double& V) {
  const u64x2 r = philox(k.seed, k.c0, k.c1, k.c2 | j, TAG_YREP);
  U = u53(r.a);
  V = u53(r.b);
}

STK_HD double yrep_nan() { return __builtin_nan(""); }
STK_HD void yrep_gap(double* mg, double diff, double scale) {
  if (mg) {
    const double g = fabs(diff) / scale;
    if (g < *mg) *mg = g;
  }
}
STK_HD void yrep_gap_cmp(double* mg, double a, double b) {
  const double fa = fabs(a), fb = fabs(b);
  yrep_gap(mg, a - b, fa > fb ? fa : fb);
}
STK_HD void yrep_gap_floor(double* mg, double x, double mu) {
  if (mg) yrep_gap(mg, x - rint(x), mu > 1.0 ? mu : 1.0);
}

// logistic: g, 1 - g and g (1 - g) = e / (1 + e)^2, each without cancellation (e = e^-|eta|)
STK_HD void yrep_logistic_mean(double eta, const double* tab, double& g, double& omg, double& V) {
  const double e = pd_exp(-fabs(eta), tab);
  const double r1 = pd_rcp(1.0 + e);
  const double er = e * r1;
  g = eta >= 0.0 ? r1 : er;
  omg = eta >= 0.0 ? er : r1;
  V = er * r1;
  if (eta != eta) g = omg = V = eta;                 // pd_exp turns a NaN into 0: put it back
}
STK_HD double yrep_poisson_mean(double eta, const double* tab) {
  const double mu = pd_exp(eta, tab);
  return eta != eta ? eta : mu;
}

STK_HD double yrep_normal(double U, double V) { return sqrt(-2.0 * log(U)) * cos(6.283185307179586 * V); }

STK_HD double yrep_logistic(double U, double g, double* mg) {
  if (g != g) return g;
  yrep_gap_cmp(mg, U, g);
  return U < g ? 1.0 : 0.0;
}

STK_HD double yrep_linear(double U, double V, double eta, double sigma) {
  const double y = fma(sigma, yrep_normal(U, V), eta);
  return isfinite(eta) && isfinite(sigma) && isfinite(y) ? y : yrep_nan();
}

// (U, V): call 0 of the element
STK_HD double yrep_poisson(const YrepKey& key, double U, double V, double mu, const double* tab, double* mg) {
  if (!(mu < __builtin_huge_val())) return yrep_nan();   // NaN or +inf
  if (mu < YREP_PTRS_MIN) {
    double k = 0.0, p = pd_exp(-mu, tab), c = p;
    for (int it = 0; it < YREP_SEARCH; ++it) {
      yrep_gap_cmp(mg, U, c);
      if (!(U > c)) break;
      k += 1.0;
      p *= mu / k;
      c += p;
    }
    return k;
  }
  if (mu < YREP_NORMAL_MIN) {
    const double slam = sqrt(mu), loglam = log(mu);
    const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    double res = floor(mu + 0.5);
    for (int j = 0; j < YREP_ATTEMPTS; ++j) {
      if (j > 0) yrep_uv(key, (uint32_t)j, U, V);
      const double Us = U - 0.5, us = 0.5 - fabs(Us);
      const double x = (2.0 * a / us + b) * Us + mu + 0.43;
      const double k = floor(x);
      yrep_gap_floor(mg, x, mu);
      yrep_gap_cmp(mg, us, 0.07);
      if (us >= 0.07) {
        yrep_gap_cmp(mg, V, vr);
        if (V <= vr) {
          res = k;
          break;
        }
      }
      if (k < 0.0) continue;
      yrep_gap_cmp(mg, us, 0.013);
      if (us < 0.013) {
        yrep_gap_cmp(mg, V, us);
        if (V > us) continue;
      }
      const double t1 = k * loglam, t2 = lgamma(k + 1.0);
      const double lhs = log(V) + log(invalpha) - log(a / (us * us) + b), rhs = -mu + t1 - t2;
      if (mg) {
        double sc = 1.0;
        sc = mu > sc ? mu : sc;
        sc = fabs(t1) > sc ? fabs(t1) : sc;
        sc = fabs(t2) > sc ? fabs(t2) : sc;
        yrep_gap(mg, lhs - rhs, sc);
      }
      if (lhs <= rhs) {
        res = k;
        break;
      }
    }
    return res;
  }
  const double x = mu + sqrt(mu) * yrep_normal(U, V) + 0.5;
  yrep_gap_floor(mg, x, mu);
  const double k = floor(x);
  return k > 0.0 ? k : 0.0;
}

// The twin's element: eta -> y_rep (family: STK_LINREG 2, STK_LOGREG 3, STK_POISSON 4; u: log sigma, linear)
STK_HD double yrep_element(int family, uint64_t seed, uint32_t stream, int64_t row, uint32_t s, double eta, double u,
                           const double* tab, double* mg) {
  const YrepKey key = yrep_key(seed, stream, row, s);
  double U, V;
  yrep_uv(key, 0u, U, V);
  if (family == 3) {
    double g, omg, var;
    yrep_logistic_mean(eta, tab, g, omg, var);
    return yrep_logistic(U, g, mg);
  }
  if (family == 4) return yrep_poisson(key, U, V, yrep_poisson_mean(eta, tab), tab, mg);
  return yrep_linear(U, V, eta, exp(u));
}

}  // namespace stk
