// Host check of stark_amd/csrc/psis_math.h against long double: the largest errors of elpd_loo (relative
// to max(1, max |ll|)) and khat (absolute) of psis_row over random rows of several shapes and S, the
// integer tail lengths against their definition, the fit's recovery of a known Pareto shape, and the
// unsmoothed cases; and ps_log1p / ps_log against long double (bar: 4 ulp).
//   g++ -O2 -std=c++17 -o psis_math_check tools/psis_math_check.cpp && ./psis_math_check
// Exits non-zero when elpd_loo is off by more than 1e-12 max(1, max |ll|), khat by more than 1e-9, a tail
// length is wrong, a shape is not recovered or a special case is wrong.  This is also the program to
// build with -fsanitize=address,undefined for a sanitizer run of this arithmetic.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>
#include "../stark_amd/csrc/psis_math.h"

typedef long double ld;

// the definitions of include/stark_hip.h in long double; v sorted ascending
static void ref_row(const std::vector<double>& v, ld out[4]) {
  const int S = (int)v.size();
  const int M = (int)ceill(fminl(0.2L * S, 3.0L * sqrtl((ld)S)));
  const ld mx = v[S - 1];
  std::vector<ld> lr(S);
  for (int k = 0; k < S; ++k) lr[k] = (ld)v[k] - mx;
  ld khat = INFINITY;
  if (M >= 5 && lr[S - 1] - lr[S - M] > 0) {
    const int N = M, Mg = 30 + (int)floorl(sqrtl((ld)N));
    const ld ecut = expl(lr[S - M - 1]);
    std::vector<ld> x(N), l(Mg), th(Mg);
    for (int i = 0; i < N; ++i) x[i] = expl(lr[S - M + i]) - ecut;
    const ld xstar = x[(int)floorl(N / 4.0L + 0.5L) - 1];
    for (int j = 1; j <= Mg; ++j) {
      th[j - 1] = 1 / x[N - 1] + (1 - sqrtl((ld)Mg / (j - 0.5L))) / 3 / xstar;
      ld k = 0;
      for (int i = 0; i < N; ++i) k += log1pl(-th[j - 1] * x[i]);
      k /= N;
      l[j - 1] = N * (logl(-th[j - 1] / k) - k - 1);
    }
    ld that = 0;
    for (int j = 0; j < Mg; ++j) {
      ld s = 0;
      for (int i = 0; i < Mg; ++i) s += expl(l[i] - l[j]);
      that += th[j] / s;
    }
    ld k = 0;
    for (int i = 0; i < N; ++i) k += log1pl(-that * x[i]);
    k /= N;
    const ld sigma = -k / that;
    khat = (k * N + 5) / (N + 10);
    if (std::isfinite((double)khat))
      for (int j = 1; j <= M; ++j)
        lr[S - M + j - 1] = logl(sigma * expm1l(-khat * log1pl(-(j - 0.5L) / M)) / khat + ecut);
  }
  ld s1 = 0, s2 = 0, s3 = 0, m2 = -INFINITY;
  for (int k = 0; k < S; ++k) {
    lr[k] = fminl(lr[k], 0);
    m2 = fmaxl(m2, lr[k] - v[k]);
  }
  for (int k = 0; k < S; ++k) {
    s1 += expl(lr[k]);
    s2 += expl(lr[k] - (ld)v[k] - m2);
    s3 += expl(-(ld)v[k] + (ld)v[0]);
  }
  out[0] = m2 + logl(s2) - logl(s1);
  out[1] = khat;
  out[2] = -(ld)v[0] + logl(s3) - logl((ld)S);
  out[3] = out[2] - out[0];
}

// the fit's pieces on N exceedances (ascending): khat
static double fit(const std::vector<double>& x, const double* tab) {
  const int N = (int)x.size(), Mg = stk::psis_grid(N);
  std::vector<double> l(Mg), th(Mg);
  const double xN = x[N - 1], xstar = x[stk::psis_xstar_index(N) - 1];
  for (int j = 1; j <= Mg; ++j) {
    th[j - 1] = stk::psis_theta(j, Mg, xN, xstar);
    l[j - 1] = stk::psis_profile(th[j - 1], stk::psis_kbar(th[j - 1], x.data(), N), N);
  }
  double that = 0.0;
  for (int j = 0; j < Mg; ++j) that += th[j] * stk::psis_weight(l.data(), Mg, j, tab);
  return stk::psis_khat(stk::psis_kbar(that, x.data(), N), N);
}

int main() {
  static double tab[1024];
  for (int i = 0; i < 1024; ++i) tab[i] = (double)exp2l((ld)i / 1024.0L);
  int bad = 0;
  for (int S = 1; S <= stk::PSIS_SMAX; ++S) {
    const int M = (int)ceill(fminl(0.2L * S, 3.0L * sqrtl((ld)S)));
    if (stk::psis_tail_len(S) != M || M > stk::PSIS_MMAX) ++bad;
    if (M >= 1 && (stk::psis_grid(M) != 30 + (int)floorl(sqrtl((ld)M)) || stk::psis_grid(M) > stk::PSIS_GMAX)) ++bad;
    if (M >= 1 && stk::psis_xstar_index(M) != (int)floorl(M / 4.0L + 0.5L)) ++bad;
  }
  printf("tail lengths, grid sizes, xstar indices wrong: %d\n", bad);
  // ps_log1p over (-1, 1e6] and near 0, ps_log over the whole range, against long double
  double e_l1p = 0, e_log = 0;
  {
    std::mt19937_64 r2(5);
    std::uniform_real_distribution<double> V(0.0, 1.0);
    for (int i = 0; i < 2000000; ++i) {
      const double z = i % 4 == 0 ? -1.0 + V(r2) : (i % 4 == 1 ? exp(-40.0 * V(r2)) * (V(r2) < 0.5 ? -1 : 1)
                                                   : (i % 4 == 2 ? 1e6 * V(r2) * V(r2) : -1.0 + exp(-30.0 * V(r2))));
      const ld rl = log1pl((ld)z);
      if (z > -1.0 && z != 0.0) e_l1p = fmax(e_l1p, (double)fabsl(((ld)stk::ps_log1p(z) - rl) / rl));
      const double u = exp(1400.0 * V(r2) - 700.0);
      const ld rg = logl((ld)u);
      if (fabsl(rg) > 1e-3) e_log = fmax(e_log, (double)fabsl(((ld)stk::ps_log(u) - rg) / rg));
    }
    bad += !(stk::ps_log1p(0.0) == 0.0) + !(stk::ps_log1p(-1.0) == -INFINITY) + !(stk::ps_log1p(-2.0) != stk::ps_log1p(-2.0));
    bad += !(stk::ps_log1p(INFINITY) == INFINITY) + !(stk::ps_log1p(NAN) != stk::ps_log1p(NAN)) + !(stk::ps_log1p(1e-300) == 1e-300);
    bad += !(stk::ps_log(5e-324) == log(5e-324));
    printf("max relative error: ps_log1p %.3e  ps_log %.3e\n", e_l1p, e_log);
  }

  std::mt19937_64 rng(11);
  std::normal_distribution<double> N01(0.0, 1.0);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  double work[stk::PSIS_MMAX + 2 * stk::PSIS_GMAX];
  double e_elpd = 0, e_khat = 0, e_lppd = 0, kmin = INFINITY, kmax = -INFINITY;
  const int sizes[] = {1, 2, 20, 21, 33, 64, 65, 100, 224, 225, 226, 256, 1000, 1023, 1024};
  for (const int S : sizes) {
    for (int rep = 0; rep < 200; ++rep) {
      // ll: a location, a spread from narrow to heavy-tailed, and sometimes a cluster of ties
      const double loc = -50.0 * U(rng), sd = rep % 4 == 0 ? 0.01 : (rep % 4 == 1 ? 0.3 : (rep % 4 == 2 ? 1.5 : 4.0));
      std::vector<double> v(S);
      for (int k = 0; k < S; ++k) {
        const double z = N01(rng);
        v[k] = -(loc - sd * z * z);
      }
      if (rep % 17 == 0 && S > 30)
        for (int k = 0; k < 5; ++k) v[k] = v[5];
      std::sort(v.begin(), v.end());
      double out[4], scale = 1.0;
      ld ref[4];
      stk::psis_row(v.data(), S, tab, work, out);
      ref_row(v, ref);
      for (int k = 0; k < S; ++k) scale = fmax(scale, fabs(v[k]));
      e_elpd = fmax(e_elpd, (double)fabsl(out[0] - ref[0]) / scale);
      e_lppd = fmax(e_lppd, (double)fabsl(out[2] - ref[2]) / scale);
      if (std::isfinite((double)ref[1])) {
        e_khat = fmax(e_khat, (double)fabsl(out[1] - ref[1]));
        kmin = fmin(kmin, out[1]);
        kmax = fmax(kmax, out[1]);
      } else if (!(out[1] == (double)ref[1] || (out[1] != out[1] && ref[1] != ref[1]))) {
        printf("S = %d rep %d: khat %g, long double %g\n", S, rep, out[1], (double)ref[1]);
        ++bad;
      }
      if (S <= 20 && !(out[1] == INFINITY)) ++bad;
      if (S == 1 && !(out[0] == -v[0] && out[2] == -v[0] && out[3] == 0.0)) ++bad;
    }
  }
  printf("max error: elpd_loo %.3e  lppd %.3e (relative to max(1, max |ll|))  khat %.3e (absolute; khat in [%.3f, %.3f])\n",
         e_elpd, e_lppd, e_khat, kmin, kmax);

  // identical draws: a constant tail, no smoothing, elpd_loo = ll
  {
    std::vector<double> v(100, 3.25);
    double out[4];
    stk::psis_row(v.data(), 100, tab, work, out);
    bad += !(out[1] == INFINITY) + !(fabs(out[0] + 3.25) < 1e-13) + !(fabs(out[2] + 3.25) < 1e-13);
  }
  // 20000 generalised Pareto variates of shape k: x = ((1 - u)^-k - 1) / k
  for (const double k : {0.2, 0.7}) {
    std::vector<double> x(20000);
    for (auto& xi : x) xi = expm1(-k * log1p(-U(rng))) / k;
    std::sort(x.begin(), x.end());
    const double got = fit(x, tab);
    printf("shape %.1f from 20000 variates: %.3f\n", k, got);
    bad += !(fabs(got - k) < 0.05);
  }
  printf("special cases wrong: %d\n", bad);
  return (bad || e_l1p > 8.9e-16 || e_log > 8.9e-16 || e_elpd > 1e-12 || e_lppd > 1e-12 || e_khat > 1e-9) ? 1 : 0;
}
