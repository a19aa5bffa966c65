// Host check of stark_amd/csrc/predictive_math.h against long double: the largest relative error of
// pd_exp, pd_rcp and pd_log1p01 over their ranges, and the split of ln 2 / 1024 the header must carry.
//   g++ -O2 -std=c++17 -o predictive_math_check tools/predictive_math_check.cpp && ./predictive_math_check
// Exits non-zero when an error is above 4 ulp (8.9e-16) or a special value is wrong.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <random>
#include "../stark_amd/csrc/predictive_math.h"

int main() {
  static double tab[1024];
  for (int i = 0; i < 1024; ++i) tab[i] = (double)exp2l((long double)i / 1024.0L);
  const long double L = M_LN2l / 1024.0L;
  double hi = (double)L;
  uint64_t b;
  memcpy(&b, &hi, 8);
  b &= ~((1ull << 21) - 1);                               // 32 significant bits
  memcpy(&hi, &b, 8);
  const double lo = (double)(L - (long double)hi);
  printf("L_HI = %.17g  L_LO = %.17g\n", hi, lo);

  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  double e_exp = 0, e_exp_mod = 0, e_rcp = 0, e_l1p = 0;
  for (int i = 0; i < 4000000; ++i) {
    const double x = -745.0 + 1454.0 * U(rng);            // normal results only above -708
    const long double ref = expl((long double)x);
    const double got = stk::pd_exp(x, tab);
    if (x > -708.0) e_exp = fmax(e_exp, (double)fabsl(((long double)got - ref) / ref));
    const double xm = -40.0 + 80.0 * U(rng);
    const long double refm = expl((long double)xm);
    e_exp_mod = fmax(e_exp_mod, (double)fabsl(((long double)stk::pd_exp(xm, tab) - refm) / refm));
    const double u = 1.0 + U(rng);
    e_rcp = fmax(e_rcp, (double)fabsl(((long double)stk::pd_rcp(u) - 1.0L / u) * u));
    const double e = i % 3 == 0 ? U(rng) : (i % 3 == 1 ? exp(-745.0 * U(rng)) : 0.41421356237309503 + 1e-3 * (U(rng) - 0.5));
    const long double rl = log1pl((long double)e);
    if (e > 0) e_l1p = fmax(e_l1p, (double)fabsl(((long double)stk::pd_log1p01(e) - rl) / rl));
  }
  printf("max relative error: pd_exp %.3e (|x| <= 40: %.3e)  pd_rcp %.3e  pd_log1p01 %.3e\n", e_exp, e_exp_mod, e_rcp, e_l1p);
  int bad = 0;
  bad += !(stk::pd_exp(710.0, tab) == INFINITY) + !(stk::pd_exp(1e308, tab) == INFINITY) + !(stk::pd_exp(INFINITY, tab) == INFINITY);
  bad += !(stk::pd_exp(-746.0, tab) == 0.0) + !(stk::pd_exp(-INFINITY, tab) == 0.0) + !(stk::pd_exp(0.0, tab) == 1.0);
  bad += !(stk::pd_log1p01(0.0) == 0.0) + !(stk::pd_log1p01(1.0) == 0.69314718055994531) + !(stk::pd_log1p01(5e-324) == 5e-324);
  printf("special values wrong: %d\n", bad);
  const double bar = 8.9e-16;
  return (bad || e_exp > bar || e_rcp > bar || e_l1p > bar) ? 1 : 0;
}
