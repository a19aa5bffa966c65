// Host check of stark_amd/csrc/student_math.h against long double: the largest relative error of st_log1p over
// 0, the subnormals, 1e-300 .. 1e300 in decade steps (nine mantissas each), neighbourhoods of every branch point
// of the implementation (sqrt(2) - 1, 1, the w at which 1 + w passes sqrt(2) 2^k and 2^k, 2^53 where 1 + w = w)
// and two million log-uniform arguments; and the special cases (0, +inf, NaN, w -> 0).
//   g++ -O2 -std=c++17 -o student_math_check tools/student_math_check.cpp && ./student_math_check
// Prints the largest error in units of 2^-53 and exits non-zero when it passes BAR (twice the largest found
// when the function was written: 2.9) or a special case is wrong.  This is also the program to build with
// -fsanitize=address,undefined for a sanitizer run of this arithmetic.
#include <cmath>
#include <cstdio>
#include <random>
#include "../stark_amd/csrc/student_math.h"

typedef long double ld;
static const double BAR = 5.8;   // units of 2^-53 relative

static double worst = 0.0, worst_at = 0.0;
static void probe(double w) {
  if (!(w > 0.0) || !std::isfinite(w)) return;
  const ld ref = log1pl((ld)w);
  const double e = (double)(fabsl((ld)stk::st_log1p(w) - ref) / ref) * 9007199254740992.0;
  if (e > worst) worst = e, worst_at = w;
}
static void around(double w) {   // w and 40 neighbours on either side
  double a = w, b = w;
  probe(w);
  for (int i = 0; i < 40; ++i) {
    a = nextafter(a, 0.0);
    b = nextafter(b, INFINITY);
    probe(a);
    probe(b);
  }
}

int main() {
  int bad = 0;
  bad += !(stk::st_log1p(0.0) == 0.0) + !(stk::st_log1p(INFINITY) == INFINITY) + !(stk::st_log1p(NAN) != stk::st_log1p(NAN));
  bad += !(stk::st_log1p(5e-324) == 5e-324) + !(stk::st_log1p(1e-310) == 1e-310) + !(stk::st_log1p(1e-300) == 1e-300);
  bad += !(stk::st_log1p(1.7976931348623157e308) == (double)log1pl(1.7976931348623157e308L));
  for (int dec = -323; dec <= 308; ++dec)
    for (int mant = 1; mant <= 9; ++mant) probe((double)((ld)mant * powl(10.0L, (ld)dec)));
  around(0.41421356237309503);
  around(1.0);
  around(9007199254740992.0);
  around(4503599627370496.0);
  for (int k = 0; k <= 1023; ++k) {
    around((double)(ldexpl(1.0L, k) - 1.0L));                        // 1 + w passes 2^k
    around((double)(ldexpl(1.41421356237309504880L, k) - 1.0L));     // 1 + w passes sqrt(2) 2^k: m wraps, k steps
  }
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  for (int i = 0; i < 2000000; ++i) {
    probe(exp(1400.0 * U(rng) - 700.0));
    probe(exp(12.0 * U(rng) - 6.0));       // the body of the range a fit meets
  }
  printf("st_log1p: largest relative error %.3f x 2^-53 at w = %.17g; special cases wrong: %d\n", worst, worst_at, bad);
  return (bad || worst > BAR) ? 1 : 0;
}
