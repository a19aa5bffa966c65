// The negative-binomial (neg_binomial_2_log) instantiations of k_sweep16
// and their launchers: sweep16.hip compiled with STK_SWEEP16_NEGBIN_TU, by the mechanism of sweep16_pois.hip, so
// that the logistic, linear and Poisson kernels are built from the code they always were.
#define STK_SWEEP16_NEGBIN_TU 1
#include "sweep16.hip"
