// The negative-binomial (neg_binomial_2_log) instantiations of k_sweep16w
// and their launchers: sweep16w.hip compiled with STK_SWEEP16W_NEGBIN_TU, by the mechanism of sweep16w_pois.hip, so
// that the logistic, linear and Poisson kernels are built from the code they always were.
#define STK_SWEEP16W_NEGBIN_TU 1
#include "sweep16w.hip"
