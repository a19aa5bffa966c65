// The negative-binomial (neg_binomial_2_log) instantiations of sweep.hip's kernels -- k_sweep, k_sweep2, k_sweep3, pass F of the 64-chain sweep (k_gemm_fwd) -- and the family's reduce (k_sweep_reduce_nb)
// and their launchers: sweep.hip compiled with STK_SWEEP_NEGBIN_TU, by the mechanism of sweep_pois.hip, so
// that the logistic, linear and Poisson kernels are built from the code they always were.
#define STK_SWEEP_NEGBIN_TU 1
#include "sweep.hip"
