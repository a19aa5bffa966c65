// The Poisson (poisson_log) instantiations of sweep.hip's kernels -- k_sweep, k_sweep2, k_sweep3,
// pass F of the 64-chain sweep (k_gemm_fwd) and k_sweep_reduce -- and their launchers: sweep.hip
// compiled with STK_SWEEP_POISSON_TU, so that the logistic and linear instantiations of sweep.hip
// itself (built with STK_POISSON_OWN_TU, as the Makefile does) are built from the code they always
// were (see the launchers at the end of sweep.hip).
#define STK_SWEEP_POISSON_TU 1
#include "sweep.hip"
