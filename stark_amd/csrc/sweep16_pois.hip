// The Poisson (poisson_log) instantiations of k_sweep16 and their launcher: sweep16.hip compiled
// with STK_SWEEP16_POISSON_TU, so that the logistic and linear instantiations of sweep16.hip itself
// (built with STK_POISSON_OWN_TU, as the Makefile does) are built from the code they always were
// (see the launchers at the end of sweep16.hip).
#define STK_SWEEP16_POISSON_TU 1
#include "sweep16.hip"
