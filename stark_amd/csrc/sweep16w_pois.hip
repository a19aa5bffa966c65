// The Poisson (poisson_log) instantiations of k_sweep16w and their launcher: sweep16w.hip compiled
// with STK_SWEEP16W_POISSON_TU, so that the logistic and linear instantiations of sweep16w.hip
// itself (built with STK_POISSON_OWN_TU, as the Makefile does) are built from the code they always
// were (see the launchers at the end of sweep16w.hip).
#define STK_SWEEP16W_POISSON_TU 1
#include "sweep16w.hip"
