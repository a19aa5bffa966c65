// The Student-t (student_t) instantiations of k_sweep16w
// and their launcher: sweep16w.hip compiled with STK_SWEEP16W_STUDENT_TU, by the mechanism of sweep16w_pois.hip, so
// that the kernels of the other families are built from the code they always were.
#define STK_SWEEP16W_STUDENT_TU 1
#include "sweep16w.hip"
