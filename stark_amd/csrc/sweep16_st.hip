// The Student-t (student_t) instantiations of k_sweep16
// and their launcher: sweep16.hip compiled with STK_SWEEP16_STUDENT_TU, by the mechanism of sweep16_pois.hip, so
// that the kernels of the other families are built from the code they always were.
#define STK_SWEEP16_STUDENT_TU 1
#include "sweep16.hip"
