// The Student-t (student_t) instantiations of sweep.hip's kernels -- k_sweep, k_sweep2, k_sweep3, pass F of the 64-chain sweep (k_gemm_fwd) and the reduce (k_sweep_reduce<STK_STUDENT>)
// and their launchers: sweep.hip compiled with STK_SWEEP_STUDENT_TU, by the mechanism of sweep_pois.hip, so
// that the kernels of the other families are built from the code they always were.
#define STK_SWEEP_STUDENT_TU 1
#include "sweep.hip"
