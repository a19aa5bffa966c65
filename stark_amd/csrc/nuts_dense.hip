// The dense_e (full inverse metric) instantiations of k_nuts_step and their launchers: nuts.hip
// compiled with STK_NUTS_DENSE_TU, so that the diagonal instantiations of nuts.hip itself are
// built from the code they always were (see the launchers at the end of nuts.hip).
#define STK_NUTS_DENSE_TU 1
#include "nuts.hip"
