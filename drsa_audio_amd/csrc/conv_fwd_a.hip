// Instantiations of the 3x3 conv kernel (lrp_conv_kernel.h through lrp_conv_inst.h), split across files so the
// build compiles them in parallel.
#include "lrp_conv_inst.h"

#ifndef DRSA_CONV_CIC_FWD32
#define DRSA_CONV_CIC_FWD32 8
#endif

CONV_TABLE(kTableFwdA,
    FWD_SET(1, 32, 1),
    FWD_SET(32, 32, DRSA_CONV_CIC_FWD32))
