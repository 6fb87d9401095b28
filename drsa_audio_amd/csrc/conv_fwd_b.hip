// Instantiations of the 3x3 conv kernel (lrp_conv_kernel.h through lrp_conv_inst.h), split across files so the
// build compiles them in parallel.
#include "lrp_conv_inst.h"

CONV_TABLE(kTableFwdB,
    FWD_SET(32, 64, 8))
