// Instantiations of the 3x3 conv kernel (lrp_conv_kernel.h through lrp_conv_inst.h), split across files so the
// build compiles them in parallel.  VGGish-BN first layer (1 -> 64, create_model.py:100-137).
#include "lrp_conv_inst.h"

CONV_TABLE(kTableFwdD,
    FWD_SET(1, 64, 1))
