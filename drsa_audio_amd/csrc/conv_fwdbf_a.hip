// Instantiations of the bf16-operand forward conv (lrp_conv_kernel.h through lrp_conv_inst.h, ET = 1), split across
// files so the build compiles them in parallel.  GTZAN trunk widths (create_model.py:100-137).
#include "lrp_conv_inst.h"

CONV_TABLE(kTableFwdBfA,
    FWD_SET_BF(32, 32),
    FWD_SET_BF(32, 64))
