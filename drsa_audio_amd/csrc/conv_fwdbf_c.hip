// Instantiations of the bf16-operand forward conv (lrp_conv_kernel.h through lrp_conv_inst.h, ET = 1), split across
// files so the build compiles them in parallel.  VGGish-BN blocks 3-5 (100 channels pad to 128).
#include "lrp_conv_inst.h"

CONV_TABLE(kTableFwdBfC,
    FWD_SET_BF(64, 128),
    FWD_SET_BF(128, 128))
