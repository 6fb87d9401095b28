// Instantiations of the bf16-operand forward conv (lrp_conv_kernel.h through lrp_conv_inst.h, ET = 1), split across
// files so the build compiles them in parallel.  64-channel trunk (GTZAN blocks 3-4, VGGish blocks 1-2).
#include "lrp_conv_inst.h"

CONV_TABLE(kTableFwdBfB,
    FWD_SET_BF(64, 64))
