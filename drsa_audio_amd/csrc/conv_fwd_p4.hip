// Instantiations of the 3x3 conv kernel with the 2x4 max-pool fused into the forward epilogue
// (lrp_conv_kernel.h through lrp_conv_inst.h, PW = 4): VGGish-BN block 1 (64 -> 64 at 128x256, pool_kernels[0] = (2,4),
// create_model.py:61), fp32 (CIC 8) and bf16 operands.
#include "lrp_conv_inst.h"

CONV_TABLE(kTableFwdP4,
    FWD_SET_P4(64, 64, 8, 0),
    FWD_SET_P4(64, 64, 16, 1))
