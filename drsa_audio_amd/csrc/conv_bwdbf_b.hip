// Instantiations of the bf16-operand per-clone backward conv (see conv_bwdbf_a.hip): 128-wide g.
#include "lrp_conv_inst.h"

CONV_TABLE(kTableBwdBfB,
    BWD_SET_BF(128, 64),
    BWD_SET_BF(128, 128))
