// Instantiations of the bf16-operand per-clone backward conv (lrp_conv_kernel.h through lrp_conv_inst.h, ET = 1, EPI_BWD),
// split across files so the build compiles them in parallel: the GTZAN and VGGish trunk widths
// (backward cin = forward cout, backward cout = forward cin, both padded to 32).
#include "lrp_conv_inst.h"

CONV_TABLE(kTableBwdBfA,
    BWD_SET_BF(32, 32),
    BWD_SET_BF(64, 32),
    BWD_SET_BF(64, 64),
    BWD_SET_BF_P4(64, 64))
