// Instantiations of the 3x3 conv kernel (lrp_conv_kernel.h through lrp_conv_inst.h), split across files so the
// build compiles them in parallel.  VGGish-BN blocks 3-5 backward (128 -> 128 padded).
#include "lrp_conv_inst.h"

CONV_TABLE(kTableBwdC,
    BWD_SET(128, 128, 8))
