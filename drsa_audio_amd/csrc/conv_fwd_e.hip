// Instantiations of the 3x3 conv kernel (lrp_conv_kernel.h through lrp_conv_inst.h), split across files so the
// build compiles them in parallel.  VGGish-BN blocks 3-5 (100/128 -> 128 channels padded).
#include "lrp_conv_inst.h"

#ifndef DRSA_CONV_CIC_FWD128_128
#define DRSA_CONV_CIC_FWD128_128 4   // 8 x 8 tiles at 3 waves/SIMD (168 VGPRs): conv_fwd:features.12 0.106 -> 0.092 ms
#endif

CONV_TABLE(kTableFwdE,
    FWD_SET(128, 128, DRSA_CONV_CIC_FWD128_128))
