// Instantiations of the 3x3 conv kernel (lrp_conv_kernel.h through lrp_conv_inst.h), split across files so the
// build compiles them in parallel.
#include "lrp_conv_inst.h"

// backward into 64 channels, written out per tile because the two tiles take their own chunk sizes:
// the rule's wide tile (8 x 16: the 8 x 32 tile with either chunk size spills) and the 8 x 8 tile,
// 8-channel chunks except the 8 x 8 tiles of the backward from 128 channels (16).  At W >= 32
// (VGGish blocks 1-2) the 8-channel chunk takes 124 VGPRs, 4 waves/SIMD instead of 3 (16-channel
// chunks: 148): conv_bwd:features.3 0.75 -> 0.66 ms, .7 0.107 -> 0.092 ms, fp32 standard LRP
// 7.94k -> 8.11k samples/s.
#ifndef DRSA_CONV_CIC_BWD64
#define DRSA_CONV_CIC_BWD64 8
#endif
#ifndef DRSA_CONV_CIC_BWD64_T8
#define DRSA_CONV_CIC_BWD64_T8 8
#endif
#define CONV_FAMILY_BWD64(CIN, NG, AM, C8)                                                   \
  CONV_ENTRY_WIDE(CIN, 64, 8, 16, 8, DRSA_CONV_CIC_BWD64, NG, AM, drsa_conv::EPI_BWD, 0, 2), \
  CONV_ENTRY(CIN, 64, 8, 8, 4, C8, NG, AM, drsa_conv::EPI_BWD, 0, 2)
// C8: the chunk of the 8 x 8 tile (64 -> 64: 8, 0.212 -> 0.193 ms; 128 -> 64: 16, 0.053 vs 0.057 ms)
#define BWD_SET64(CIN, C8)                                \
  CONV_FAMILY_BWD64(CIN, 1, drsa_conv::A_DENSE, C8),      \
  CONV_FAMILY_BWD64(CIN, 2, drsa_conv::A_DENSE, C8),      \
  CONV_FAMILY_BWD64(CIN, 1, drsa_conv::A_POOLSPARSE, C8), \
  CONV_FAMILY_BWD64(CIN, 2, drsa_conv::A_POOLSPARSE, C8)

CONV_TABLE(kTableBwdA,
    BWD_SET64(128, 16),
    BWD_SET64(64, DRSA_CONV_CIC_BWD64_T8),
    // the (2,4) pool backward folded into the staging (VGGish block 1 at W = 256): the wide tile only
    // (fp32 2 x 4 cells need tiles of whole float4 cell groups, so narrower maps have no kernel)
    CONV_ENTRY_WIDE(64, 64, 8, 16, 8, DRSA_CONV_CIC_BWD64, 1, drsa_conv::A_POOLSPARSE, drsa_conv::EPI_BWD, 0, 4))
