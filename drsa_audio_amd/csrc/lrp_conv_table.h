// The dispatch tables of the 3x3 conv kernels: what lrp_conv.hip searches and the conv_*.hip files
// fill (lrp_conv_inst.h).  No kernel code here.
#pragma once
#include "lrp_conv.h"
#include "lrp_conv_config.h"

namespace drsa_conv {

typedef void (*KernFn)(ConvArgs);

struct Entry {
  int cin_p, cout_p, th, tw, mw, cic, ng, amode, epi;
  KernFn fn;
  size_t lds;
  int et = 0;     // operand type (ConvCfg ET)
  int pw = 2;     // pool window width (ConvCfg PW)
  int wide = 0;   // width class served: 1 = maps with W >= kWideW, 0 = narrower ones
};

struct Table {
  const Entry* entries;
  int n;
};

}  // namespace drsa_conv
