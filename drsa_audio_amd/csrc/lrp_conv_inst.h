// Instantiation side of the 3x3 conv kernels: what every conv_*.hip file includes to fill its table.
//
// Contract: a table holds only tiles the dispatch can pick.  Per kernel set (CIN, COUT, NG, AMODE,
// EPI, ET, PW) that is the wide tile of the tile rule (lrp_conv_config.h wide_tile_w(), entered for
// the maps with W >= kWideW) and the 8 x 8 tile (entered for the narrower ones); CONV_FAMILY emits
// exactly these two.  A hand-written CONV_ENTRY / CONV_ENTRY_WIDE must name the same tiles (it may
// choose its own chunk size CIC per tile, conv_bwd_a.hip): lrp_conv.hip's find() takes the first
// entry of the key and width class and never looks at the tile.  conv_small.hip's 4 x 8 tiles are
// picked by small_tile() in place of an 8 x 8 entry and are searched by nothing else.
#pragma once
#include "lrp_conv_kernel.h"
#include "lrp_conv_table.h"

namespace drsa_conv {

// One table entry from the eleven template arguments of ConvCfg / conv3x3_kernel, in their order:
// CIN, COUT, TH, TW, MW, CIC, NG, AMODE, EPI, ET, PW
template <int... P>
constexpr Entry conv_entry(int wide) {
  static_assert(sizeof...(P) == 11, "CONV_ENTRY takes every ConvCfg parameter");
  constexpr int p[] = {P...};
  return Entry{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8],
               conv3x3_kernel<P...>, ConvCfg<P...>::lds_floats * sizeof(float), p[9], p[10], wide};
}
// an entry for the maps narrower than kWideW (8 x 8; conv_small.hip: 4 x 8) / for the wider ones
#define CONV_ENTRY(CIN, COUT, TH, TW, MW, CIC, NG, AM, EP, ET, PW) \
  drsa_conv::conv_entry<CIN, COUT, TH, TW, MW, CIC, NG, AM, EP, ET, PW>(0)
#define CONV_ENTRY_WIDE(CIN, COUT, TH, TW, MW, CIC, NG, AM, EP, ET, PW) \
  drsa_conv::conv_entry<CIN, COUT, TH, TW, MW, CIC, NG, AM, EP, ET, PW>(1)

// tile family: the rule's wide tile and the 8 x 8 tile (one instantiation where the wide tile is 8 x 8)
#define CONV_FAMILY(CIN, COUT, CIC, NG, AM, EP, ET, PW)                                             \
  CONV_ENTRY_WIDE(CIN, COUT, 8, drsa_conv::wide_tile_w(EP, ET, CIN, COUT),                          \
                  drsa_conv::tile_mw(drsa_conv::wide_tile_w(EP, ET, CIN, COUT)), CIC, NG, AM, EP, ET, PW), \
  CONV_ENTRY(CIN, COUT, 8, 8, 4, CIC, NG, AM, EP, ET, PW)

// forward: every denominator set count and both epilogues (2x2 pool, ReLU only)
#define FWD_SET_ET(CIN, COUT, CIC, ET)                                                      \
  CONV_FAMILY(CIN, COUT, CIC, 1, drsa_conv::A_DENSE, drsa_conv::EPI_FWD_POOL, ET, 2),        \
  CONV_FAMILY(CIN, COUT, CIC, 2, drsa_conv::A_DENSE, drsa_conv::EPI_FWD_POOL, ET, 2),        \
  CONV_FAMILY(CIN, COUT, CIC, 3, drsa_conv::A_DENSE, drsa_conv::EPI_FWD_POOL, ET, 2),        \
  CONV_FAMILY(CIN, COUT, CIC, 1, drsa_conv::A_DENSE, drsa_conv::EPI_FWD_RELU, ET, 2),        \
  CONV_FAMILY(CIN, COUT, CIC, 2, drsa_conv::A_DENSE, drsa_conv::EPI_FWD_RELU, ET, 2),        \
  CONV_FAMILY(CIN, COUT, CIC, 3, drsa_conv::A_DENSE, drsa_conv::EPI_FWD_RELU, ET, 2)
#define FWD_SET(CIN, COUT, CIC) FWD_SET_ET(CIN, COUT, CIC, 0)
// bf16-operand forward (ET = 1, 16-channel chunks)
#define FWD_SET_BF(CIN, COUT) FWD_SET_ET(CIN, COUT, 16, 1)

// 2x4-pool forward (VGGish block 1, create_model.py:61): fp32 and bf16 operands
#define FWD_SET_P4(CIN, COUT, CIC, ET)                                                      \
  CONV_FAMILY(CIN, COUT, CIC, 1, drsa_conv::A_DENSE, drsa_conv::EPI_FWD_POOL, ET, 4),        \
  CONV_FAMILY(CIN, COUT, CIC, 2, drsa_conv::A_DENSE, drsa_conv::EPI_FWD_POOL, ET, 4),        \
  CONV_FAMILY(CIN, COUT, CIC, 3, drsa_conv::A_DENSE, drsa_conv::EPI_FWD_POOL, ET, 4)

// fp32 per-clone backward: one or two weight sets, dense and 2x2-pool-sparse g
#define BWD_SET(CIN, COUT, CIC)                                                             \
  CONV_FAMILY(CIN, COUT, CIC, 1, drsa_conv::A_DENSE, drsa_conv::EPI_BWD, 0, 2),              \
  CONV_FAMILY(CIN, COUT, CIC, 2, drsa_conv::A_DENSE, drsa_conv::EPI_BWD, 0, 2),              \
  CONV_FAMILY(CIN, COUT, CIC, 1, drsa_conv::A_POOLSPARSE, drsa_conv::EPI_BWD, 0, 2),         \
  CONV_FAMILY(CIN, COUT, CIC, 2, drsa_conv::A_POOLSPARSE, drsa_conv::EPI_BWD, 0, 2)

// bf16-operand per-clone backward (ET = 1), dense and pool-sparse g, one weight set
#define BWD_SET_BF(CIN, COUT)                                                               \
  CONV_FAMILY(CIN, COUT, 16, 1, drsa_conv::A_DENSE, drsa_conv::EPI_BWD, 1, 2),               \
  CONV_FAMILY(CIN, COUT, 16, 1, drsa_conv::A_POOLSPARSE, drsa_conv::EPI_BWD, 1, 2)
// bf16-operand per-clone backward with g at (2,4)-pool resolution (VGGish block 1)
#define BWD_SET_BF_P4(CIN, COUT) CONV_FAMILY(CIN, COUT, 16, 1, drsa_conv::A_POOLSPARSE, drsa_conv::EPI_BWD, 1, 4)

// A conv_*.hip file's entries and its table (listed in lrp_conv.hip's DRSA_CONV_TABLES)
#define CONV_TABLE(NAME, ...)                                                                     \
  namespace drsa_conv {                                                                           \
  static const Entry NAME##_e[] = {__VA_ARGS__};                                                  \
  extern const Table NAME = {NAME##_e, (int)(sizeof(NAME##_e) / sizeof(NAME##_e[0]))};            \
  }

}  // namespace drsa_conv
