// Configuration of the 3x3 conv kernel (lrp_conv_kernel.h): the build knobs, the tile rule and
// ConvCfg, the compile-time geometry of one instantiation.  Host and device code both include this;
// nothing here needs the kernel.
#pragma once
#include <stddef.h>

#ifndef DRSA_CONV_PD_BWD
#define DRSA_CONV_PD_BWD 2
#endif
#ifndef DRSA_CONV_BWD_ES
#define DRSA_CONV_BWD_ES 1
#endif
#ifndef DRSA_CONV_BWD_WPE
#define DRSA_CONV_BWD_WPE 3
#endif
// small-chunk rule backward (SMALL_BWD: GTZAN conv_bwd:features.3 / .6): its MFMA operand ring is
// pinned (a sched_barrier per k-step keeps step k + PD's LDS reads ahead of step k's MFMAs; the
// scheduler otherwise sinks each read next to its MFMA behind an lgkmcnt(0) wait) at distance 3.
// Measured in the step (gpurun_out/r6j, r6k): features.3 1.373-1.383 -> 1.335 ms, .6 0.632 ->
// 0.613; pinning the forwards or the wider backwards as well made them 2-6 % slower.
#ifndef DRSA_CONV_PIN_SMALL
#define DRSA_CONV_PIN_SMALL 1
#endif
#ifndef DRSA_CONV_PD_SMALL
#define DRSA_CONV_PD_SMALL 3
#endif
#ifndef DRSA_CONV_SMALL_WPE
#define DRSA_CONV_SMALL_WPE 4      // small-chunk backward: 4 workgroups (16 waves) per CU
#endif
#ifndef DRSA_CONV_SMALL_ES
#define DRSA_CONV_SMALL_ES 2       // small-chunk backward: epilogue in 2 channel passes of 16
#endif
#ifndef DRSA_CONV_PRE_D
#define DRSA_CONV_PRE_D 0
#endif
#ifndef DRSA_CONV_PRE_N
#define DRSA_CONV_PRE_N 64
#endif
#ifndef DRSA_CONV_BF_WPE
#define DRSA_CONV_BF_WPE 2
#endif
#ifndef DRSA_CONV_FWD_WPE_128
#define DRSA_CONV_FWD_WPE_128 3    // 8 x 8-tile forwards into 128 channels with 4-channel chunks: 2 -> 3 waves/SIMD
#endif
#ifndef DRSA_CONV_FWD_WPE_WIDE
#define DRSA_CONV_FWD_WPE_WIDE 3   // forwards into 64 channels (CIC <= 8, NG <= 2): 1 -> 3 conv_fwd:features.6 0.361 -> 0.343 ms
#endif
#ifndef DRSA_CONV_FWD_WPE
#define DRSA_CONV_FWD_WPE 3
#endif
#ifndef DRSA_CONV_FWD128_TW
#define DRSA_CONV_FWD128_TW 8    // fp32 forward into 128 channels at W >= 32: tile width (32, 16 or 8)
#endif

namespace drsa_conv {

constexpr int kThreads = 256;

template <int V, int M>
constexpr int round_up() { return (V + M - 1) / M * M; }

// halo row stride: the 32 lanes of one ds_read_b32 group read a (16/MW x 2) grid of
// MW*2-pixel runs; RS = 16 (mod 32) for 2 rows x 16, RS = 8 (mod 32) for 4 rows x 8 puts the
// runs on disjoint banks.
constexpr int halo_stride(int hx, int mw) {
  int r = hx;
  const int want = (mw == 8) ? 16 : 8;
  while (r % 32 != want) ++r;
  return r;
}

enum AMode { A_DENSE = 0, A_POOLSPARSE = 1 };
enum Epi { EPI_FWD_POOL = 0, EPI_FWD_RELU = 1, EPI_BWD = 2 };

// Tile shape per direction, channel width and map width (measured choices; variant builds change
// them with -D, scripts/build_variant.py).  Every tile is 8 rows high; a map at least kWideW wide
// takes the wide tile (wide_tile_w() columns), a narrower one the 8 x 8 tile; tile_mw() gives the
// MW of either.  The tables hold exactly these two tiles per kernel set (lrp_conv_inst.h), and the
// dispatch (lrp_conv.hip find()) only picks the width class.
// * W >= 32: 8 x 32 tiles, except 8 x 16 for the fp32 forward into 64 channels (half the
//   accumulators: 2 waves/SIMD instead of 1; GTZAN conv_fwd:features.6 0.391 -> 0.356 ms, VGGish
//   features.3 1.43 -> 1.36 ms), the fp32 backward into 64 channels (the 8 x 32 tile with 16-channel
//   chunks spills 91-115 VGPRs) and into 128 channels (VGGish features.17: the 8 x 32 tile spills
//   358-435 VGPRs; 0.291 -> 0.101 ms); the fp32 forward into 128 channels on 8 x 8 tiles (4 times the
//   workgroups at 3 waves/SIMD instead of 1: VGGish conv_fwd:features.17 0.318 -> 0.175 ms, .14 0.168
//   -> 0.100 ms, fp32 standard LRP 7.6k -> 8.0k samples/s; 8 x 16: 0.189 / 0.101 ms);
// * 8 < W < 32: 8 x 8 tiles (more workgroups for the small layers: conv_fwd:features.9 0.287 -> 0.266
//   ms, conv_bwd 0.218 -> 0.214 at B = 512);  W <= 8: 8 x 8.
// Measured slower and dropped: 16-row tiles, 32-channel fp32 forwards / backwards on 8 x 16 tiles.
constexpr int kWideW = 32;
constexpr int wide_tile_w(int epi, int et, int cin_p, int cout_p, int fwd128_tw = DRSA_CONV_FWD128_TW) {
  if (et != 0) return 32;
  if (epi != EPI_BWD) return cout_p == 128 ? fwd128_tw : cout_p == 64 ? 16 : 32;
  return (cout_p == 64 && cin_p <= 128) || cout_p == 128 ? 16 : 32;
}
constexpr int tile_mw(int tw) { return tw == 8 ? 4 : 8; }

// halo column c (pixel tx0 - 1 + c) lives at LDS column c + XO, so the tile interior starts
// 16-byte aligned (float4 staging stores) and pool cells cover aligned float2 pairs.
constexpr int XO = 3;

// bf16 halo row stride in 16-byte pixels: >= hx and 8 (mod 16), so the two rows of a 2x2-window
// run of 16 lanes land on disjoint bank halves (ds_read_b128)
constexpr int bf_stride(int hx) {
  int r = hx;
  while (r % 16 != 8) ++r;
  return r;
}

// ET (element type of the MFMA operands): 0 = fp32 (v_mfma_f32_32x32x2_f32, the exact k-ordered
// chain), 1 = bf16 (v_mfma_f32_32x32x16_bf16, forward only: conv inputs and weights rounded to
// bf16 when staged, fp32 accumulation, fp32 outputs).  The bf16 chunk is 16 input channels = one
// tap per MFMA (k = tap * 16 + ci); its halo is pixel-major, 8 channels per 16-byte pixel slot.
template <int CIN, int COUT, int TH, int TW, int MW, int CIC, int NG, int AMODE, int EPI, int ET = 0, int PW = 2>
struct ConvCfg {
  static constexpr int CIN_ = CIN, COUT_ = COUT, TH_ = TH, TW_ = TW, MW_ = MW, CIC_ = CIC, NG_ = NG;
  static constexpr int AMODE_ = AMODE, EPI_ = EPI;
  static constexpr bool BF = ET == 1;
  static constexpr int HY = TH + 2, HX = TW + 2;
  static constexpr int HXB = bf_stride(HX);
  // bf16 staging: halo [2 channel halves][HY][HXB] x 16 B, weights [NG][9 taps][2][COUT] x 16 B
  static constexpr size_t bf_halo_floats = (size_t)2 * HY * HXB * 4;
  static constexpr size_t bf_w_floats = (size_t)NG * 9 * 2 * COUT * 4;
  static constexpr int RS = halo_stride(HX + XO, MW);
  static constexpr int PLANE_RAW = HY * RS;
  static constexpr int PLANE = PLANE_RAW + ((PLANE_RAW % 32) == 0 ? 4 : 0);
  // M-tile = the 32 pixels of one MFMA B operand: window-major 2x2 pool windows (MTH = 16/MW rows
  // x 2*MW)
  static constexpr int MTW = 2 * MW;
  static constexpr int MTH = 32 / MTW;
  static constexpr int MTX = TW / MTW;     // M-tiles per tile row
  static constexpr int MT = (TH / MTH) * MTX;
  static constexpr int NT = COUT / 32;
  static constexpr int WM = MT >= 4 ? 4 : MT;
  static constexpr int WN = (4 / WM) < NT ? (4 / WM) : NT;   // waves >= WM*WN idle (tiny layers)
  static constexpr int MPW = MT / WM;      // m-tiles per wave
  static constexpr int NPW = NT / WN;      // n-tiles per wave
  static constexpr int KC = 9 * CIC;
  static constexpr int KCP = round_up<KC, 2>();
  static constexpr int NCHUNK = CIN / CIC;
  static constexpr int TWP = (TW == 32) ? 48 : TW;          // epilogue tile row stride (conflict-free writes)
  // backward epilogue in ES channel passes (halves the epilogue LDS and registers; WN == 1 only)
  // small-chunk rule backward (CIC <= 8, 32 output channels): 24.6 KB LDS and <= 128 VGPRs, so
  // 4 workgroups (16 waves) per CU
  static constexpr bool SMALL_BWD = EPI == EPI_BWD && NG == 1 && CIC <= 8 && COUT <= 32;
  static constexpr int ES = (EPI == EPI_BWD && WN == 1) ? (SMALL_BWD ? DRSA_CONV_SMALL_ES : DRSA_CONV_BWD_ES) : 1;
  static constexpr int TCH = WN * 32 / ES;                     // channels staged per epilogue pass
  static constexpr size_t staging_floats =
      BF ? bf_halo_floats + bf_w_floats : (size_t)CIC * PLANE + (size_t)NG * KCP * COUT;
  static constexpr size_t epi_floats = (size_t)TCH * TH * TWP;
  static constexpr size_t lds_floats = staging_floats > epi_floats ? staging_floats : epi_floats;
  // minimum waves per SIMD the register allocation must allow (1 block = 1 wave per SIMD)
  static constexpr int WPE = BF ? (COUT <= 64 ? DRSA_CONV_BF_WPE : 1)
                             : (EPI == EPI_BWD && NG == 1) ? (SMALL_BWD ? DRSA_CONV_SMALL_WPE : DRSA_CONV_BWD_WPE)
                             : (EPI != EPI_BWD && CIC <= 8 && COUT <= 32 && NG <= 2 ? DRSA_CONV_FWD_WPE
                                : EPI != EPI_BWD && CIC <= 8 && NG <= 2 && COUT == 64 ? DRSA_CONV_FWD_WPE_WIDE
                                : EPI != EPI_BWD && CIC <= 4 && NG <= 2 && COUT == 128 && TW == 8 ? DRSA_CONV_FWD_WPE_128 : 1);
  // operand prefetch distance of the MFMA loop (k-steps)
  static constexpr bool PIN = SMALL_BWD && DRSA_CONV_PIN_SMALL;
  static constexpr int PD = PIN ? DRSA_CONV_PD_SMALL : DRSA_CONV_PD_BWD > 0 && EPI >= EPI_BWD ? DRSA_CONV_PD_BWD : 1;
  static_assert(TH % MTH == 0 && TW % MTW == 0, "tile must be a multiple of the M-tile");
  static_assert(COUT % 32 == 0, "COUT must be padded to 32");
  static_assert(CIN % CIC == 0, "CIN must be a multiple of the chunk");
  static_assert(MT % WM == 0 && NT % WN == 0 && WM * WN <= 4, "wave split");
  static_assert(!BF || (CIC == 16 && (EPI < EPI_BWD ? AMODE == A_DENSE : EPI == EPI_BWD)),
                "bf16: 16-channel chunks; dense forward, or the per-clone backward (dense or pool-sparse g)");
  static_assert(PW == 2 || (PW == 4 && (EPI == EPI_FWD_POOL || (EPI == EPI_BWD && AMODE == A_POOLSPARSE &&
                                                                  (ET == 1 || TW % 16 == 0)))),
                "2x4 pool windows: the forward pool epilogue, or the backward's pool-sparse staging (fp32: "
                "tiles of whole float4 cell groups)");
  static constexpr int PW_ = PW;
};

}  // namespace drsa_conv
