// The MFMA loops of the 3x3 conv kernel (lrp_conv_kernel.h) over one staged chunk: fp32 and bf16.
#pragma once
#include "common.h"
#include "lrp_conv_config.h"

namespace drsa_conv {

// ---- MFMA over one staged chunk.  k = k0 + h (h = lane half) with k = ci*9 + tap: the halo
//      offset pattern repeats every 9 k-steps (two channels), so every LDS read in the fully
//      unrolled loop is a per-lane base register + immediate.  Operands of step k0 are read
//      one step ahead (explicit software pipeline). ----
template <class Cfg, int PD = 1>
__device__ __forceinline__ void mfma_chunk(const float* halo, const float* wl, const int (&pix_off)[Cfg::MPW],
                                           int lane, int wn, f32x16 (&acc)[Cfg::NG_][Cfg::MPW][Cfg::NPW]) {
  constexpr int MPW = Cfg::MPW, NPW = Cfg::NPW, NG = Cfg::NG_, COUT = Cfg::COUT_;
  constexpr int KC = Cfg::KC, KCP = Cfg::KCP, PLANE = Cfg::PLANE, RS = Cfg::RS, EPI = Cfg::EPI_;
  const int h = lane >> 5;
  // Halo offset of k = k0 + h (k = ci * 9 + tap):  off(k0) + h * delta(k0 % 9), with off(k0) a
  // compile-time immediate (the loop is unrolled) and delta one of three values: +1 inside a tap
  // row, RS - 2 from the row's last tap to the next row, PLANE - 2 RS - 2 from tap 8 to the next
  // channel's tap 0.  So each m-tile needs three per-lane base registers (pix_off + h * delta)
  // instead of one per k-step pattern, and every operand read is base + immediate.
  constexpr int DLT[3] = {1, RS - 2, PLANE - 2 * RS - 2};
  int xb[MPW][3];
#pragma unroll
  for (int u = 0; u < MPW; ++u)
#pragma unroll
    for (int t = 0; t < 3; ++t) xb[u][t] = pix_off[u] + h * DLT[t];
  auto read_x = [&](int k0, float (&xv)[MPW]) {
    const int r9 = k0 % 9;
    const int off = (k0 / 9) * PLANE + (r9 / 3) * RS + (r9 % 3);
    const int t = (r9 == 8) ? 2 : (r9 == 2 || r9 == 5) ? 1 : 0;
#pragma unroll
    for (int u = 0; u < MPW; ++u) {
      if constexpr (KC % 2 == 0) xv[u] = halo[xb[u][t] + off];
      else xv[u] = (k0 + h < KC) ? halo[xb[u][t] + off] : 0.f;
    }
  };
  auto read_w = [&](int k0, float (&wv)[NG][NPW]) {
#pragma unroll
    for (int v = 0; v < NPW; ++v)
#pragma unroll
      for (int g = 0; g < NG; ++g) wv[g][v] = wl[((size_t)g * KCP + k0 + h) * COUT + (wn * NPW + v) * 32 + (lane & 31)];
  };
  // operand ring: step k0's operands are read PD steps ahead
  float xr[PD + 1][MPW], wr[PD + 1][NG][NPW];
#pragma unroll
  for (int d = 0; d < PD; ++d)
    if (2 * d < KCP) {
      read_x(2 * d, xr[d]);
      read_w(2 * d, wr[d]);
    }
#pragma unroll
  for (int k0 = 0; k0 < KCP; k0 += 2) {
    const int cur = (k0 / 2) % (PD + 1), nxt = (k0 / 2 + PD) % (PD + 1);
    if (k0 + 2 * PD < KCP) {
      read_x(k0 + 2 * PD, xr[nxt]);
      read_w(k0 + 2 * PD, wr[nxt]);
    }
    if constexpr (Cfg::PIN) __builtin_amdgcn_sched_barrier(0);   // keep the ring (see DRSA_CONV_PIN_SMALL)
#pragma unroll
    for (int v = 0; v < NPW; ++v)
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int u = 0; u < MPW; ++u) {
          float x = xr[cur][u];
          // NG == 2 is the Gamma forward on a non-negative input (ABI contract): x+ = x, so both
          // sets read the same operand with no per-k-step transform
          if constexpr (EPI < EPI_BWD && NG == 3) {
            x = (g == 0) ? x : (g == 1 ? fmaxf(x, 0.f) : fminf(x, 0.f));
          }
          acc[g][u][v] = mfma32(wr[cur][g][v], x, acc[g][u][v]);
        }
  }
}

// x+ / x- of 8 packed bf16 (sign bit per 16-bit half): Gamma's NG = 3 forward on a signed input
__device__ __forceinline__ uint32_t bf2_neg_mask(uint32_t w) { return ((w >> 15) & 0x00010001u) * 0xffffu; }

// ---- bf16 MFMA over one staged 16-channel chunk: one v_mfma_f32_32x32x16_bf16 per tap and
//      (set, m-tile, n-tile); lane l reads its 8 channels (half l>>5) of pixel l&31 (B) and of
//      output channel l&31 (A) as one ds_read_b128 each, one tap ahead. ----
template <class Cfg>
__device__ __forceinline__ void mfma_chunk_bf(const uint4* hb, const uint4* wb, const int (&pix_off)[Cfg::MPW],
                                              int lane, int wn, f32x16 (&acc)[Cfg::NG_][Cfg::MPW][Cfg::NPW]) {
  constexpr int MPW = Cfg::MPW, NPW = Cfg::NPW, NG = Cfg::NG_, COUT = Cfg::COUT_, HXB = Cfg::HXB;
  const uint4* wlane = wb + (lane >> 5) * COUT + wn * NPW * 32 + (lane & 31);
  uint4 xr[2][MPW], wr[2][NG][NPW];
  auto rd = [&](int t, uint4 (&x)[MPW], uint4 (&w)[NG][NPW]) {
    const int toff = (t / 3) * HXB + t % 3;
#pragma unroll
    for (int u = 0; u < MPW; ++u) x[u] = hb[pix_off[u] + toff];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int v = 0; v < NPW; ++v) w[g][v] = wlane[(g * 9 + t) * 2 * COUT + v * 32];
  };
  rd(0, xr[0], wr[0]);
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int cur = t & 1;
    if (t + 1 < 9) rd(t + 1, xr[cur ^ 1], wr[cur ^ 1]);
#pragma unroll
    for (int v = 0; v < NPW; ++v)
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int u = 0; u < MPW; ++u) {
          uint4 b = xr[cur][u];
          if constexpr (NG == 3) {
            if (g > 0) {
              const uint4 m = make_uint4(bf2_neg_mask(b.x), bf2_neg_mask(b.y), bf2_neg_mask(b.z), bf2_neg_mask(b.w));
              b = (g == 1) ? make_uint4(b.x & ~m.x, b.y & ~m.y, b.z & ~m.z, b.w & ~m.w)
                           : make_uint4(b.x & m.x, b.y & m.y, b.z & m.z, b.w & m.w);
            }
          }
          acc[g][u][v] = mfma32_bf16(__builtin_bit_cast(u16x8, wr[cur][g][v]), __builtin_bit_cast(u16x8, b),
                                     acc[g][u][v]);
        }
  }
}

}  // namespace drsa_conv
