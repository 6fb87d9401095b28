// fp32 staging (ET = 0) of the 3x3 conv kernel (lrp_conv_kernel.h).
#pragma once
#include "common.h"
#include "lrp_conv.h"
#include "lrp_conv_config.h"

namespace drsa_conv {

// ---- staging of one input-channel chunk: registers <- global (load), LDS <- registers
//      (store), split so that the loads of the next chunk can be issued before the MFMA loop
//      of the current one.  NT_ threads take part (tid in [0, NT_)). ----
template <class Cfg, int NT_ = kThreads>
struct Stager {
  static constexpr int CIN = Cfg::CIN_, COUT = Cfg::COUT_, TH = Cfg::TH_, TW = Cfg::TW_, CIC = Cfg::CIC_;
  static constexpr int NG = Cfg::NG_, HY = Cfg::HY, HX = Cfg::HX, RS = Cfg::RS, PLANE = Cfg::PLANE;
  static constexpr int KC = Cfg::KC, KCP = Cfg::KCP;
  static constexpr bool DENSE = Cfg::AMODE_ == A_DENSE;
  // dense halo: interior rows of TW/4 float4 + the two halo columns
  static constexpr int Q4 = TW / 4, DROWS = CIC * HY;
  static constexpr int DI = (DROWS * Q4 + NT_ - 1) / NT_, DH = (DROWS * 2 + NT_ - 1) / NT_;
  // pool-sparse cells: interior rows of TW/8 float4 (4 cells) + the two halo cell columns
  static constexpr int CY = TH / 2 + 2, CX = TW / 2 + 2, Q8 = TW / 8 > 0 ? TW / 8 : 1, SROWS = CIC * CY;
  static constexpr int SI = (SROWS * Q8 + NT_ - 1) / NT_, SH = (SROWS * 2 + NT_ - 1) / NT_;
  // P4: 2 x 4 cells (VGGish's (2,4) pool folded into the staging): interior rows of TW/16 float4
  // (4 cells = 16 pixels each) + the two halo cells, which reach 1 pixel into the halo each
  static constexpr bool P4 = !DENSE && Cfg::PW_ == 4;
  static constexpr int Q16 = TW / 16 > 0 ? TW / 16 : 1;
  static constexpr int SI4 = (SROWS * Q16 + NT_ - 1) / NT_;
  static constexpr int NI = DENSE ? DI : P4 ? SI4 : SI, NH = DENSE ? DH : SH;
  static constexpr int NWV = NG * KCP * (COUT / 4), WIT = (NWV + NT_ - 1) / NT_;
  float4 st_i[NI];
  uint32_t st_ia[DENSE ? 1 : NI];
  float st_h[NH];
  int st_ha[DENSE ? 1 : NH];
  float4 st_w[WIT];

  // Loads are unconditional from a clamped (always valid) address and masked afterwards, so
  // the compiler issues them back to back without exec branches or per-load waits.
  __device__ __forceinline__ void load(const ConvArgs& a, int c0, int tid, int ty0, int tx0, int bq, int bs) {
    const int H = a.H, W = a.W, H2 = H >> 1, W2 = W >> 1;
    // per-sample bases (uniform) + 32-bit per-lane offsets: saddr + voffset loads instead of a
    // 64-bit multiply-add per element (the host keeps one sample's cin x H x W below 2^31)
    const int W4 = W >> 2;
    const float* __restrict__ inb = a.in + (size_t)bq * a.cin * (DENSE ? H * W : H2 * (P4 ? W4 : W2));
    const uint8_t* __restrict__ amb = DENSE ? nullptr : a.in_amax + (size_t)bs * a.cin * H2 * (P4 ? W4 : W2);
    if constexpr (P4) {
      // host contract: W / 4 % 4 == 0, so every 4-cell group is one aligned float4 / uint32
      const int qy0 = (ty0 >> 1) - 1, cx0 = tx0 >> 2;
#pragma unroll
      for (int it = 0; it < SI4; ++it) {
        const int i = tid + it * NT_;
        const int row = i / Q16, q = i % Q16;
        const int ci = row / CY, ry = row % CY;
        const int cy = qy0 + ry, cx = cx0 + 4 * q, c = c0 + ci;
        const bool ok = i < SROWS * Q16 && cy >= 0 && cy < H2 && c < a.cin && cx < W4;
        const int o = ok ? (c * H2 + cy) * W4 + cx : 0;
        const float4 v = *reinterpret_cast<const float4*>(inb + o);
        const uint32_t am = *reinterpret_cast<const uint32_t*>(amb + o);
        st_i[it] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        st_ia[it] = ok ? am : 0xffffffffu;   // 0xff names no pixel of a 2 x 4 window
      }
#pragma unroll
      for (int it = 0; it < SH; ++it) {
        const int i = tid + it * NT_;
        const int row = i >> 1, side = i & 1;
        const int ci = row / CY, ry = row % CY;
        const int cy = qy0 + ry, cx = side ? cx0 + TW / 4 : cx0 - 1, c = c0 + ci;
        const bool ok = i < SROWS * 2 && cy >= 0 && cy < H2 && cx >= 0 && cx < W4 && c < a.cin;
        const int o = ok ? (c * H2 + cy) * W4 + cx : 0;
        const float v = inb[o];
        const int am = (int)amb[o];
        st_h[it] = ok ? v : 0.f;
        st_ha[it] = ok ? am : 0xff;
      }
    } else if constexpr (DENSE) {
      if ((W & 3) == 0) {
#pragma unroll
        for (int it = 0; it < DI; ++it) {
          const int i = tid + it * NT_;
          const int row = i / Q4, q = i % Q4;
          const int ci = row / HY, hy = row % HY;
          const int gy = ty0 - 1 + hy, gx = tx0 + 4 * q, c = c0 + ci;
          const bool ok = i < DROWS * Q4 && gy >= 0 && gy < H && c < a.cin && gx < W;
          const int o = ok ? (c * H + gy) * W + gx : 0;
          const float4 v = *reinterpret_cast<const float4*>(inb + o);
          st_i[it] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      } else {
#pragma unroll
        for (int it = 0; it < DI; ++it) {
          const int i = tid + it * NT_;
          const int row = i / Q4, q = i % Q4;
          const int ci = row / HY, hy = row % HY;
          const int gy = ty0 - 1 + hy, gx = tx0 + 4 * q, c = c0 + ci;
          const bool rok = i < DROWS * Q4 && gy >= 0 && gy < H && c < a.cin;
          float vv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = rok && gx + e < W;
            const int o = ok ? (c * H + gy) * W + gx + e : 0;
            const float v = inb[o];
            vv[e] = ok ? v : 0.f;
          }
          st_i[it] = make_float4(vv[0], vv[1], vv[2], vv[3]);
        }
      }
#pragma unroll
      for (int it = 0; it < DH; ++it) {
        const int i = tid + it * NT_;
        const int row = i >> 1, side = i & 1;
        const int ci = row / HY, hy = row % HY;
        const int gy = ty0 - 1 + hy, gx = side ? tx0 + TW : tx0 - 1, c = c0 + ci;
        const bool ok = i < DROWS * 2 && gy >= 0 && gy < H && gx >= 0 && gx < W && c < a.cin;
        const int o = ok ? (c * H + gy) * W + gx : 0;
        const float v = inb[o];
        st_h[it] = ok ? v : 0.f;
      }
    } else {
      const int qy0 = (ty0 >> 1) - 1, qx0 = (tx0 >> 1) - 1;
      if ((W2 & 3) == 0) {
#pragma unroll
        for (int it = 0; it < SI; ++it) {
          const int i = tid + it * NT_;
          const int row = i / Q8, q = i % Q8;
          const int ci = row / CY, ry = row % CY;
          const int cy = qy0 + ry, cx = qx0 + 1 + 4 * q, c = c0 + ci;
          const bool ok = i < SROWS * Q8 && 4 * q < TW / 2 && cy >= 0 && cy < H2 && c < a.cin && cx < W2;
          const int o = ok ? (c * H2 + cy) * W2 + cx : 0;
          const float4 v = *reinterpret_cast<const float4*>(inb + o);
          const uint32_t am = *reinterpret_cast<const uint32_t*>(amb + o);
          st_i[it] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
          st_ia[it] = ok ? am : 0x04040404u;
        }
      } else {
#pragma unroll
        for (int it = 0; it < SI; ++it) {
          const int i = tid + it * NT_;
          const int row = i / Q8, q = i % Q8;
          const int ci = row / CY, ry = row % CY;
          const int cy = qy0 + ry, cx = qx0 + 1 + 4 * q, c = c0 + ci;
          const bool rok = i < SROWS * Q8 && 4 * q < TW / 2 && cy >= 0 && cy < H2 && c < a.cin;
          float vv[4];
          uint32_t aa = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = rok && cx + e < W2 && 4 * q + e < TW / 2;
            const int o = ok ? (c * H2 + cy) * W2 + cx + e : 0;
            const float v = inb[o];
            const uint32_t am = amb[o];
            vv[e] = ok ? v : 0.f;
            aa |= (ok ? am : 4u) << (8 * e);
          }
          st_i[it] = make_float4(vv[0], vv[1], vv[2], vv[3]);
          st_ia[it] = aa;
        }
      }
#pragma unroll
      for (int it = 0; it < SH; ++it) {
        const int i = tid + it * NT_;
        const int row = i >> 1, side = i & 1;
        const int ci = row / CY, ry = row % CY;
        const int cy = qy0 + ry, cx = side ? qx0 + CX - 1 : qx0, c = c0 + ci;
        const bool ok = i < SROWS * 2 && cy >= 0 && cy < H2 && cx >= 0 && cx < W2 && c < a.cin;
        const int o = ok ? (c * H2 + cy) * W2 + cx : 0;
        const float v = inb[o];
        const int am = (int)amb[o];
        st_h[it] = ok ? v : 0.f;
        st_ha[it] = ok ? am : 4;
      }
    }
    // weights: rows [c0*9, c0*9 + KC) of every set, contiguous (k = ci*9 + tap)
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const int idx = tid + it * NT_;
      const int g = idx / (KCP * (COUT / 4)), rem = idx % (KCP * (COUT / 4));
      const int k = rem / (COUT / 4), c4 = (rem % (COUT / 4)) * 4;
      const bool ok = idx < NWV && k < KC;
      const float4 v = *reinterpret_cast<const float4*>(a.wts + (ok ? ((size_t)g * 9 * CIN + c0 * 9 + k) * COUT + c4 : 0));
      st_w[it] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  // one pool cell -> its 2x2 pixels at halo rows 2ry-1, 2ry and LDS columns 2rx-1+XO, 2rx+XO
  __device__ __forceinline__ static void put_cell(float* halo, int ci, int ry, int rx, float v, int sb) {
    float* d = halo + ci * PLANE + (2 * ry - 1) * RS + 2 * rx - 1 + XO;
    if (ry > 0) *reinterpret_cast<float2*>(d) = make_float2(sb == 0 ? v : 0.f, sb == 1 ? v : 0.f);
    if (ry < CY - 1) *reinterpret_cast<float2*>(d + RS) = make_float2(sb == 2 ? v : 0.f, sb == 3 ? v : 0.f);
  }

  // one 2 x 4 cell -> its 8 pixels: halo rows 2ry-1, 2ry, LDS columns 4rx .. 4rx+3 (halo columns
  // 4rx-3 .. 4rx; rx = 0 and TW/4 + 1 are the halo cells, whose other columns are row padding)
  __device__ __forceinline__ static void put_cell4(float* halo, int ci, int ry, int rx, float v, int sb) {
    float* d = halo + ci * PLANE + (2 * ry - 1) * RS + 4 * rx;
    if (ry > 0)
      *reinterpret_cast<float4*>(d) = make_float4(sb == 0 ? v : 0.f, sb == 1 ? v : 0.f, sb == 2 ? v : 0.f, sb == 3 ? v : 0.f);
    if (ry < CY - 1)
      *reinterpret_cast<float4*>(d + RS) =
          make_float4(sb == 4 ? v : 0.f, sb == 5 ? v : 0.f, sb == 6 ? v : 0.f, sb == 7 ? v : 0.f);
  }

  __device__ __forceinline__ void store(float* halo, float* wl, int tid) const {
    if constexpr (P4) {
      static_assert(XO == 3, "P4 cells land on 16-byte aligned columns 4 rx");
#pragma unroll
      for (int it = 0; it < SI4; ++it) {
        const int i = tid + it * NT_;
        if (i < SROWS * Q16) {
          const int row = i / Q16, q = i % Q16;
          const int ci = row / CY, ry = row % CY;
          const float vv[4] = {st_i[it].x, st_i[it].y, st_i[it].z, st_i[it].w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            put_cell4(halo, ci, ry, 1 + 4 * q + e, vv[e], (int)((st_ia[it] >> (8 * e)) & 0xffu));
        }
      }
#pragma unroll
      for (int it = 0; it < SH; ++it) {
        const int i = tid + it * NT_;
        if (i < SROWS * 2) {
          const int row = i >> 1, side = i & 1;
          put_cell4(halo, row / CY, row % CY, side ? TW / 4 + 1 : 0, st_h[it], st_ha[it]);
        }
      }
    } else if constexpr (DENSE) {
#pragma unroll
      for (int it = 0; it < DI; ++it) {
        const int i = tid + it * NT_;
        if (i < DROWS * Q4) {
          const int row = i / Q4, q = i % Q4;
          const int ci = row / HY, hy = row % HY;
          *reinterpret_cast<float4*>(halo + ci * PLANE + hy * RS + 1 + XO + 4 * q) = st_i[it];
        }
      }
#pragma unroll
      for (int it = 0; it < DH; ++it) {
        const int i = tid + it * NT_;
        if (i < DROWS * 2) {
          const int row = i >> 1, side = i & 1;
          const int ci = row / HY, hy = row % HY;
          halo[ci * PLANE + hy * RS + (side ? HX - 1 : 0) + XO] = st_h[it];
        }
      }
    } else {
#pragma unroll
      for (int it = 0; it < SI; ++it) {
        const int i = tid + it * NT_;
        const int q = i % Q8;
        if (i < SROWS * Q8 && 4 * q < TW / 2) {
          const int row = i / Q8;
          const int ci = row / CY, ry = row % CY;
          const float vv[4] = {st_i[it].x, st_i[it].y, st_i[it].z, st_i[it].w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (4 * q + e < TW / 2) put_cell(halo, ci, ry, 1 + 4 * q + e, vv[e], (int)((st_ia[it] >> (8 * e)) & 0xffu));
        }
      }
#pragma unroll
      for (int it = 0; it < SH; ++it) {
        const int i = tid + it * NT_;
        if (i < SROWS * 2) {
          const int row = i >> 1, side = i & 1;
          put_cell(halo, row / CY, row % CY, side ? CX - 1 : 0, st_h[it], st_ha[it]);
        }
      }
    }
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const int idx = tid + it * NT_;
      if (idx < NWV) *reinterpret_cast<float4*>(wl + (size_t)idx * 4) = st_w[it];
    }
  }
};

}  // namespace drsa_conv
