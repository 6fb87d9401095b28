// bf16 staging (ET = 1) of the 3x3 conv kernel (lrp_conv_kernel.h).
#pragma once
#include "common.h"
#include "lrp_conv.h"
#include "lrp_conv_config.h"

namespace drsa_conv {

// ---- bf16 staging (ET = 1) of one 16-channel chunk.  Item (half, hy, hx) = the 8 channels
//      c0 + 8 half .. +7 of halo pixel (hy, hx): 8 coalesced fp32 loads (consecutive lanes on
//      consecutive pixels), rounded and packed at store time into one 16-byte LDS slot.  Weights
//      come pre-laid-out and pre-rounded ([NG][CIN/16][9][2][COUT][8] bf16): a straight copy. ----
template <class Cfg, int NT_ = kThreads>
struct StagerBF {
  static constexpr int CIN = Cfg::CIN_, COUT = Cfg::COUT_, NG = Cfg::NG_, HY = Cfg::HY, HX = Cfg::HX;
  static constexpr int HXB = Cfg::HXB, NCH = CIN / 16;
  static constexpr int NITEM = 2 * HY * HX, IT = (NITEM + NT_ - 1) / NT_;
  static constexpr int NWQ = NG * 18 * COUT, WIT = (NWQ + NT_ - 1) / NT_;
  // (2,4) pool-sparse staging: one item per (channel half, halo row, pool cell): the cell's 8
  // channel values and argmax bytes are loaded once and expanded to its 4 pixels at store time
  // (the generic per-pixel item would load each cell 4 times)
  static constexpr bool P4 = Cfg::AMODE_ == A_POOLSPARSE && Cfg::PW_ == 4;
  static constexpr int NCR = Cfg::TW_ / 4 + 2;                 // cells per halo row (2 partial)
  static constexpr int NITEM4 = 2 * HY * NCR, IT4 = (NITEM4 + NT_ - 1) / NT_;
  static constexpr int ITX = P4 ? IT4 : IT;
  float st_f[ITX][8];
  uint32_t st_a[P4 ? IT4 : 1][2];
  uint4 st_w[WIT];

  __device__ __forceinline__ void load(const ConvArgs& a, int c0, int tid, int ty0, int tx0, int bq, int bs) {
    const int H = a.H, W = a.W;
    const unsigned HW = (unsigned)(H * W);
    // per-sample bases (uniform) + 32-bit per-lane offsets (saddr + voffset loads)
    const int H2s = H >> 1, W2s = W / (P4 ? 4 : Cfg::PW_);
    const float* __restrict__ inb =
        a.in + (size_t)bq * a.cin * (Cfg::AMODE_ == A_POOLSPARSE || P4 ? (size_t)H2s * W2s : (size_t)HW);
    const uint8_t* __restrict__ amb = (Cfg::AMODE_ == A_POOLSPARSE || P4) ? a.in_amax + (size_t)bs * a.cin * H2s * W2s
                                                                          : nullptr;
    if constexpr (P4) {
      const int H2 = H >> 1, W2 = W >> 2;
      const unsigned HW2 = (unsigned)(H2 * W2);
#pragma unroll
      for (int it = 0; it < IT4; ++it) {
        const int i = tid + it * NT_;
        const int cs = i % NCR, r = i / NCR, hy = r % HY, half = r / HY;
        const int gy = ty0 - 1 + hy, cx = (tx0 >> 2) - 1 + cs, cb = c0 + 8 * half;
        const bool ok = i < NITEM4 && gy >= 0 && gy < H && cx >= 0 && cx < W2;
        const unsigned cell = ok ? (unsigned)((gy >> 1) * W2 + cx) : 0u;
        const unsigned base = ok ? (unsigned)cb * HW2 + cell : 0u;
        uint32_t ab[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool okc = ok && cb + j < a.cin;
          const float v = inb[okc ? base + j * HW2 : 0u];
          const uint32_t am = amb[okc ? base + j * HW2 : 0u];
          st_f[it][j] = okc ? v : 0.f;
          ab[j >> 2] |= (okc ? am : 0xffu) << (8 * (j & 3));   // 0xff matches no pixel
        }
        st_a[it][0] = ab[0];
        st_a[it][1] = ab[1];
      }
    } else if constexpr (Cfg::AMODE_ == A_POOLSPARSE) {
      // backward input at 2 x PW pool resolution + argmax byte (the pool backward; PW = 4: the
      // VGGish (2,4) pool, create_model.py:61): halo pixel (gy, gx) holds g[cell] where the cell's
      // argmax (row-major window position) is this pixel, else 0
      constexpr int PWB = Cfg::PW_;
      const int H2 = H >> 1, W2 = W / PWB;
      const unsigned HW2 = (unsigned)(H2 * W2);
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int i = tid + it * NT_;
        const int hx = i % HX, r = i / HX, hy = r % HY, half = r / HY;
        const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx, cb = c0 + 8 * half;
        const bool ok = i < NITEM && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const unsigned cell = ok ? (unsigned)((gy >> 1) * W2 + (gx / PWB)) : 0u;
        const unsigned base = ok ? (unsigned)cb * HW2 + cell : 0u;
        const uint32_t sub = (uint32_t)((gy & 1) * PWB + (gx % PWB));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool okc = ok && cb + j < a.cin;
          const float v = inb[okc ? base + j * HW2 : 0u];
          const uint32_t am = amb[okc ? base + j * HW2 : 0u];
          st_f[it][j] = (okc && am == sub) ? v : 0.f;
        }
      }
    } else {
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int i = tid + it * NT_;
        const int hx = i % HX, r = i / HX, hy = r % HY, half = r / HY;
        const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx, cb = c0 + 8 * half;
        const bool ok = i < NITEM && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const unsigned base = ok ? (unsigned)cb * HW + (unsigned)(gy * W + gx) : 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool okc = ok && cb + j < a.cin;
          const float v = inb[okc ? base + j * HW : 0u];
          st_f[it][j] = okc ? v : 0.f;
        }
      }
    }
    const uint4* wq = reinterpret_cast<const uint4*>(a.wts);
    const int chunk = c0 / 16;
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const int idx = tid + it * NT_;
      const bool ok = idx < NWQ;
      const int g = idx / (18 * COUT), rem = idx % (18 * COUT);
      st_w[it] = wq[ok ? ((size_t)g * NCH + chunk) * 18 * COUT + rem : 0];
    }
  }

  __device__ __forceinline__ void store(float* halo, float* wl, int tid, int ty0 = 0, int tx0 = 0) const {
    uint4* hb = reinterpret_cast<uint4*>(halo);
    if constexpr (P4) {
#pragma unroll
      for (int it = 0; it < IT4; ++it) {
        const int i = tid + it * NT_;
        if (i < NITEM4) {
          const int cs = i % NCR, r = i / NCR, hy = r % HY;
          const uint32_t rowsub = (uint32_t)(((ty0 - 1 + hy) & 1) * 4);
          // cell cs covers halo columns 4 cs - 3 .. 4 cs (halo column hx = pixel tx0 - 1 + hx)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int hx = 4 * cs - 3 + e;
            if (hx >= 0 && hx < HX) {
              float v8[8];
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const uint32_t am = (st_a[it][j >> 2] >> (8 * (j & 3))) & 0xffu;
                v8[j] = am == rowsub + (uint32_t)e ? st_f[it][j] : 0.f;
              }
              uint4 q;
              q.x = pack_bf16x2(v8[0], v8[1]);
              q.y = pack_bf16x2(v8[2], v8[3]);
              q.z = pack_bf16x2(v8[4], v8[5]);
              q.w = pack_bf16x2(v8[6], v8[7]);
              hb[r * HXB + hx] = q;
            }
          }
        }
      }
    } else {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = tid + it * NT_;
      if (i < NITEM) {
        const int hx = i % HX, r = i / HX;
        uint4 q;
        q.x = pack_bf16x2(st_f[it][0], st_f[it][1]);
        q.y = pack_bf16x2(st_f[it][2], st_f[it][3]);
        q.z = pack_bf16x2(st_f[it][4], st_f[it][5]);
        q.w = pack_bf16x2(st_f[it][6], st_f[it][7]);
        hb[r * HXB + hx] = q;   // r = half * HY + hy
      }
    }
    }
    uint4* wb = reinterpret_cast<uint4*>(wl);
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const int idx = tid + it * NT_;
      if (idx < NWQ) wb[idx] = st_w[it];
    }
  }
};

}  // namespace drsa_conv
