// 3x3 'same' convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32) for the LRP engine.
//
// One templated implicit-GEMM kernel serves the whole conv trunk of the VGG-type CNN
// (reference cxai/model/create_model.py:100-137) in both directions:
//
//   forward  (FWD_POOL / FWD_RELU):  z = conv(x; W) + b  ->  y = relu(z)  [-> 2x2 max-pool + argmax]
//            plus, in the same pass over the input tile, the LRP denominator of the layer's rule:
//            Gamma  (zennit 0.5.1):  den = (conv(x+; W+) + b+) + (conv(x-; W-) + b2)
//            (the plan passes b2 = 0: zennit zeroes the x- term's bias)
//            Epsilon:                               den = z
//            WSquare / Flat:                        den = precomputed input-independent map
//            den is stored only where the relevance can arrive: at the pool argmax.
//   backward (BWD): the transposed conv as a 'same' conv with flipped/transposed weights,
//            R_in = x+ (.) J^T_{W+} g  [+ x- (.) J^T_{W-} g]   (Gamma; g_- vanishes because every
//            conv is followed by ReLU), or x (.) J^T_W g (Epsilon) or J^T g (WSquare/Flat/plain),
//            with the pool-backward + ReLU-backward folded into the A-operand prologue (AMODE 1:
//            g lives at pool resolution plus an argmax byte) and the NEXT layer's division folded
//            into the epilogue (POST_DIV: g_next = [x > 0] R / stab(den_next)).
//
// GEMM view: M = output pixels of a TH x TW tile (window-major order so that every 2x2 pool
// window lands in 4 consecutive accumulator registers of one lane), N = output channels
// (32-wide MFMA tiles), K = 9 * Cin in the order k = ci*9 + (ky*3 + kx) (chunks of CIC input
// channels staged in LDS with the halo; weights [k][co] staged next to them).  Every output
// is one k-ordered fp32 fma chain (MFMA f32 semantics), independent of the chunking, which
// is what oracle/lrp_exact.c reproduces bit for bit.
//
// This file: the kernel (prologue, chunk loop, epilogues).  Its parts: lrp_conv_config.h (build
// knobs, tile rule, ConvCfg), lrp_conv_stage.h / lrp_conv_stage_bf.h (fp32 / bf16 staging),
// lrp_conv_mfma.h (the MFMA loops over a staged chunk); lrp_conv_inst.h instantiates it into the
// tables of lrp_conv_table.h.
#pragma once
#include "common.h"
#include "lrp_conv.h"
#include "lrp_conv_config.h"
#include "lrp_conv_mfma.h"
#include "lrp_conv_stage.h"
#include "lrp_conv_stage_bf.h"

#include <type_traits>

namespace drsa_conv {

// diagnostic build only (-DDRSA_CONV_STAMP, scripts/probe_conv_phases.py): phase times of every
// workgroup of the 32 -> 32 pool-sparse backward (GTZAN conv_bwd:features.3) into a buffer of their
// own, set by drsa_amd_debug_conv_stamps; nothing in the kernel reads them
#ifdef DRSA_CONV_STAMP
static __device__ unsigned long long* g_conv_stamps;
#endif

// bias3 of a forward call without bias ([3][COUT], COUT <= 128)
__device__ const float g_zero_bias3[3 * 128] = {};

// PW: pool window width of EPI_FWD_POOL (2 x PW windows; 4 = VGGish's (2,4) pool)
template <int CIN, int COUT, int TH, int TW, int MW, int CIC, int NG, int AMODE, int EPI, int ET = 0, int PW = 2>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(ConvCfg<CIN, COUT, TH, TW, MW, CIC, NG, AMODE, EPI, ET, PW>::WPE))) void conv3x3_kernel(ConvArgs a) {
  using Cfg = ConvCfg<CIN, COUT, TH, TW, MW, CIC, NG, AMODE, EPI, ET, PW>;
  constexpr int HY = Cfg::HY, HX = Cfg::HX, RS = Cfg::RS, PLANE = Cfg::PLANE;
  constexpr int MTH = Cfg::MTH, MTW = Cfg::MTW, MTX = Cfg::MTX;
  constexpr int WM = Cfg::WM, MPW = Cfg::MPW, NPW = Cfg::NPW;
  constexpr int KC = Cfg::KC, KCP = Cfg::KCP;

  extern __shared__ __attribute__((aligned(16))) float smem[];
#ifdef DRSA_CONV_STAMP
  constexpr bool kStamp = EPI == EPI_BWD && CIN == 32 && COUT == 32 && AMODE == A_POOLSPARSE && ET == 0;
  unsigned long long* const stp = kStamp && g_conv_stamps && threadIdx.x == 0
                                      ? g_conv_stamps + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 : nullptr;
#define CONV_STAMP(slot) do { if (stp) stp[(slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define CONV_STAMP(slot) do {} while (0)
#endif
  CONV_STAMP(0);
  float* halo = smem;                          // [CIC][PLANE]   (bf16: [2][HY][HXB] x 16 B)
  float* wl = smem + (Cfg::BF ? Cfg::bf_halo_floats : (size_t)CIC * PLANE);   // [NG][KCP][COUT]

  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int H = a.H, W = a.W;
  const int tiles_x = (W + TW - 1) / TW;
  const int tile_id = blockIdx.x, bq = blockIdx.y;  // bq: batch index (incl. clones)
  const int ty0 = (tile_id / tiles_x) * TH;
  const int tx0 = (tile_id % tiles_x) * TW;
  const int bs = bq / a.clones;               // sample index (shared forward state)
  const int wm = w % WM, wn = w / WM;
  const bool active = w < WM * Cfg::WN;
  const int h = lane >> 5;

  // MFMA orientation: D[channel][pixel] = W^T[channel][k] * X[k][pixel]
  //   A operand (lane l): W[k = k0 + (l>>5)][co = n0 + (l&31)]
  //   B operand (lane l): X[k = k0 + (l>>5)][pixel p = l&31 of the m-tile]
  //   D: lane l holds pixel p = l&31, registers r hold channels n0 + (r&3) + 8(r>>2) + 4(l>>5)
  // pixel p of an m-tile -> pool window win = p>>2, sub = p&3 (window-major order)
  int pix_off[MPW], pix_y[MPW], pix_x[MPW];
#pragma unroll
  for (int u = 0; u < MPW; ++u) {
    const int mt = wm * MPW + u;
    const int p = lane & 31, win = p >> 2, sub = p & 3;
    pix_y[u] = (mt / MTX) * MTH + 2 * (win / MW) + (sub >> 1);
    pix_x[u] = (mt % MTX) * MTW + 2 * (win % MW) + (sub & 1);
    pix_off[u] = Cfg::BF ? (h * HY + pix_y[u]) * Cfg::HXB + pix_x[u] : pix_y[u] * RS + pix_x[u] + XO;
  }

  f32x16 acc[NG][MPW][NPW];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int u = 0; u < MPW; ++u)
#pragma unroll
      for (int v = 0; v < NPW; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[g][u][v][r] = 0.f;

  // ---- epilogue, staged through LDS so global I/O is coalesced float4 rows ----
  // pass (v, kind): every active wave writes its 32-channel slice (n-tile wn*NPW + v) of its
  // m-tiles into T[TCH][TH][TWP] (lane = pixel, register = channel: conflict-free rows),
  // then all threads walk T in row order.
  constexpr int TWP = Cfg::TWP, TCH = Cfg::TCH;
  constexpr int NV4 = TCH * TH * TW / 4;                 // float4 groups per pass
  constexpr int V4T = (NV4 + kThreads - 1) / kThreads;   // per thread
  constexpr int NCELL = TCH * (TH / 2) * (TW / 2);
  constexpr int CT = (NCELL + kThreads - 1) / kThreads;
  float* T = smem;
  constexpr int ES = Cfg::ES;
  static_assert(ES == 1 || ES == 2 || ES == 4, "epilogue split must be 1, 2 or 4");
  // pass `sub` of ES stages the registers whose channel lies in [sub*TCH, (sub+1)*TCH)
  // (channel = (r&3) + 8(r>>2) + 4h: ES = 2 takes r >> 3 == sub, ES = 4 r >> 2 == sub)
  auto stage = [&](int v, auto valfn, int sub = 0) {
    __syncthreads();
    if (active) {
#pragma unroll
      for (int u = 0; u < MPW; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cf = (r & 3) + 8 * (r >> 2) + 4 * h;
          if constexpr (ES == 1) {
            T[((wn * 32 + cf) * TH + pix_y[u]) * TWP + pix_x[u]] = valfn(u, r);
          } else {
            if ((r >> (ES == 2 ? 3 : 2)) == sub) T[((cf - TCH * sub) * TH + pix_y[u]) * TWP + pix_x[u]] = valfn(u, r);
          }
        }
    }
    __syncthreads();
  };
  auto gch = [&](int cl, int v) { return ((cl >> 5) * NPW + v) * 32 + (cl & 31); };   // global channel
  // global channel of staged row cl in pass sub (ES = 2 implies WN = 1)
  auto gchs = [&](int cl, int v, int sub) { return ES == 1 ? gch(cl, v) : v * 32 + sub * TCH + cl; };
  typename std::conditional<Cfg::BF, StagerBF<Cfg>, Stager<Cfg>>::type stg;
  stg.load(a, 0, tid, ty0, tx0, bq, bs);
  CONV_STAMP(11);
  // backward: all chunks but the last here, the last one peeled below (after the epilogue
  // addressing is set up, so that none of it is live across the loop)
  for (int chunk = 0; chunk + (EPI == EPI_BWD ? 1 : 0) < Cfg::NCHUNK; ++chunk) {
    __syncthreads();
    if (chunk == 0) CONV_STAMP(9);
    if constexpr (Cfg::BF) stg.store(halo, wl, tid, ty0, tx0);
    else stg.store(halo, wl, tid);
    if (chunk == 0) CONV_STAMP(10);
    __syncthreads();
    CONV_STAMP(1 + 2 * chunk);
    if (chunk + 1 < Cfg::NCHUNK) stg.load(a, (chunk + 1) * CIC, tid, ty0, tx0, bq, bs);
    if (!active) continue;
    if constexpr (Cfg::BF)
      mfma_chunk_bf<Cfg>(reinterpret_cast<const uint4*>(halo), reinterpret_cast<const uint4*>(wl), pix_off, lane, wn, acc);
    else
      mfma_chunk<Cfg, Cfg::PD>(halo, wl, pix_off, lane, wn, acc);
    CONV_STAMP(2 + 2 * chunk);
  }
  constexpr int Q = TH * TW / 4, CS = kThreads / Q;
  static_assert(kThreads % Q == 0, "float4 groups per tile must divide the block");
  const int cl0 = tid / Q, rem = tid % Q;
  const int py = rem / (TW / 4), px = (rem % (TW / 4)) * 4;
  const bool pix_ok = ty0 + py < H && tx0 + px < W;
  const int HW = H * W;
  const size_t pix = pix_ok ? (size_t)(ty0 + py) * W + tx0 + px : 0;
  const float* xs = a.x ? a.x + (size_t)bs * a.cout * HW + pix : nullptr;
  // den_shared: the next layer's denominator is an input-independent map [cout][H][W] (WSquare /
  // Flat without a pool between): every sample reads the same plane (L2-resident), nothing per sample
  const float* ds = a.den ? a.den + (a.den_shared ? (size_t)0 : (size_t)bs * a.cout * HW) + pix : nullptr;
  float* oqp = a.out + (size_t)bq * a.cout * HW + pix;
  // x and den come from clamped, always valid addresses (den falls back to x or out when the
  // mode does not use it) and are ALL issued before any arithmetic; the rule / post modes are
  // uniform selects, not branches (a branch around the division would put each den load in
  // its own basic block, one full memory round trip after another)
  const bool need_x = a.xmode != XM_NONE || a.post != POST_NONE;
  const bool mul_x = a.xmode != XM_NONE, split_x = a.xmode == XM_SPLIT;
  // POST_DIV_RING: float4 groups off the image's border ring read the map's per-channel value
  // (den_const4, one 16-byte line per channel: an L1 broadcast) instead of the per-sample copy,
  // which the forward writes on the ring only; the pointer is a per-lane select, no branch
  const bool ring = a.post == POST_DIV_RING && a.den_const4;
  const bool post_div = a.post == POST_DIV || ring, post_any = a.post != POST_NONE;
  const float* xsrc = xs ? xs : oqp;
  const float* dsrc = (ds && post_div && !ring) ? ds : xsrc;
  const float eps = a.eps;
  const bool on_ring = !pix_ok || ty0 + py == 0 || ty0 + py == H - 1 || tx0 + px == 0 || tx0 + px + 4 >= W;
  const bool use_c4 = ring && !on_ring;
  // the compact ring of plane (sample, channel): [row 0 | row H-1 | rows 1..H-2 x (4 + 4 columns)]
  const int ring_n = 2 * W + 8 * (H - 2);
  const int Y = ty0 + py, X = tx0 + px;
  const int ring_i = !pix_ok ? 0 : Y == 0 ? X : Y == H - 1 ? W + X : 2 * W + (Y - 1) * 8 + (X == 0 ? 0 : 4);
  const float* rsrc = ring ? a.den + (size_t)bs * a.cout * ring_n + ring_i : dsrc;
  const size_t dstride = ring ? (size_t)ring_n : (size_t)HW;
  // x loads and R stores as a uniform per-sample base + a 32-bit per-lane offset (saddr + voffset
  // addressing; the host keeps one sample's cout x H x W below 2^31)
  const unsigned upix = (unsigned)pix;
  float* const obase = a.out + (size_t)bq * a.cout * HW;
  const float* const xbase = a.x ? a.x + (size_t)bs * a.cout * HW : obase;
  // epilogue x/den loads of (n-tile v, pass sub); (0, 0) is issued before the last chunk's MFMAs
  auto epi_loads = [&](int v, int sub, float4 (&xk)[V4T], float4 (&dk)[V4T], bool lx = true, bool ld = true,
                       int i0 = 0, int i1 = -1) {
    if (i1 < 0) i1 = V4T;
#pragma unroll
    for (int it = i0; it < i1; ++it) {
      const int cl = cl0 + it * CS;
      const int co = gchs(cl, v, sub);
      const bool ok = cl < TCH && co < a.cout;
      const int coc = ok ? co : 0;
      if (lx) xk[it] = *reinterpret_cast<const float4*>(xbase + (upix + (unsigned)coc * (unsigned)HW));
      if (ld) dk[it] = *reinterpret_cast<const float4*>(use_c4 ? a.den_const4 + (size_t)coc * 4 : rsrc + coc * dstride);
    }
  };
  // x groups prefetched before the last chunk's MFMAs (all of them spill a few registers)
  constexpr int kPreN = DRSA_CONV_PRE_N < V4T ? DRSA_CONV_PRE_N : V4T;
  float4 pre_x[V4T], pre_d[V4T];
  if constexpr (EPI == EPI_BWD) {
    // last chunk, peeled: the staging registers are free, so the epilogue's first x loads go
    // out here and their latency hides under the MFMAs (den too would spill: measured slower)
    __syncthreads();
    if constexpr (Cfg::BF) stg.store(halo, wl, tid, ty0, tx0);
    else stg.store(halo, wl, tid);
    __syncthreads();
    CONV_STAMP(2 * Cfg::NCHUNK - 1);
    epi_loads(0, 0, pre_x, pre_d, true, DRSA_CONV_PRE_D, 0, kPreN);

    if (active) {
      if constexpr (Cfg::BF)
        mfma_chunk_bf<Cfg>(reinterpret_cast<const uint4*>(halo), reinterpret_cast<const uint4*>(wl), pix_off, lane, wn,
                           acc);
      else
        mfma_chunk<Cfg, Cfg::PD>(halo, wl, pix_off, lane, wn, acc);
    }
    CONV_STAMP(2 * Cfg::NCHUNK);
  }

  // the pool cells of the staged tile T (2 x PWc windows), one per thread and iteration `it`
  // (it < CT; CT is sized for 2x2 cells, the most)
  auto pool_cells = [&](auto pwc, auto&& fn) {
    constexpr int PWc = decltype(pwc)::value;
    constexpr int CW = TW / PWc, NC = TCH * (TH / 2) * CW;
    const int H2 = H >> 1, W2 = W / PWc;
#pragma unroll
    for (int it = 0; it < CT; ++it) {
      const int i = tid + it * kThreads;
      if (i < NC) {
        const int cl = i / ((TH / 2) * CW), rem = i % ((TH / 2) * CW);
        const int cy = rem / CW, cx = rem % CW;
        fn(it, cl, cy, cx, (ty0 >> 1) + cy, tx0 / PWc + cx, H2, W2);
      }
    }
  };
#pragma unroll
  for (int v = 0; v < NPW; ++v) {
    if constexpr (EPI == EPI_FWD_POOL || EPI == EPI_FWD_RELU) {
      // the lane's 16 channels' biases, loaded unconditionally (bias3 is [3][COUT]; a missing bias
      // reads a zero table) and all issued before any use: a branch around each load had put
      // every one of them in its own basic block behind its own wait
      const float* bb = a.bias ? a.bias : g_zero_bias3;
      float b0[16], b1[16], b2[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = gch(wn * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, v);
        const bool cok = co < a.cout;
        const float x0 = bb[co], x1 = bb[COUT + co], x2 = bb[2 * COUT + co];
        b0[r] = cok ? x0 : 0.f;
        b1[r] = cok ? x1 : 0.f;
        b2[r] = cok ? x2 : 0.f;
      }
      // pass 0: y = relu(z)
      stage(v, [&](int u, int r) {
        const float z = acc[0][u][v][r] + b0[r];
        float y = z > 0.f ? z : 0.f;
        if (z != z) y = z;   // relu(NaN) = NaN (torch semantics)
        return y;
      });
      int am_keep[CT];
      if constexpr (EPI == EPI_FWD_POOL) {
        // 2 x PWc pool windows (PWc = PW: 2, or 4 for VGGish's (2,4) pool): first maximum
        // in row-major window order, NaN wins (torch max_pool2d); argmax byte = row * PWc + col
        auto pass0 = [&](auto pwc) {
          constexpr int PWc = decltype(pwc)::value;
          pool_cells(pwc, [&](int it, int cl, int cy, int cx, int qy, int qx, int H2, int W2) {
            const int co = gch(cl, v);
            const float* t = T + (cl * TH + 2 * cy) * TWP + PWc * cx;
            int am = 0;
            float m = t[0];
#pragma unroll
            for (int s4 = 1; s4 < 2 * PWc; ++s4) {
              const float yv = t[(s4 / PWc) * TWP + s4 % PWc];
              if (yv > m || (yv != yv && m == m)) { m = yv; am = s4; }
            }
            am_keep[it] = am;
            if (co < a.cout && qy < H2 && qx < W2) {
              const size_t o = (size_t)bq * a.cout * H2 * W2 + (unsigned)((co * H2 + qy) * W2 + qx);
              a.out[o] = m;
              a.out_amax[o] = (uint8_t)am;
            }
          });
        };
        if constexpr (PW == 4) {
#pragma unroll
          for (int it = 0; it < CT; ++it) am_keep[it] = 0;
          pass0(std::integral_constant<int, 4>{});
        } else {
          // 2x2 (the GTZAN trunk): the original straight-line form (the generic lambda form costs
          // the fp32 forward kernels ~2-10 %: one more spilled register)
          const int H2 = H >> 1, W2 = W >> 1;
#pragma unroll
          for (int it = 0; it < CT; ++it) {
            const int i = tid + it * kThreads;
            am_keep[it] = 0;
            if (i < NCELL) {
              const int cl = i / ((TH / 2) * (TW / 2)), rem = i % ((TH / 2) * (TW / 2));
              const int cy = rem / (TW / 2), cx = rem % (TW / 2);
              const int co = gch(cl, v);
              const int qy = (ty0 >> 1) + cy, qx = (tx0 >> 1) + cx;
              const float* t = T + (cl * TH + 2 * cy) * TWP + 2 * cx;
              const float yy[4] = {t[0], t[1], t[TWP], t[TWP + 1]};
              int am = 0;
              float m = yy[0];
#pragma unroll
              for (int s4 = 1; s4 < 4; ++s4)
                if (yy[s4] > m || (yy[s4] != yy[s4] && m == m)) { m = yy[s4]; am = s4; }
              am_keep[it] = am;
              if (co < a.cout && qy < H2 && qx < W2) {
                const size_t o = (size_t)bq * a.cout * H2 * W2 + (unsigned)((co * H2 + qy) * W2 + qx);
                a.out[o] = m;
                a.out_amax[o] = (uint8_t)am;
              }
            }
          }
        }
      } else {
#pragma unroll
        for (int it = 0; it < V4T; ++it) {
          const int i = tid + it * kThreads;
          if (i < NV4) {
            const int cl = i / (TH * TW / 4), rem = i % (TH * TW / 4);
            const int py = rem / (TW / 4), px = (rem % (TW / 4)) * 4;
            const int co = gch(cl, v);
            if (co < a.cout && ty0 + py < H && tx0 + px < W) {
              const float4 val = *reinterpret_cast<const float4*>(T + (cl * TH + py) * TWP + px);
              *reinterpret_cast<float4*>(a.out + (size_t)bq * a.cout * H * W + (unsigned)((co * H + ty0 + py) * W + tx0 + px)) = val;
            }
          }
        }
      }
      if (a.out_den && a.den_map) {
        // WSquare / Flat: input-independent map, read directly (coalesced) where it is stored
        if constexpr (EPI == EPI_FWD_POOL) {
          auto gather_map = [&](auto pwc) {
            constexpr int PWc = decltype(pwc)::value;
            pool_cells(pwc, [&](int it, int cl, int, int, int qy, int qx, int H2, int W2) {
              const int co = gch(cl, v);
              const int am = am_keep[it];
              if (co < a.cout && qy < H2 && qx < W2)
                a.out_den[(size_t)bq * a.cout * H2 * W2 + (unsigned)((co * H2 + qy) * W2 + qx)] =
                    a.den_map[(unsigned)((co * H + 2 * qy + am / PWc) * W + PWc * qx + am % PWc)];
            });
          };
          if constexpr (PW == 4) {
            gather_map(std::integral_constant<int, 4>{});
          } else {
            const int H2 = H >> 1, W2 = W >> 1;
#pragma unroll
            for (int it = 0; it < CT; ++it) {
              const int i = tid + it * kThreads;
              if (i < NCELL) {
                const int cl = i / ((TH / 2) * (TW / 2)), rem = i % ((TH / 2) * (TW / 2));
                const int cy = rem / (TW / 2), cx = rem % (TW / 2);
                const int co = gch(cl, v);
                const int qy = (ty0 >> 1) + cy, qx = (tx0 >> 1) + cx;
                const int am = am_keep[it];
                if (co < a.cout && qy < H2 && qx < W2)
                  a.out_den[(size_t)bq * a.cout * H2 * W2 + (unsigned)((co * H2 + qy) * W2 + qx)] =
                      a.den_map[(unsigned)((co * H + 2 * qy + (am >> 1)) * W + 2 * qx + (am & 1))];
              }
            }
          }
        } else {
#pragma unroll
          for (int it = 0; it < V4T; ++it) {
            const int i = tid + it * kThreads;
            if (i < NV4) {
              const int cl = i / (TH * TW / 4), rem = i % (TH * TW / 4);
              const int py = rem / (TW / 4), px = (rem % (TW / 4)) * 4;
              const int co = gch(cl, v);
              if (co < a.cout && ty0 + py < H && tx0 + px < W)
                *reinterpret_cast<float4*>(a.out_den + (size_t)bq * a.cout * H * W + (unsigned)((co * H + ty0 + py) * W + tx0 + px)) =
                    *reinterpret_cast<const float4*>(a.den_map + (unsigned)((co * H + ty0 + py) * W + tx0 + px));
            }
          }
        }
      } else if (a.out_den) {
        // pass 1: the rule's denominator
        stage(v, [&](int u, int r) {
          if constexpr (NG >= 2) {
            const float z0 = acc[1][u][v][r] + b1[r];
            float z1 = b2[r];
            if constexpr (NG == 3) z1 = acc[2][u][v][r] + b2[r];
            return z0 + z1;
          }
          // Epsilon: den = conv(x; W) + b_den (b_den = b, or 0 under zero_params=['bias'])
          return acc[0][u][v][r] + b1[r];
        });
        if constexpr (EPI == EPI_FWD_POOL) {
          auto gather_den = [&](auto pwc) {
            constexpr int PWc = decltype(pwc)::value;
            pool_cells(pwc, [&](int it, int cl, int cy, int cx, int qy, int qx, int H2, int W2) {
              const int co = gch(cl, v);
              const int am = am_keep[it];
              if (co < a.cout && qy < H2 && qx < W2)
                a.out_den[(size_t)bq * a.cout * H2 * W2 + (unsigned)((co * H2 + qy) * W2 + qx)] =
                    T[(cl * TH + 2 * cy + am / PWc) * TWP + PWc * cx + am % PWc];
            });
          };
          if constexpr (PW == 4) {
            gather_den(std::integral_constant<int, 4>{});
          } else {
            const int H2 = H >> 1, W2 = W >> 1;
#pragma unroll
            for (int it = 0; it < CT; ++it) {
              const int i = tid + it * kThreads;
              if (i < NCELL) {
                const int cl = i / ((TH / 2) * (TW / 2)), rem = i % ((TH / 2) * (TW / 2));
                const int cy = rem / (TW / 2), cx = rem % (TW / 2);
                const int co = gch(cl, v);
                const int qy = (ty0 >> 1) + cy, qx = (tx0 >> 1) + cx;
                const int am = am_keep[it];
                if (co < a.cout && qy < H2 && qx < W2)
                  a.out_den[(size_t)bq * a.cout * H2 * W2 + (unsigned)((co * H2 + qy) * W2 + qx)] =
                      T[(cl * TH + 2 * cy + (am >> 1)) * TWP + 2 * cx + (am & 1)];
              }
            }
          }
        } else {
#pragma unroll
          for (int it = 0; it < V4T; ++it) {
            const int i = tid + it * kThreads;
            if (i < NV4) {
              const int cl = i / (TH * TW / 4), rem = i % (TH * TW / 4);
              const int py = rem / (TW / 4), px = (rem % (TW / 4)) * 4;
              const int co = gch(cl, v);
              if (co < a.cout && ty0 + py < H && tx0 + px < W) {
                const float4 val = *reinterpret_cast<const float4*>(T + (cl * TH + py) * TWP + px);
                *reinterpret_cast<float4*>(a.out_den + (size_t)bq * a.cout * H * W + (unsigned)((co * H + ty0 + py) * W + tx0 + px)) = val;
              }
            }
          }
        }
      }
    } else {   // EPI_BWD: R = xmode(acc, x) -> post -> out
      // float4 group i = tid + it * 256: the pixel (py, px) is fixed per thread and the staged
      // row advances by CS = 256 / Q per iteration, so every address is a per-thread base plus
      // a channel offset.  Loads come from clamped (always valid) addresses and the arithmetic
      // runs unconditionally (no exec branches that would serialise the load latency); only the
      // store is masked.  x is loaded once for the rule and the division.
#pragma unroll
     for (int sub = 0; sub < ES; ++sub) {
      float4 Rk[V4T], xk[V4T], dk[V4T];
      if (v == 0 && sub == 0) {
#pragma unroll
        for (int it = 0; it < kPreN; ++it) xk[it] = pre_x[it];
        epi_loads(v, sub, xk, dk, true, false, kPreN, V4T);
        if (DRSA_CONV_PRE_D) {
#pragma unroll
          for (int it = 0; it < V4T; ++it) dk[it] = pre_d[it];
        } else {
          epi_loads(v, sub, xk, dk, false, true);
        }
      } else {
        epi_loads(v, sub, xk, dk);
      }
      stage(v, [&](int u, int r) { return acc[0][u][v][r]; }, sub);
      // the common mode (Epsilon-type rule: R = x * J^T g, then the next layer's division)
      // specialised: the loads above are already in flight, this branch is uniform
      if (NG == 1 && a.xmode == XM_MUL && post_div) {
#pragma unroll
        for (int it = 0; it < V4T; ++it) {
          const int cl = cl0 + it * CS;
          const int co = gchs(cl, v, sub);
          const bool ok = cl < TCH && co < a.cout;
          const int clc = ok ? cl : 0, coc = ok ? co : 0;
          const float4 t = *reinterpret_cast<const float4*>(T + (clc * TH + py) * TWP + px);
          const float4 x = xk[it], d = dk[it];
          auto f = [&](float tt, float xx, float dd) {
            const float q = div_nb(xx * tt, stab(dd, eps));
            return (xx > 0.f) ? q : 0.f;
          };
          const float4 R = make_float4(f(t.x, x.x, d.x), f(t.y, x.y, d.y), f(t.z, x.z, d.z), f(t.w, x.w, d.w));
          if (ok && pix_ok) *reinterpret_cast<float4*>(obase + (upix + (unsigned)coc * (unsigned)HW)) = R;
        }
        continue;
      }
#pragma unroll
      for (int it = 0; it < V4T; ++it) {
        const int cl = cl0 + it * CS;
        const int co = gchs(cl, v, sub);
        const int clc = (cl < TCH && co < a.cout) ? cl : 0;
        const float4 t = *reinterpret_cast<const float4*>(T + (clc * TH + py) * TWP + px);
        if (!need_x) xk[it] = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 x = xk[it];
        // XM_NONE: 1 * t = t;  XM_MUL: x * t;  XM_SPLIT: max(x, 0) * t
        auto xm = [&](float xx) { const float m = split_x ? fmaxf(xx, 0.f) : xx; return mul_x ? m : 1.f; };
        Rk[it] = make_float4(xm(x.x) * t.x, xm(x.y) * t.y, xm(x.z) * t.z, xm(x.w) * t.w);
      }
      if constexpr (NG >= 2) {
        if (split_x) {
          stage(v, [&](int u, int r) { return acc[1][u][v][r]; }, sub);
#pragma unroll
          for (int it = 0; it < V4T; ++it) {
            const int cl = cl0 + it * CS;
            const int co = gchs(cl, v, sub);
            const int clc = (cl < TCH && co < a.cout) ? cl : 0;
            const float4 t = *reinterpret_cast<const float4*>(T + (clc * TH + py) * TWP + px);
            const float4 x = xk[it];
            Rk[it].x += fminf(x.x, 0.f) * t.x;
            Rk[it].y += fminf(x.y, 0.f) * t.y;
            Rk[it].z += fminf(x.z, 0.f) * t.z;
            Rk[it].w += fminf(x.w, 0.f) * t.w;
          }
        }
      }
#pragma unroll
      for (int it = 0; it < V4T; ++it) {
        const int cl = cl0 + it * CS;
        const int co = gchs(cl, v, sub);
        const bool ok = cl < TCH && co < a.cout;
        const int coc = ok ? co : 0;
        float4 R = Rk[it];
        // POST_DIV: x > 0 ? R / stab(den) : 0;  POST_MASK: x > 0 ? R : 0 (quotients evaluated for
        // every lane and mode, then selected)
        const float4 x = xk[it], d = dk[it];
        auto post = [&](float rr, float xx, float dd) {
          const float q = div_nb(rr, stab(dd, eps));
          const float y = post_div ? q : rr;
          return (post_any && !(xx > 0.f)) ? 0.f : y;
        };
        R = make_float4(post(R.x, x.x, d.x), post(R.y, x.y, d.y), post(R.z, x.z, d.z), post(R.w, x.w, d.w));
        if (ok && pix_ok) *reinterpret_cast<float4*>(obase + (upix + (unsigned)coc * (unsigned)HW)) = R;
      }
     }
    }
  }
#ifdef DRSA_CONV_STAMP
  if (stp) {
    stp[13] = __builtin_amdgcn_s_memtime();
    stp[14] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11));    // HW_ID
    stp[15] = (unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11));   // XCC_ID
  }
#endif
#undef CONV_STAMP
}

}  // namespace drsa_conv
