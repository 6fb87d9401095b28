// The first layer's backward kernels (one input channel), shared by the WSquare / Flat rules
// (first_layer.hip) and the ZBox rule (first_layer_zbox.hip):
//   S_n[y][x] = sum_co sum_{dy,dx} G[co][y+dy][x+dx] * w[n][co][1-dy][1-dx],   n < NCH
//   G dense (16 x 64 output tile, 4 pixels per thread) or pool-sparse (gp, argmax)
// NCH is the number of fma chains every pixel carries over the same staged g: 1 for WSquare / Flat
// (w = w2 [C][9], the chain is the result), 2 for ZBox (w = wpn [2][C][9], W+ then W-).  Chain n of a
// pixel takes w[(n * C + c) * 9 + t] in the order (channel, dy, dx); within a tap the chains are taken
// in the order n = 0 .. NCH-1.  What a rule makes of a pixel's chains is its Epilogue, a small struct:
//   float  px (size_t so, int o, const float  (&s)[NCH])   pixel o of the H x W plane
//   float4 px4(size_t so, int o, const float4 (&s)[NCH])   pixels o .. o+3 (o % 4 == 0)
// so = (bq / clones) * H * W is the plane of the sample that relevance clone bq belongs to.  The
// struct's members travel as kernel arguments of their own (EpArgs) and the kernel puts it together:
// a struct argument is copied at kernel entry, and its pointers then sit in SGPRs across the channel
// loop (4 of them spilled in the scalar-load dense kernel with two chains).
#pragma once
#include "common.h"

namespace {

// the one-chain epilogue: the chain is the result
struct StoreChain {
  __device__ float px(size_t, int, const float (&s)[1]) const { return s[0]; }
  __device__ float4 px4(size_t, int, const float4 (&s)[1]) const { return s[0]; }
};

constexpr int FL_TH = 16, FL_TW = 64;                         // output tile: 16 rows x 16 threads x 4 px
constexpr int FL_CC = 4;                                      // channels staged per group
constexpr int FL_HY = FL_TH + 2, FL_RS = FL_TW + 8;           // LDS row: halo col 3, interior 4..67, halo 68
constexpr int FL_ROWS = FL_CC * FL_HY;                        // staged rows per channel group
constexpr int FL_NV4 = FL_ROWS * (FL_TW / 4);                 // interior float4 per group
constexpr int FL_IV = (FL_NV4 + 255) / 256, FL_IH = (FL_ROWS * 2 + 255) / 256;

// Each thread owns 4 adjacent output pixels of one row.  A channel group's g tile (+1 halo) is
// loaded as coalesced float4 rows (all of a thread's loads issued back to back into registers, the
// next group's while the current one is consumed), then written to LDS; the chains per output pixel
// run in the order (channel, dy, dx), the order of oracle/lrp_exact.c and of the pooled kernel below.
template <int NCH, bool VEC, class Epilogue, class... EpArgs>
__global__ __launch_bounds__(256) void first_layer_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                              float* __restrict__ out, int C, int H, int W, int clones,
                                                              EpArgs... ea) {
  const Epilogue ep{ea...};
  __shared__ __attribute__((aligned(16))) float hal[FL_CC][FL_HY][FL_RS];
  const int tid = threadIdx.x;
  const int tiles_x = (W + FL_TW - 1) / FL_TW;
  const int ty0 = (blockIdx.x / tiles_x) * FL_TH, tx0 = (blockIdx.x % tiles_x) * FL_TW;
  const int bq = blockIdx.y;
  const int ly = tid / 16, lx = (tid % 16) * 4;   // 16 rows x 16 threads, 4 px each
  const size_t plane = (size_t)H * W;
  const int iplane = H * W;   // 32-bit per-lane offsets from the per-sample base (C * H * W < 2^31)
  const float* gb = g + (size_t)bq * C * plane;
  float4 rv[FL_IV];
  float rh[FL_IH];
  // loads from clamped (always valid) addresses, masked afterwards
  auto fetch = [&](int c0) {
#pragma unroll
    for (int it = 0; it < FL_IV; ++it) {
      const int i = tid + it * 256;
      const int row = i / (FL_TW / 4), q = i % (FL_TW / 4);
      const int ci = row / FL_HY, hy = row % FL_HY;
      const int gy = ty0 - 1 + hy, gx = tx0 + 4 * q, c = c0 + ci;
      const bool rok = i < FL_NV4 && c < C && gy >= 0 && gy < H;
      if constexpr (VEC) {
        const bool ok = rok && gx < W;
        const float4 v = *reinterpret_cast<const float4*>(gb + (ok ? c * iplane + gy * W + gx : 0));
        rv[it] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        float e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool ok = rok && gx + k < W;
          const float v = gb[ok ? c * iplane + gy * W + gx + k : 0];
          e[k] = ok ? v : 0.f;
        }
        rv[it] = make_float4(e[0], e[1], e[2], e[3]);
      }
    }
#pragma unroll
    for (int it = 0; it < FL_IH; ++it) {
      const int i = tid + it * 256;
      const int row = i >> 1, side = i & 1;
      const int ci = row / FL_HY, hy = row % FL_HY;
      const int gy = ty0 - 1 + hy, gx = side ? tx0 + FL_TW : tx0 - 1, c = c0 + ci;
      const bool ok = i < FL_ROWS * 2 && c < C && gy >= 0 && gy < H && gx >= 0 && gx < W;
      const float v = gb[ok ? c * iplane + gy * W + gx : 0];
      rh[it] = ok ? v : 0.f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int it = 0; it < FL_IV; ++it) {
      const int i = tid + it * 256;
      if (i < FL_NV4) {
        const int row = i / (FL_TW / 4), q = i % (FL_TW / 4);
        *reinterpret_cast<float4*>(&hal[row / FL_HY][row % FL_HY][4 + 4 * q]) = rv[it];
      }
    }
#pragma unroll
    for (int it = 0; it < FL_IH; ++it) {
      const int i = tid + it * 256;
      if (i < FL_ROWS * 2) {
        const int row = i >> 1, side = i & 1;
        hal[row / FL_HY][row % FL_HY][side ? 4 + FL_TW : 3] = rh[it];
      }
    }
  };
  float acc[4][NCH] = {};   // [pixel][chain]
  fetch(0);
  for (int c0 = 0; c0 < C; c0 += FL_CC) {
    __syncthreads();
    stage();
    __syncthreads();
    if (c0 + FL_CC < C) fetch(c0 + FL_CC);
#pragma unroll 2
    for (int ci = 0; ci < FL_CC; ++ci) {
      // channels past C were staged as zeros: fma(0, w, acc) == acc, so any finite weight will do
      const int c = min(c0 + ci, C - 1);
      float wv[NCH][9];
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int n = 0; n < NCH; ++n) wv[n][t] = w[(n * C + c) * 9 + t];
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const float* r = &hal[ci][ly + 1 + dy][3 + lx];      // pixel tx0 + lx - 1 ..
        const float4 m = *reinterpret_cast<const float4*>(r + 1);
        const float row[6] = {r[0], m.x, m.y, m.z, m.w, r[5]};
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int t = (1 - dy) * 3 + (1 - dx);
#pragma unroll
          for (int n = 0; n < NCH; ++n)
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[p][n] = fmaf(row[p + 1 + dx], wv[n][t], acc[p][n]);
        }
      }
    }
  }
  const int y = ty0 + ly;
  if (y < H) {
    const size_t so = (size_t)(bq / clones) * plane;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int x = tx0 + lx + p;
      if (x < W) {
        const int o = y * W + x;
        out[(size_t)bq * plane + o] = ep.px(so, o, acc[p]);
      }
    }
  }
}

// Pool-sparse variant (the VGG case: conv0 -> ReLU -> MaxPool2d(2)).  A workgroup covers
// 16 x 64 pool cells (32 x 128 output pixels); each thread owns 2 x 2 cells = a 4 x 4 pixel
// block.  Per channel the cells of the tile (+1 halo) are expanded to pixels while staging
// (value at the argmax position, zeros elsewhere) into an image with origin pixel
// (2qy0-2, 2qx0-2) at column FQ_C0; the next channel's cells are prefetched (branch-free, range
// checked by the buffer loads) into registers while the current channel is consumed.  Every
// thread reads its 6 x 6 patch per channel row by row as five pixel pairs (one row of pairs
// live: fewer VGPRs, more waves) and runs packed fmas (v_pk_fma_f32: two output pixels per
// instruction, each pair once into every chain) in the dense chain order (channel, dy, dx) — the
// chain of the dense kernel above and of oracle/lrp_exact.c (the zero terms included:
// fma(0, w, acc) == acc).
// One register set of staged cells, at 8 waves/SIMD with one chain: a second set in flight (106
// VGPRs, 4 waves/SIMD, or spills at 6) keeps no more bytes in flight.
constexpr int FQ_Y = 16, FQ_X = 64;
constexpr int FQ_RY = FQ_Y + 2, FQ_RX = FQ_X + 2;            // cells incl. halo
constexpr int FQ_PY = 2 * FQ_RY, FQ_PX = 2 * FQ_RX + 4;      // pixel image (row pad 4)
constexpr int FQ_KR = (FQ_RY + 3) / 4;                       // row passes of 4 waves
// image column of the halo origin: 3 puts every thread's 6-pixel window (starting at 4tx + 4) on
// a 16-byte boundary, so a row of it is one ds_read_b128 + one ds_read_b64 over consecutive lanes
// (bank-conflict free; the former origin 1 gave 8-byte reads at a 16-byte lane stride)
constexpr int FQ_C0 = 3;
constexpr int FQ_NS = FQ_KR + 1;                             // staged cells per thread

typedef float fq2 __attribute__((ext_vector_type(2)));

// W2C > 0: the pooled width as a compile-time constant (GTZAN: 64), so the per-k row offsets of the
// staging loads are instruction immediates instead of adds.  The one-chain kernel is held to 8
// waves/SIMD; two chains are left to the compiler (waves_per_eu(1) constrains nothing).
template <int NCH, int W2C, class Epilogue, class... EpArgs>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NCH == 1 ? 8 : 1))) void
first_layer_bwd_pooled_kernel(const float* __restrict__ g, const uint8_t* __restrict__ amax,
                              const float* __restrict__ w, float* __restrict__ out, int C, int H, int W, int clones,
                              EpArgs... ea) {
  const Epilogue ep{ea...};
  extern __shared__ __attribute__((aligned(16))) float img[];    // [FQ_PY][FQ_PX]
  const int tid = threadIdx.x, lane = tid & 63, wv4 = tid >> 6;
  const int H2 = H / 2, W2 = W2C > 0 ? W2C : W / 2;
  const int tiles_x = (W2 + FQ_X - 1) / FQ_X;
  const int qy0 = (blockIdx.x / tiles_x) * FQ_Y, qx0 = (blockIdx.x % tiles_x) * FQ_X;
  const int bq = blockIdx.y, bs = bq / clones;
  const int ty = tid / (FQ_X / 2), tx = tid % (FQ_X / 2);      // 8 x 32 threads, 2x2 cells each
  const size_t plane = (size_t)H2 * W2;
  const int iplane = H2 * W2;
  const float* gb = g + (size_t)bq * C * plane;
  const uint8_t* ab = amax + (size_t)bs * C * plane;
  // staging map: interior columns rx = 1 + lane, rows ry = wave + 4k; the two halo columns
  // (rx = 0, 65) of all rows by threads tid < 2 * FQ_RY
  const int hr = tid % (2 * FQ_RY);
  const int hry = hr >> 1, hrx = (hr & 1) ? FQ_RX - 1 : 0;
  const bool hact = tid < 2 * FQ_RY;
  fq2 acc[NCH][4][2];
#pragma unroll
  for (int n = 0; n < NCH; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[n][i][0] = acc[n][i][1] = fq2{0.f, 0.f};
  auto compute = [&](int c) {
    float wv[NCH][9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int n = 0; n < NCH; ++n) wv[n][t] = w[(n * C + c) * 9 + t];
    // patch P[i][j] = pixel (2qy0 + 4ty - 1 + i, 2qx0 + 4tx - 1 + j) = img[4ty + 1 + i][4tx + FQ_C0 + 1 + j];
    // pair q (q = 0..4) = (P[i][q], P[i][q + 1])
    const float* base = img + (4 * ty + 1) * FQ_PX + 4 * tx + FQ_C0 + 1;
    // patch rows streamed: row i feeds output rows py = i - 1 - dy, i.e. each output row takes
    // its taps in dy order (then dx) -- the chain order -- with only one patch row live
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const float* r = base + i * FQ_PX;
      const float4 q4 = *reinterpret_cast<const float4*>(r);
      const fq2 q2 = *reinterpret_cast<const fq2*>(r + 4);
      const fq2 rp[5] = {fq2{q4.x, q4.y}, fq2{q4.y, q4.z}, fq2{q4.z, q4.w}, fq2{q4.w, q2.x}, q2};
#pragma unroll
      for (int py = 0; py < 4; ++py) {
        const int dy = i - py - 1;
        if (dy < -1 || dy > 1) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int t = (1 - dy) * 3 + (1 - dx);
#pragma unroll
          for (int n = 0; n < NCH; ++n) {
            const fq2 ww = fq2{wv[n][t], wv[n][t]};
            acc[n][py][0] = __builtin_elementwise_fma(rp[1 + dx], ww, acc[n][py][0]);
            acc[n][py][1] = __builtin_elementwise_fma(rp[3 + dx], ww, acc[n][py][1]);
          }
        }
      }
    }
  };
  // Cells through buffer loads: a per-channel descriptor (uniform) over the channel's plane, so a
  // cell above / below the image reads 0 (value and argmax byte) by the hardware range check, and
  // a cell left / right of it is pushed out of range by its lane offset; the per-k lane offsets
  // are one base + k rows.  The pixel image keeps its zeros between channels: each staged cell
  // clears the one pixel it set for the previous channel and sets the argmax pixel of this one
  // (LDS writes of a lane land in order), 3 VALU per cell instead of 4 compares + 4 selects.
  const int cxl = qx0 + lane;
  const unsigned OOR = 0x80000000u;   // >= any plane's byte size: the range check returns 0
  const unsigned lane_off = cxl < W2 ? (unsigned)(((qy0 - 1 + wv4) * W2 + cxl) * 4) : OOR;
  const int cxh = qx0 - 1 + hrx;
  const unsigned halo_off =
      (hact && cxh >= 0 && cxh < W2) ? (unsigned)(((qy0 - 1 + hry) * W2 + cxh) * 4) : OOR;
  const unsigned row4 = (unsigned)(4 * 4 * W2);   // 4 cell rows in bytes
  const unsigned pbytes = (unsigned)(iplane * 4);
  float vi[FQ_NS];
  unsigned si[FQ_NS];
  auto fetch = [&](int c) {
    // re-derive the per-k offsets every channel (5 adds) instead of holding 10 of them live
    unsigned lo = lane_off, ho = halo_off;
    asm volatile("" : "+v"(lo), "+v"(ho));
    // row k = 0 may lie above the image (a negative offset, out of range as unsigned); rows k >= 1
    // hang off a base that is never negative, so their offsets add as instruction immediates (the
    // hardware sums voffset + immediate without a 32-bit wrap)
    const unsigned lo1 = lo + row4;
    const unsigned la0 = lo >> 2, la1 = lo1 >> 2;   // the argmax plane's (byte) offsets are the cell indices
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(gb + (size_t)c * plane), 0, (int)pbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(ab + (size_t)c * plane), 0, (int)(pbytes / 4), 0x00020000);
#pragma unroll
    for (int k = 0; k < FQ_KR; ++k) {
      // stays >= 2^31 (2^29 for the argmax plane) when lane_off is OOR
      const unsigned og = k == 0 ? lo : lo1 + (unsigned)(k - 1) * row4;
      const unsigned oa = k == 0 ? la0 : la1 + (unsigned)(k - 1) * (row4 / 4);
      vi[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, og, 0, 0));
      si[k] = __builtin_amdgcn_raw_buffer_load_b8(ra, oa, 0, 0);
    }
    vi[FQ_NS - 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, ho, 0, 0));
    si[FQ_NS - 1] = __builtin_amdgcn_raw_buffer_load_b8(ra, ho >> 2, 0, 0);
  };
  // LDS byte address of each staged cell's top-left pixel and of the pixel set last channel
  typedef __attribute__((address_space(3))) char lds_char;
  typedef __attribute__((address_space(3))) float lds_float;
  lds_char* const imgb = (lds_char*)img;
  int cell0[FQ_NS];
  lds_float* prev[FQ_NS];
#pragma unroll
  for (int k = 0; k < FQ_KR; ++k) cell0[k] = 4 * (2 * (wv4 + 4 * k) * FQ_PX + 2 * (1 + lane) + FQ_C0);
  cell0[FQ_NS - 1] = 4 * (2 * hry * FQ_PX + 2 * hrx + FQ_C0);
#pragma unroll
  for (int k = 0; k < FQ_NS; ++k) prev[k] = (lds_float*)(imgb + cell0[k]);
  auto act = [&](int k) { return k == FQ_NS - 1 ? hact : (wv4 + 4 * k < FQ_RY); };
  for (int i = tid; i < FQ_PY * FQ_PX; i += 256) img[i] = 0.f;
  fetch(0);
  for (int c = 0; c < C; ++c) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FQ_NS; ++k) {
      if (act(k)) {
        // argmax b = 2 row + col -> byte offset 4 col + 4 FQ_PX row = 4 b + (4 FQ_PX - 8) (b & 2)
        const int b = (int)(si[k] & 3u);
        lds_float* const nw = (lds_float*)(imgb + (cell0[k] + 4 * b + (4 * FQ_PX - 8) / 2 * (b & 2)));
        *prev[k] = 0.f;
        *nw = vi[k];
        prev[k] = nw;
      }
    }
    __syncthreads();
    if (c + 1 < C) fetch(c + 1);
    compute(c);
  }
  const int oy = 2 * qy0 + 4 * ty, ox = 2 * qx0 + 4 * tx;
  if (2 * (qx0 + 2 * tx) < W && ox < W) {
    const size_t so = (size_t)bs * H * W;
#pragma unroll
    for (int py = 0; py < 4; ++py) {
      if (oy + py < H) {
        const int o = (oy + py) * W + ox;
        float4 s[NCH];
#pragma unroll
        for (int n = 0; n < NCH; ++n)
          s[n] = make_float4(acc[n][py][0].x, acc[n][py][0].y, acc[n][py][1].x, acc[n][py][1].y);
        *reinterpret_cast<float4*>(out + (size_t)bq * H * W + o) = ep.px4(so, o, s);
      }
    }
  }
}

// The launch both rules share: `name` is the entry point's, for the messages; `ea` are the
// Epilogue's members in their order; the entry point has checked what is only its own.
template <int NCH, class Epilogue, class... EpArgs>
int first_layer_bwd_launch(const char* name, const float* g, const uint8_t* amax, const float* w, float* out, int Bq,
                           int clones, int C, int H, int W, void* stream, EpArgs... ea) {
  DRSA_REQUIRE(Bq > 0 && clones > 0 && Bq % clones == 0, "%s: bad batch", name);
  DRSA_REQUIRE((int64_t)C * H * W < ((int64_t)1 << 31), "%s: one sample's C x H x W must stay below 2^31", name);
  if (amax) {
    DRSA_REQUIRE(H % 2 == 0 && W % 4 == 0, "%s: pooled path needs even H and W %% 4 == 0", name);
    DRSA_REQUIRE(((uintptr_t)out & 15) == 0, "%s: pooled path stores float4: out must be 16-byte aligned", name);
    const int H2 = H / 2, W2 = W / 2;
    const dim3 grid(((H2 + FQ_Y - 1) / FQ_Y) * ((W2 + FQ_X - 1) / FQ_X), Bq);
    constexpr size_t lds = sizeof(float) * FQ_PY * FQ_PX;
    auto kf = W == 128 ? first_layer_bwd_pooled_kernel<NCH, 64, Epilogue, EpArgs...>
                        : first_layer_bwd_pooled_kernel<NCH, 0, Epilogue, EpArgs...>;
    DRSA_SMEM(kf, lds);
    hipLaunchKernelGGL(kf, grid, dim3(256), lds, (hipStream_t)stream, g, amax, w, out, C, H, W, clones, ea...);
  } else {
    const dim3 grid(((H + FL_TH - 1) / FL_TH) * ((W + FL_TW - 1) / FL_TW), Bq);
    // float4 loads of g rows: every row starts a multiple of 4 floats from the base (W % 4 == 0), so
    // the base decides the alignment; any other base takes the scalar loads (same chains, same values)
    auto kf = W % 4 == 0 && ((uintptr_t)g & 15) == 0 ? first_layer_bwd_kernel<NCH, true, Epilogue, EpArgs...>
                                                     : first_layer_bwd_kernel<NCH, false, Epilogue, EpArgs...>;
    hipLaunchKernelGGL(kf, grid, dim3(256), 0, (hipStream_t)stream, g, w, out, C, H, W, clones, ea...);
  }
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

}  // namespace
