// LRP first layer under the ZBox rule (zennit 0.5.1 ZBox), one input channel, for an
// input that lives in a box low <= x <= high:
//   * the rule's two input-independent maps  zl = conv(low; W+) + b+,  zh = conv(high; W-) + b-
//   * the per-sample denominator copy        den = (a - zl[at]) - zh[at]
//   * backward  R[y][x] = (x - low) S+ + (x - high) S-,  S+- = sum_co sum_{dy,dx} G[co][y+dy][x+dx] W+-[co][1-dy][1-dx]
//               G dense (16 x 64 output tile, 4 pixels per thread) or pool-sparse (gp, argmax)
// Every tap of W is in exactly one of W+ = max(W, 0), W- = min(W, 0), so the two chains are zennit's
// three-term reducer x J^T_W g - l J^T_{W+} g - h J^T_{W-} g with the terms grouped by weight sign; the
// factors x - low >= 0 >= x - high do not cancel.  The kernels have the shape of first_layer.hip's:
// the staging is the same, every pixel carries two accumulator chains instead of one.
#include "common.h"

namespace {

constexpr int ZL_TH = 16, ZL_TW = 64;                         // output tile: 16 rows x 16 threads x 4 px
constexpr int ZL_CC = 4;                                      // channels staged per group
constexpr int ZL_HY = ZL_TH + 2, ZL_RS = ZL_TW + 8;           // LDS row: halo col 3, interior 4..67, halo 68
constexpr int ZL_ROWS = ZL_CC * ZL_HY;                        // staged rows per channel group
constexpr int ZL_NV4 = ZL_ROWS * (ZL_TW / 4);                 // interior float4 per group
constexpr int ZL_IV = (ZL_NV4 + 255) / 256, ZL_IH = (ZL_ROWS * 2 + 255) / 256;

// out = (x - l) sp + (x - h) sn: four roundings and a fifth for the sum, none contracted
__device__ __forceinline__ float zbox_out(float x, float l, float h, float sp, float sn) {
  return __fadd_rn(__fmul_rn(__fsub_rn(x, l), sp), __fmul_rn(__fsub_rn(x, h), sn));
}

// Dense g.  The staging of first_layer_bwd_kernel (a channel group's g tile + 1 halo as coalesced
// float4 rows, the next group's loads in flight while the current one is consumed); per output pixel
// the chains S+ and S- run in the order (channel, dy, dx).  wpn = [2][C][9]: W+ then W-.
template <bool VEC>
__global__ __launch_bounds__(256) void zbox_bwd_kernel(const float* __restrict__ g, const float* __restrict__ wpn,
                                                       const float* __restrict__ xin, const float* __restrict__ low,
                                                       const float* __restrict__ high, float* __restrict__ out, int C,
                                                       int H, int W, int clones) {
  __shared__ __attribute__((aligned(16))) float hal[ZL_CC][ZL_HY][ZL_RS];
  const int tid = threadIdx.x;
  const int tiles_x = (W + ZL_TW - 1) / ZL_TW;
  const int ty0 = (blockIdx.x / tiles_x) * ZL_TH, tx0 = (blockIdx.x % tiles_x) * ZL_TW;
  const int bq = blockIdx.y;
  const int ly = tid / 16, lx = (tid % 16) * 4;   // 16 rows x 16 threads, 4 px each
  const size_t plane = (size_t)H * W;
  const int iplane = H * W;   // 32-bit per-lane offsets from the per-sample base (C * H * W < 2^31)
  const float* gb = g + (size_t)bq * C * plane;
  float4 rv[ZL_IV];
  float rh[ZL_IH];
  // loads from clamped (always valid) addresses, masked afterwards
  auto fetch = [&](int c0) {
#pragma unroll
    for (int it = 0; it < ZL_IV; ++it) {
      const int i = tid + it * 256;
      const int row = i / (ZL_TW / 4), q = i % (ZL_TW / 4);
      const int ci = row / ZL_HY, hy = row % ZL_HY;
      const int gy = ty0 - 1 + hy, gx = tx0 + 4 * q, c = c0 + ci;
      const bool rok = i < ZL_NV4 && c < C && gy >= 0 && gy < H;
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
    for (int it = 0; it < ZL_IH; ++it) {
      const int i = tid + it * 256;
      const int row = i >> 1, side = i & 1;
      const int ci = row / ZL_HY, hy = row % ZL_HY;
      const int gy = ty0 - 1 + hy, gx = side ? tx0 + ZL_TW : tx0 - 1, c = c0 + ci;
      const bool ok = i < ZL_ROWS * 2 && c < C && gy >= 0 && gy < H && gx >= 0 && gx < W;
      const float v = gb[ok ? c * iplane + gy * W + gx : 0];
      rh[it] = ok ? v : 0.f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int it = 0; it < ZL_IV; ++it) {
      const int i = tid + it * 256;
      if (i < ZL_NV4) {
        const int row = i / (ZL_TW / 4), q = i % (ZL_TW / 4);
        *reinterpret_cast<float4*>(&hal[row / ZL_HY][row % ZL_HY][4 + 4 * q]) = rv[it];
      }
    }
#pragma unroll
    for (int it = 0; it < ZL_IH; ++it) {
      const int i = tid + it * 256;
      if (i < ZL_ROWS * 2) {
        const int row = i >> 1, side = i & 1;
        hal[row / ZL_HY][row % ZL_HY][side ? 4 + ZL_TW : 3] = rh[it];
      }
    }
  };
  float sp[4] = {0.f, 0.f, 0.f, 0.f}, sn[4] = {0.f, 0.f, 0.f, 0.f};
  fetch(0);
  for (int c0 = 0; c0 < C; c0 += ZL_CC) {
    __syncthreads();
    stage();
    __syncthreads();
    if (c0 + ZL_CC < C) fetch(c0 + ZL_CC);
#pragma unroll 2
    for (int ci = 0; ci < ZL_CC; ++ci) {
      // channels past C were staged as zeros: fma(0, w, acc) == acc, so any finite weight will do
      const int c = min(c0 + ci, C - 1);
      float wp[9], wn[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        wp[t] = wpn[c * 9 + t];
        wn[t] = wpn[(C + c) * 9 + t];
      }
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const float* r = &hal[ci][ly + 1 + dy][3 + lx];      // pixel tx0 + lx - 1 ..
        const float4 m = *reinterpret_cast<const float4*>(r + 1);
        const float row[6] = {r[0], m.x, m.y, m.z, m.w, r[5]};
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int t = (1 - dy) * 3 + (1 - dx);
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            sp[p] = fmaf(row[p + 1 + dx], wp[t], sp[p]);
            sn[p] = fmaf(row[p + 1 + dx], wn[t], sn[p]);
          }
        }
      }
    }
  }
  const int y = ty0 + ly;
  if (y < H) {
    const float* xb = xin + (size_t)(bq / clones) * plane;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int x = tx0 + lx + p;
      if (x < W) {
        const int o = y * W + x;
        out[(size_t)bq * plane + o] = zbox_out(xb[o], low[o], high[o], sp[p], sn[p]);
      }
    }
  }
}

// Pool-sparse g (conv0 -> ReLU -> MaxPool2d(2)): first_layer_bwd_pooled_kernel with two chains.  A
// workgroup covers 16 x 64 pool cells (32 x 128 output pixels), each thread 2 x 2 cells = a 4 x 4
// pixel block.  Per channel the cells of the tile (+1 halo) are expanded to pixels while staging
// (value at the argmax position, zeros elsewhere; each staged cell clears the pixel it set for the
// previous channel), the next channel's cells are prefetched through range-checked buffer loads, and
// every thread streams its 6 x 6 patch row by row as five pixel pairs into packed fmas
// (v_pk_fma_f32), each pair once into S+ and once into S-, in the dense chain order (channel, dy, dx).
constexpr int ZQ_Y = 16, ZQ_X = 64;
constexpr int ZQ_RY = ZQ_Y + 2, ZQ_RX = ZQ_X + 2;            // cells incl. halo
constexpr int ZQ_PY = 2 * ZQ_RY, ZQ_PX = 2 * ZQ_RX + 4;      // pixel image (row pad 4)
constexpr int ZQ_KR = (ZQ_RY + 3) / 4;                       // row passes of 4 waves
constexpr int ZQ_C0 = 3;                                     // image column of the halo origin (16-byte patch rows)
constexpr int ZQ_NS = ZQ_KR + 1;                             // staged cells per thread

typedef float zq2 __attribute__((ext_vector_type(2)));

// W2C > 0: the pooled width as a compile-time constant (GTZAN: 64)
template <int W2C>
__global__ __launch_bounds__(256) void zbox_bwd_pooled_kernel(const float* __restrict__ g,
                                                              const uint8_t* __restrict__ amax,
                                                              const float* __restrict__ wpn,
                                                              const float* __restrict__ xin,
                                                              const float* __restrict__ low,
                                                              const float* __restrict__ high, float* __restrict__ out,
                                                              int C, int H, int W, int clones) {
  extern __shared__ __attribute__((aligned(16))) float img[];    // [ZQ_PY][ZQ_PX]
  const int tid = threadIdx.x, lane = tid & 63, wv4 = tid >> 6;
  const int H2 = H / 2, W2 = W2C > 0 ? W2C : W / 2;
  const int tiles_x = (W2 + ZQ_X - 1) / ZQ_X;
  const int qy0 = (blockIdx.x / tiles_x) * ZQ_Y, qx0 = (blockIdx.x % tiles_x) * ZQ_X;
  const int bq = blockIdx.y, bs = bq / clones;
  const int ty = tid / (ZQ_X / 2), tx = tid % (ZQ_X / 2);      // 8 x 32 threads, 2x2 cells each
  const size_t plane = (size_t)H2 * W2;
  const int iplane = H2 * W2;
  const float* gb = g + (size_t)bq * C * plane;
  const uint8_t* ab = amax + (size_t)bs * C * plane;
  // staging map: interior columns rx = 1 + lane, rows ry = wave + 4k; the two halo columns
  // (rx = 0, 65) of all rows by threads tid < 2 * ZQ_RY
  const int hr = tid % (2 * ZQ_RY);
  const int hry = hr >> 1, hrx = (hr & 1) ? ZQ_RX - 1 : 0;
  const bool hact = tid < 2 * ZQ_RY;
  zq2 sp[4][2], sn[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) sp[i][0] = sp[i][1] = sn[i][0] = sn[i][1] = zq2{0.f, 0.f};
  auto compute = [&](int c) {
    float wp[9], wn[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      wp[t] = wpn[c * 9 + t];
      wn[t] = wpn[(C + c) * 9 + t];
    }
    // patch P[i][j] = pixel (2qy0 + 4ty - 1 + i, 2qx0 + 4tx - 1 + j) = img[4ty + 1 + i][4tx + ZQ_C0 + 1 + j];
    // pair q (q = 0..4) = (P[i][q], P[i][q + 1])
    const float* base = img + (4 * ty + 1) * ZQ_PX + 4 * tx + ZQ_C0 + 1;
    // patch rows streamed: row i feeds output rows py = i - 1 - dy, i.e. each output row takes
    // its taps in dy order (then dx) -- the chain order -- with only one patch row live
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const float* r = base + i * ZQ_PX;
      const float4 q4 = *reinterpret_cast<const float4*>(r);
      const zq2 q2 = *reinterpret_cast<const zq2*>(r + 4);
      const zq2 rp[5] = {zq2{q4.x, q4.y}, zq2{q4.y, q4.z}, zq2{q4.z, q4.w}, zq2{q4.w, q2.x}, q2};
#pragma unroll
      for (int py = 0; py < 4; ++py) {
        const int dy = i - py - 1;
        if (dy < -1 || dy > 1) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int t = (1 - dy) * 3 + (1 - dx);
          const zq2 wwp = zq2{wp[t], wp[t]}, wwn = zq2{wn[t], wn[t]};
          sp[py][0] = __builtin_elementwise_fma(rp[1 + dx], wwp, sp[py][0]);
          sp[py][1] = __builtin_elementwise_fma(rp[3 + dx], wwp, sp[py][1]);
          sn[py][0] = __builtin_elementwise_fma(rp[1 + dx], wwn, sn[py][0]);
          sn[py][1] = __builtin_elementwise_fma(rp[3 + dx], wwn, sn[py][1]);
        }
      }
    }
  };
  // Cells through buffer loads: a per-channel descriptor (uniform) over the channel's plane, so a
  // cell above / below the image reads 0 (value and argmax byte) by the hardware range check, and
  // a cell left / right of it is pushed out of range by its lane offset.
  const int cxl = qx0 + lane;
  const unsigned OOR = 0x80000000u;   // >= any plane's byte size: the range check returns 0
  const unsigned lane_off = cxl < W2 ? (unsigned)(((qy0 - 1 + wv4) * W2 + cxl) * 4) : OOR;
  const int cxh = qx0 - 1 + hrx;
  const unsigned halo_off =
      (hact && cxh >= 0 && cxh < W2) ? (unsigned)(((qy0 - 1 + hry) * W2 + cxh) * 4) : OOR;
  const unsigned row4 = (unsigned)(4 * 4 * W2);   // 4 cell rows in bytes
  const unsigned pbytes = (unsigned)(iplane * 4);
  float vi[ZQ_NS];
  unsigned si[ZQ_NS];
  auto fetch = [&](int c) {
    unsigned lo = lane_off, ho = halo_off;
    asm volatile("" : "+v"(lo), "+v"(ho));
    // row k = 0 may lie above the image (a negative offset, out of range as unsigned); rows k >= 1
    // hang off a base that is never negative, so their offsets add as instruction immediates
    const unsigned lo1 = lo + row4;
    const unsigned la0 = lo >> 2, la1 = lo1 >> 2;   // the argmax plane's (byte) offsets are the cell indices
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(gb + (size_t)c * plane), 0, (int)pbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(ab + (size_t)c * plane), 0, (int)(pbytes / 4), 0x00020000);
#pragma unroll
    for (int k = 0; k < ZQ_KR; ++k) {
      // stays >= 2^31 (2^29 for the argmax plane) when lane_off is OOR
      const unsigned og = k == 0 ? lo : lo1 + (unsigned)(k - 1) * row4;
      const unsigned oa = k == 0 ? la0 : la1 + (unsigned)(k - 1) * (row4 / 4);
      vi[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, og, 0, 0));
      si[k] = __builtin_amdgcn_raw_buffer_load_b8(ra, oa, 0, 0);
    }
    vi[ZQ_NS - 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, ho, 0, 0));
    si[ZQ_NS - 1] = __builtin_amdgcn_raw_buffer_load_b8(ra, ho >> 2, 0, 0);
  };
  // LDS byte address of each staged cell's top-left pixel and of the pixel set last channel
  typedef __attribute__((address_space(3))) char lds_char;
  typedef __attribute__((address_space(3))) float lds_float;
  lds_char* const imgb = (lds_char*)img;
  int cell0[ZQ_NS];
  lds_float* prev[ZQ_NS];
#pragma unroll
  for (int k = 0; k < ZQ_KR; ++k) cell0[k] = 4 * (2 * (wv4 + 4 * k) * ZQ_PX + 2 * (1 + lane) + ZQ_C0);
  cell0[ZQ_NS - 1] = 4 * (2 * hry * ZQ_PX + 2 * hrx + ZQ_C0);
#pragma unroll
  for (int k = 0; k < ZQ_NS; ++k) prev[k] = (lds_float*)(imgb + cell0[k]);
  auto act = [&](int k) { return k == ZQ_NS - 1 ? hact : (wv4 + 4 * k < ZQ_RY); };
  for (int i = tid; i < ZQ_PY * ZQ_PX; i += 256) img[i] = 0.f;
  fetch(0);
  for (int c = 0; c < C; ++c) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ZQ_NS; ++k) {
      if (act(k)) {
        // argmax b = 2 row + col -> byte offset 4 col + 4 ZQ_PX row = 4 b + (4 ZQ_PX - 8) (b & 2)
        const int b = (int)(si[k] & 3u);
        lds_float* const nw = (lds_float*)(imgb + (cell0[k] + 4 * b + (4 * ZQ_PX - 8) / 2 * (b & 2)));
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
    const float* xb = xin + (size_t)bs * H * W;
#pragma unroll
    for (int py = 0; py < 4; ++py) {
      if (oy + py < H) {
        const int o = (oy + py) * W + ox;
        const float4 xv = *reinterpret_cast<const float4*>(xb + o);
        const float4 lv = *reinterpret_cast<const float4*>(low + o);
        const float4 hv = *reinterpret_cast<const float4*>(high + o);
        *reinterpret_cast<float4*>(out + (size_t)bq * H * W + o) =
            make_float4(zbox_out(xv.x, lv.x, hv.x, sp[py][0].x, sn[py][0].x),
                        zbox_out(xv.y, lv.y, hv.y, sp[py][0].y, sn[py][0].y),
                        zbox_out(xv.z, lv.z, hv.z, sp[py][1].x, sn[py][1].x),
                        zbox_out(xv.w, lv.w, hv.w, sp[py][1].y, sn[py][1].y));
      }
    }
  }
}

// zl[co][y][x] = sum_{in-bounds taps} low[yy][xx] w+[co][ky][kx] + b+[co], zh likewise with high, w-, b-:
// one fma chain per output in the tap order of first_layer_den_kernel, the bias added last
__global__ void zbox_maps_kernel(const float* __restrict__ wp, const float* __restrict__ bp,
                                 const float* __restrict__ wn, const float* __restrict__ bn,
                                 const float* __restrict__ low, const float* __restrict__ high, float* __restrict__ zl,
                                 float* __restrict__ zh, int C, int H, int W) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)C * H * W) return;
  const int co = (int)(i / ((size_t)H * W));
  const int y = (int)((i / W) % H), x = (int)(i % W);
  float al = 0.f, ah = 0.f;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      const int yy = y + ky - 1, xx = x + kx - 1;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        al = fmaf(low[yy * W + xx], wp[(co * 3 + ky) * 3 + kx], al);
        ah = fmaf(high[yy * W + xx], wn[(co * 3 + ky) * 3 + kx], ah);
      }
    }
  zl[i] = __fadd_rn(al, bp ? bp[co] : 0.f);
  zh[i] = __fadd_rn(ah, bn ? bn[co] : 0.f);
}

// den = (a - zl[at]) - zh[at]; a [B][C][Ha][Wa] at pool resolution (amax: at = the cell's argmax
// pixel of the 2Ha x 2Wa maps) or at full resolution (amax == nullptr: at = the pixel itself).  A workgroup
// takes 256 cells of one (sample, channel) plane, so the plane and the channel are uniform and the per-lane
// index arithmetic is 32-bit.  A pooled cell reads the pixel pair of its argmax row from each map (8-byte
// loads, contiguous over the lanes of a cell row) and picks the argmax column.
__global__ __launch_bounds__(256) void zbox_den_kernel(const float* __restrict__ a, const uint8_t* __restrict__ amax,
                                                       const float* __restrict__ zl, const float* __restrict__ zh,
                                                       float* __restrict__ den, int C, int Ha, int Wa, int chunks) {
  const int pl = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int j = chunk * 256 + threadIdx.x;   // the cell in its plane
  if (j >= Ha * Wa) return;
  const size_t i = (size_t)pl * ((size_t)Ha * Wa) + (size_t)j;
  const size_t zoff = (size_t)(pl % C) * ((size_t)Ha * Wa) * (amax ? 4 : 1);   // the channel's map
  float l, h;
  if (amax) {
    const int y = j / Wa, x = j % Wa;
    const int b = amax[i] & 3;
    const int at = (2 * y + (b >> 1)) * (2 * Wa) + 2 * x;   // the left pixel of the cell's argmax row
    const float2 lv = *reinterpret_cast<const float2*>(zl + zoff + at);
    const float2 hv = *reinterpret_cast<const float2*>(zh + zoff + at);
    l = (b & 1) ? lv.y : lv.x;
    h = (b & 1) ? hv.y : hv.x;
  } else {
    l = zl[zoff + j];
    h = zh[zoff + j];
  }
  den[i] = __fsub_rn(__fsub_rn(a[i], l), h);
}

}  // namespace

extern "C" {

int drsa_amd_first_layer_zbox_maps(const float* wp, const float* bp, const float* wn, const float* bn,
                                   const float* low_img, const float* high_img, float* zl, float* zh, int C, int H,
                                   int W, void* stream) {
  DRSA_REQUIRE(C > 0 && H > 0 && W > 0, "first_layer_zbox_maps: bad shape");
  DRSA_REQUIRE(wp && wn && low_img && high_img && zl && zh, "first_layer_zbox_maps: null pointer");
  const size_t n = (size_t)C * H * W;
  hipLaunchKernelGGL(zbox_maps_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wp, bp,
                     wn, bn, low_img, high_img, zl, zh, C, H, W);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

int drsa_amd_first_layer_zbox_den(const float* a, const uint8_t* amax, const float* zl, const float* zh, float* den,
                                  int B, int C, int H, int W, void* stream) {
  DRSA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "first_layer_zbox_den: bad shape");
  DRSA_REQUIRE(a && zl && zh && den, "first_layer_zbox_den: null pointer");
  DRSA_REQUIRE(!amax || (H % 2 == 0 && W % 2 == 0), "first_layer_zbox_den: pooled path needs even H and W");
  DRSA_REQUIRE((int64_t)C * H * W < ((int64_t)1 << 31),
               "first_layer_zbox_den: one sample's C x H x W must stay below 2^31");
  const int Ha = amax ? H / 2 : H, Wa = amax ? W / 2 : W;
  DRSA_REQUIRE(!amax || (((uintptr_t)zl | (uintptr_t)zh) & 7) == 0,
               "first_layer_zbox_den: pooled path loads pixel pairs: zl and zh must be 8-byte aligned");
  const int chunks = (Ha * Wa + 255) / 256;
  const int64_t blocks = (int64_t)B * C * chunks;
  DRSA_REQUIRE(blocks < ((int64_t)1 << 31), "first_layer_zbox_den: B x C x H x W too large for one launch");
  hipLaunchKernelGGL(zbox_den_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, amax, zl, zh, den,
                     C, Ha, Wa, chunks);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

int drsa_amd_first_layer_zbox_bwd(const float* g, const uint8_t* amax, const float* wpn, const float* x,
                                  const float* low_img, const float* high_img, float* out, int Bq, int clones, int C,
                                  int H, int W, void* stream) {
  DRSA_REQUIRE(Bq > 0 && clones > 0 && Bq % clones == 0, "first_layer_zbox_bwd: bad batch");
  DRSA_REQUIRE(C > 0 && H > 0 && W > 0, "first_layer_zbox_bwd: bad shape");
  DRSA_REQUIRE((int64_t)C * H * W < ((int64_t)1 << 31),
               "first_layer_zbox_bwd: one sample's C x H x W must stay below 2^31");
  DRSA_REQUIRE(g && wpn && x && low_img && high_img && out, "first_layer_zbox_bwd: null pointer");
  if (amax) {
    DRSA_REQUIRE(H % 2 == 0 && W % 4 == 0, "first_layer_zbox_bwd: pooled path needs even H and W % 4 == 0");
    DRSA_REQUIRE(((uintptr_t)out & 15) == 0,
                 "first_layer_zbox_bwd: pooled path stores float4: out must be 16-byte aligned");
    DRSA_REQUIRE((((uintptr_t)x | (uintptr_t)low_img | (uintptr_t)high_img) & 15) == 0,
                 "first_layer_zbox_bwd: pooled path loads float4: x, low_img and high_img must be 16-byte aligned");
    const int H2 = H / 2, W2 = W / 2;
    const dim3 grid(((H2 + ZQ_Y - 1) / ZQ_Y) * ((W2 + ZQ_X - 1) / ZQ_X), Bq);
    constexpr size_t lds = sizeof(float) * ZQ_PY * ZQ_PX;
    auto kf = W == 128 ? zbox_bwd_pooled_kernel<64> : zbox_bwd_pooled_kernel<0>;
    DRSA_SMEM(kf, lds);
    hipLaunchKernelGGL(kf, grid, dim3(256), lds, (hipStream_t)stream, g, amax, wpn, x, low_img, high_img, out, C, H, W,
                       clones);
  } else {
    const dim3 grid(((H + ZL_TH - 1) / ZL_TH) * ((W + ZL_TW - 1) / ZL_TW), Bq);
    // float4 loads of g rows when every row starts 16-byte aligned; any other base or width takes the
    // scalar loads (same chains, same values)
    if (W % 4 == 0 && ((uintptr_t)g & 15) == 0)
      hipLaunchKernelGGL(zbox_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g, wpn, x, low_img, high_img,
                         out, C, H, W, clones);
    else
      hipLaunchKernelGGL(zbox_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, g, wpn, x, low_img, high_img,
                         out, C, H, W, clones);
  }
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

}  // extern "C"
