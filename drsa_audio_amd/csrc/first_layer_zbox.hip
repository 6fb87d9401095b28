// LRP first layer under the ZBox rule (zennit 0.5.1 ZBox), one input channel, for an
// input that lives in a box low <= x <= high:
//   * the rule's two input-independent maps  zl = conv(low; W+) + b+,  zh = conv(high; W-) + b-
//   * the per-sample denominator copy        den = (a - zl[at]) - zh[at]
//   * backward  R[y][x] = (x - low) S+ + (x - high) S-,  S+- = sum_co sum_{dy,dx} G[co][y+dy][x+dx] W+-[co][1-dy][1-dx]
//               the two-chain kernels of first_layer_bwd.h (wpn = [2][C][9]: W+ then W-), G dense or pool-sparse
// Every tap of W is in exactly one of W+ = max(W, 0), W- = min(W, 0), so the two chains are zennit's
// three-term reducer x J^T_W g - l J^T_{W+} g - h J^T_{W-} g with the terms grouped by weight sign; the
// factors x - low >= 0 >= x - high do not cancel.
#include "first_layer_bwd.h"

namespace {

// out = (x - l) sp + (x - h) sn: four roundings and a fifth for the sum, none contracted
__device__ __forceinline__ float zbox_out(float x, float l, float h, float sp, float sn) {
  return __fadd_rn(__fmul_rn(__fsub_rn(x, l), sp), __fmul_rn(__fsub_rn(x, h), sn));
}

// the two-chain epilogue: x [Bq / clones][H x W] (so: the sample's plane), low and high [H x W]
struct ZBoxOut {
  const float *x, *low, *high;
  __device__ float px(size_t so, int o, const float (&s)[2]) const {
    return zbox_out(x[so + o], low[o], high[o], s[0], s[1]);
  }
  __device__ float4 px4(size_t so, int o, const float4 (&s)[2]) const {
    const float4 xv = *reinterpret_cast<const float4*>(x + so + o);
    const float4 lv = *reinterpret_cast<const float4*>(low + o);
    const float4 hv = *reinterpret_cast<const float4*>(high + o);
    return make_float4(zbox_out(xv.x, lv.x, hv.x, s[0].x, s[1].x), zbox_out(xv.y, lv.y, hv.y, s[0].y, s[1].y),
                       zbox_out(xv.z, lv.z, hv.z, s[0].z, s[1].z), zbox_out(xv.w, lv.w, hv.w, s[0].w, s[1].w));
  }
};

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
  DRSA_REQUIRE(C > 0 && H > 0 && W > 0, "first_layer_zbox_bwd: bad shape");
  DRSA_REQUIRE(g && wpn && x && low_img && high_img && out, "first_layer_zbox_bwd: null pointer");
  DRSA_REQUIRE(!amax || (((uintptr_t)x | (uintptr_t)low_img | (uintptr_t)high_img) & 15) == 0,
               "first_layer_zbox_bwd: pooled path loads float4: x, low_img and high_img must be 16-byte aligned");
  return first_layer_bwd_launch<2, ZBoxOut>("first_layer_zbox_bwd", g, amax, wpn, out, Bq, clones, C, H, W, stream, x,
                                            low_img, high_img);
}

}  // extern "C"
