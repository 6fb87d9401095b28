// Average pooling of a conv block (Conv2d -> [BN] -> ReLU -> AvgPool2d(k), stride = kernel, no padding), in
// both directions of the LRP engine.
//
// Forward: y = (sum of the window) / float(ph * pw), the sum one fp32 chain from 0 over the window in row-major
// order (rows outer, columns inner), then one IEEE division: torch's CPU avg_pool2d for contiguous NCHW, bit for
// bit.  No tree, whatever the window: a global pool is one chain per output.
//
// Backward: everything between the relevance at the pool's output and the dense g of the block's conv backward,
// one launch: the pool's rule (plain gradient, or Epsilon / Norm on the pool), the block's ReLU mask and the
// conv rule's own division.  Each thread owns four neighbouring pixels of one row (float4 rows); nothing is
// written and read again.
#include "common.h"
#include "drsa_amd.h"

namespace {

// ---- forward, pool width 1, 2 or 4: a thread reads one float4 of each of the window's ph rows and owns the
// 4 / PW outputs under it.  Every output's chain is still rows outer, columns inner.  One 64-bit division per
// thread: the channel map.  (Two or four float4 per row and thread, for a float4 of outputs, measured no faster.)
template <int PW>
__global__ __launch_bounds__(256) void avgpool_fwd_vec_kernel(const float* __restrict__ a, float* __restrict__ y,
                                                              int64_t BC, int H, int W, int ph, float k) {
  constexpr int NO = 4 / PW;
  const int WV = W / 4, H2 = H / ph, W2 = W / PW;
  const int per = H2 * WV;                  // threads per channel map
  const int64_t total = BC * per;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t bc = t / per;
    const int rem = (int)(t - bc * per);
    const int i = rem / WV, xq = rem - i * WV;
    const float* src = a + (bc * H + (int64_t)i * ph) * W + 4 * xq;
    float acc[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = 0.f;
    for (int u = 0; u < ph; ++u) {
      const float4 r = *reinterpret_cast<const float4*>(src + (int64_t)u * W);
      const float v[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e / PW] += v[e];
    }
    float* dst = y + (bc * H2 + i) * W2 + NO * xq;
    if constexpr (NO == 4) {
      *reinterpret_cast<float4*>(dst) = make_float4(acc[0] / k, acc[1] / k, acc[2] / k, acc[3] / k);
    } else if constexpr (NO == 2) {
      *reinterpret_cast<float2*>(dst) = make_float2(acc[0] / k, acc[1] / k);
    } else {
      dst[0] = acc[0] / k;
    }
  }
}

// ---- forward, any window: one thread per output walks its window
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const float* __restrict__ a, float* __restrict__ y, int64_t BC,
                                                          int H, int W, int ph, int pw, float k) {
  const int H2 = H / ph, W2 = W / pw;
  const int per = H2 * W2;
  const int64_t total = BC * per;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int64_t bc = o / per;
    const int rem = (int)(o - bc * per);
    const int i = rem / W2, j = rem - i * W2;
    const float* src = a + (bc * H + (int64_t)i * ph) * W + (int64_t)j * pw;
    float acc = 0.f;
    for (int u = 0; u < ph; ++u)
      for (int v = 0; v < pw; ++v) acc += src[(int64_t)u * W + v];
    y[o] = acc / k;
  }
}

// what a window hands each of its pixels before the pixel's own factor: R / K under the plain gradient,
// (R / stab(y, eps)) / K under Epsilon / Norm on the pool
template <bool RULE>
__device__ __forceinline__ float window_share(const float* __restrict__ R, const float* __restrict__ y, int64_t ro,
                                              int64_t yo, float eps_pool, float k) {
  float r = R[ro];
  if constexpr (RULE) r = r / stab(y[yo], eps_pool);
  return r / k;
}

// ---- backward: thread t owns pixels 4 t .. 4 t + 3 of the full-resolution map [Bq][C][H][W] (W % 4 == 0, so the
// four share a row).  PW = 1, 2, 4: the pool width at compile time (the four pixels lie in 4 / PW windows);
// PW = 0: any width, the window looked up per pixel and kept while it does not change.
template <int PW, bool RULE>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ R, const float* __restrict__ y,
                                                          const float* __restrict__ a, const float* __restrict__ den,
                                                          int den_bcast, float eps_pool, float eps_conv,
                                                          float* __restrict__ g, float* __restrict__ rel_full,
                                                          int64_t total4, int clones, int C, int H, int W, int ph,
                                                          int pw_rt, float k) {
  const int pw = PW ? PW : pw_rt;
  const int W4 = W / 4, H2 = H / ph, W2 = W / pw;
  const int per = H * W4;                   // threads per channel map (below 2^31: the entry point's check)
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total4; t += (int64_t)gridDim.x * 256) {
    const int qc32 = (int)(t / per);        // q * C + c: the one 64-bit division; Bq * C is below 2^31
    const int rem = (int)(t - (int64_t)qc32 * per);
    const int yy = rem / W4, xq = rem - yy * W4;
    const int q = qc32 / C, c = qc32 - q * C;
    const int64_t qc = qc32;
    const int64_t sc = (int64_t)(q / clones) * C + c;   // the sample's channel map: a, y, den
    const int i = yy / ph;
    const int64_t ao = (sc * H + yy) * W + 4 * xq;
    const int64_t ro = (qc * H2 + i) * W2, yo = (sc * H2 + i) * W2;
    const float4 a4 = *reinterpret_cast<const float4*>(a + ao);
    const float av[4] = {a4.x, a4.y, a4.z, a4.w};
    float s[4];
    if constexpr (PW == 0) {
      int jl = -1;
      float sl = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = (4 * xq + e) / pw;
        if (j != jl) {
          sl = window_share<RULE>(R, y, ro + j, yo + j, eps_pool, k);
          jl = j;
        }
        s[e] = sl;
      }
    } else {
      constexpr int NW = 4 / (PW ? PW : 1);
      float sw[NW];
#pragma unroll
      for (int o = 0; o < NW; ++o) {
        const int j = NW * xq + o;
        sw[o] = window_share<RULE>(R, y, ro + j, yo + j, eps_pool, k);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = sw[e / (PW ? PW : 1)];
    }
    float tv[4], gv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) tv[e] = RULE ? av[e] * s[e] : s[e];
    if (rel_full) *reinterpret_cast<float4*>(rel_full + 4 * t) = make_float4(tv[0], tv[1], tv[2], tv[3]);
    if (den) {
      const int64_t dofs = den_bcast ? (((int64_t)c * H + yy) * W + 4 * xq) : ao;
      const float4 d4 = *reinterpret_cast<const float4*>(den + dofs);
      const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = (av[e] > 0.f) ? div_nb(tv[e], stab(dv[e], eps_conv)) : 0.f;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = (av[e] > 0.f) ? tv[e] : 0.f;
    }
    *reinterpret_cast<float4*>(g + 4 * t) = make_float4(gv[0], gv[1], gv[2], gv[3]);
  }
}

unsigned pool_grid(int64_t total) {
  const int64_t g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int PW>
void launch_bwd(bool rule, hipStream_t st, const float* R, const float* y, const float* a, const float* den,
                int den_bcast, float eps_pool, float eps_conv, float* g, float* rel_full, int64_t total4, int clones,
                int C, int H, int W, int ph, int pw) {
  const float k = (float)(ph * pw);
  if (rule) {
    hipLaunchKernelGGL((avgpool_bwd_kernel<PW, true>), dim3(pool_grid(total4)), dim3(256), 0, st, R, y, a, den,
                       den_bcast, eps_pool, eps_conv, g, rel_full, total4, clones, C, H, W, ph, pw, k);
  } else {
    hipLaunchKernelGGL((avgpool_bwd_kernel<PW, false>), dim3(pool_grid(total4)), dim3(256), 0, st, R, y, a, den,
                       den_bcast, eps_pool, eps_conv, g, rel_full, total4, clones, C, H, W, ph, pw, k);
  }
}

}  // namespace

extern "C" int drsa_amd_avgpool_fwd(const float* a, float* y, int B, int C, int H, int W, int ph, int pw,
                                    void* stream) {
  DRSA_REQUIRE(a && y, "avgpool_fwd: null pointer");
  DRSA_REQUIRE(ph >= 1 && pw >= 1, "avgpool_fwd: bad pool kernel %dx%d", ph, pw);
  DRSA_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0 && H % ph == 0 && W % pw == 0,
               "avgpool_fwd: bad shape (the map's sides must be multiples of the pool's)");
  if (B == 0) return DRSA_OK;
  const int64_t BC = (int64_t)B * C;
  const float k = (float)(ph * pw);
  hipStream_t st = (hipStream_t)stream;
  DRSA_REQUIRE((int64_t)H * W < (1ll << 31), "avgpool_fwd: one channel map must stay below 2^31 elements");
  if ((pw == 1 || pw == 2 || pw == 4) && W % 4 == 0 && aligned16(a) && aligned16(y)) {
    const unsigned grid = pool_grid(BC * (H / ph) * (W / 4));
    if (pw == 1) hipLaunchKernelGGL(avgpool_fwd_vec_kernel<1>, dim3(grid), dim3(256), 0, st, a, y, BC, H, W, ph, k);
    if (pw == 2) hipLaunchKernelGGL(avgpool_fwd_vec_kernel<2>, dim3(grid), dim3(256), 0, st, a, y, BC, H, W, ph, k);
    if (pw == 4) hipLaunchKernelGGL(avgpool_fwd_vec_kernel<4>, dim3(grid), dim3(256), 0, st, a, y, BC, H, W, ph, k);
  } else {
    hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(pool_grid(BC * (H / ph) * (W / pw))), dim3(256), 0, st, a, y, BC, H, W,
                       ph, pw, k);
  }
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

extern "C" int drsa_amd_avgpool_bwd(const float* R_y, const float* y, const float* a, const float* den, int den_bcast,
                                    int rule, float eps_pool, float eps_conv, float* g, float* rel_full, int Bq,
                                    int clones, int C, int H, int W, int ph, int pw, void* stream) {
  DRSA_REQUIRE(R_y && a && g, "avgpool_bwd: null pointer");
  DRSA_REQUIRE(rule == 0 || rule == 1, "avgpool_bwd: rule must be 0 (plain gradient) or 1 (Epsilon / Norm)");
  DRSA_REQUIRE(rule == 0 || y, "avgpool_bwd: the Epsilon / Norm rule needs the pool's output y");
  DRSA_REQUIRE(den_bcast == 0 || den_bcast == 1, "avgpool_bwd: den_bcast must be 0 or 1");
  DRSA_REQUIRE(clones >= 1 && Bq >= 0 && Bq % clones == 0, "avgpool_bwd: bad clones");
  DRSA_REQUIRE(ph >= 1 && pw >= 1, "avgpool_bwd: bad pool kernel %dx%d", ph, pw);
  DRSA_REQUIRE(C > 0 && H > 0 && W > 0 && H % ph == 0 && W % pw == 0,
               "avgpool_bwd: bad shape (the map's sides must be multiples of the pool's)");
  DRSA_REQUIRE(W % 4 == 0, "avgpool_bwd: the map width must be a multiple of 4 (float4 rows)");
  DRSA_REQUIRE(aligned16(a) && aligned16(g) && aligned16(den) && aligned16(rel_full),
               "avgpool_bwd: a, den, g and rel_full must be 16-byte aligned");
  DRSA_REQUIRE((int64_t)H * W < (1ll << 31) && (int64_t)Bq * C < (1ll << 31),
               "avgpool_bwd: one channel map, and the number of them, must stay below 2^31");
  if (Bq == 0) return DRSA_OK;
  const int64_t total4 = (int64_t)Bq * C * H * (W / 4);
  hipStream_t st = (hipStream_t)stream;
#define DRSA_AVG_BWD(PWT) \
  launch_bwd<PWT>(rule != 0, st, R_y, y, a, den, den_bcast, eps_pool, eps_conv, g, rel_full, total4, clones, C, H, W, ph, pw)
  if (pw == 1) {
    DRSA_AVG_BWD(1);
  } else if (pw == 2) {
    DRSA_AVG_BWD(2);
  } else if (pw == 4) {
    DRSA_AVG_BWD(4);
  } else {
    DRSA_AVG_BWD(0);
  }
#undef DRSA_AVG_BWD
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}
