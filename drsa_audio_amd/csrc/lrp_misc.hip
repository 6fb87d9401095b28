// LRP engine kernels that belong to no layer family:
//   * heatmap split / per-subspace sums / descending sort (explainer.py:99-176)
//   * AlphaBeta split / combine around two plain backward convs (pf.py:289)
//   * the post step of a layer as a launch of its own (multi-layer DRSA capture)
// The dense head is in linear.hip, the ProjectionModel layers in projection.hip, the first-layer
// backward and its denominator map in first_layer.hip.
#include "common.h"
#include "lrp_conv.h"

namespace {

// ===========================================================================
// heatmap finalisation (per sample): hm [B][K+1][H*W]
//   std_out [B][HW], std_rel [B], sub_out [B][K][HW] sorted by descending relevance,
//   rel [B][K] sorted, mask [B][K] int64 (numpy argsort(...)[..., ::-1] semantics:
//   stable ascending order reversed, i.e. ties -> larger index first)
//
// The per-map relevance is the reference's numpy float32 sum over the last two axes
// (explainer.py:161, :120): chunks of 8192 elements folded left to right into 0, each chunk by
// numpy's pairwise summation -- n < 8: a plain left-to-right chain; n <= 128: eight strided
// accumulators r[j] = a[j] + a[8+j] + ... combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then
// the n % 8 tail; n > 128: split at n2 = n/2 - (n/2 % 8) and add the two halves' sums.  For
// n = 128 * 2^m the leaves are the 128-element blocks and the tree over them is balanced (a
// butterfly); other n take a serial walk of the same recursion.  Bit-identical to numpy (pinned
// by tests/golden/lrp_pins_fixture.npz).
// ===========================================================================
__device__ float pw_leaf(const float* a, int n) {   // numpy pairwise_sum for n <= 128
  if (n < 8) {
    float r = 0.f;
    for (int i = 0; i < n; ++i) r = r + a[i];
    return r;
  }
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
  float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res = res + a[i];
  return res;
}

__device__ float pw_serial(const float* a, int n) {   // the full recursion, one thread
  struct Fr { int lo, n, state; float left; };
  Fr st[32];
  int sp = 0;
  float ret = 0.f;
  st[0] = {0, n, 0, 0.f};
  while (sp >= 0) {
    Fr& f = st[sp];
    if (f.n <= 128) { ret = pw_leaf(a + f.lo, f.n); --sp; continue; }
    int n2 = f.n / 2;
    n2 -= n2 % 8;
    if (f.state == 0) { f.state = 1; st[sp + 1] = {f.lo, n2, 0, 0.f}; ++sp; continue; }
    if (f.state == 1) { f.state = 2; f.left = ret; st[sp + 1] = {f.lo + n2, f.n - n2, 0, 0.f}; ++sp; continue; }
    ret = f.left + ret;
    --sp;
  }
  return ret;
}

// half-leaf partial of the balanced case: thread (leaf L, half h) owns accumulators 4h..4h+3 of
// leaf L; returns ((r_4h + r_4h+1) + (r_4h+2 + r_4h+3)) -- the leaf is the two halves' sum
__device__ __forceinline__ float pw_half(const float4* leaf, int h) {
  float4 r = leaf[h];
#pragma unroll
  for (int i = 1; i < 16; ++i) {
    const float4 v = leaf[2 * i + h];
    r.x = r.x + v.x; r.y = r.y + v.y; r.z = r.z + v.z; r.w = r.w + v.w;
  }
  return (r.x + r.y) + (r.z + r.w);
}

// numpy pairwise sum of one run of n <= 8192 by the whole workgroup (256 threads); part: >= 128
// floats of LDS.  Result valid in every thread.  Contains barriers: call uniformly.
__device__ float pw_chunk_wg(const float* __restrict__ src, int n, float* part, float* bc) {
  const int tid = threadIdx.x;
  const int leaves = n / 128;
  if (n > 128 && n % 128 == 0 && (leaves & (leaves - 1)) == 0) {     // balanced: <= 64 leaves
    if (tid < 2 * leaves) part[tid] = pw_half(reinterpret_cast<const float4*>(src) + (size_t)(tid >> 1) * 32, tid & 1);
    __syncthreads();
    for (int w = 2 * leaves; w > 1; w >>= 1) {      // halves -> leaves -> balanced tree, adjacent pairs
      const float v = tid < w / 2 ? part[2 * tid] + part[2 * tid + 1] : 0.f;
      __syncthreads();
      if (tid < w / 2) part[tid] = v;
      __syncthreads();
    }
    const float r = part[0];
    __syncthreads();
    return r;
  }
  if (tid == 0) *bc = pw_serial(src, n);
  __syncthreads();
  const float r = *bc;
  __syncthreads();
  return r;
}

// numpy's float32 sum of a contiguous run: the reduction iterator feeds the inner loop chunks of
// 8192 elements (its buffer size), folded left to right into the identity 0, each chunk summed
// pairwise (oracle/lrp_ref.py numpy_pairwise_sum).
__device__ float pw_sum_wg(const float* __restrict__ src, int n, float* part, float* bc) {
  float acc = 0.f;
  for (int lo = 0; lo < n; lo += 8192) acc = acc + pw_chunk_wg(src + lo, n - lo < 8192 ? n - lo : 8192, part, bc);
  return acc;
}

__device__ void sort_desc(const float* sums, int K, int* order) {   // descending; ties: larger index first
  for (int k = 0; k < K; ++k) order[k] = k;
  for (int i = 1; i < K; ++i) {
    const int cur = order[i];
    int j = i - 1;
    while (j >= 0) {
      const float a = sums[1 + order[j]], c = sums[1 + cur];
      const bool before = (c > a) || (c == a && cur > order[j]);
      if (!before) break;
      order[j + 1] = order[j];
      --j;
    }
    order[j + 1] = cur;
  }
}

__global__ __launch_bounds__(256) void heatmap_sort_kernel(const float* __restrict__ hm, int K, int HW, int std_sum,
                                                           float* __restrict__ std_out, float* __restrict__ std_rel,
                                                           float* __restrict__ sub_out, float* __restrict__ rel,
                                                           int64_t* __restrict__ mask) {
  __shared__ float part[128];
  __shared__ float bc;
  __shared__ float sums[65];
  __shared__ int order[64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int NM = std_sum ? K : K + 1;              // maps per sample in hm
  const float* base = hm + (size_t)b * NM * HW;
  const float* sub0 = base + (std_sum ? 0 : (size_t)HW);
  float* so = std_out + (size_t)b * HW;
  // the standard map: clone 0, or (std_sum) the sum of the K concept maps, k ascending
  for (int i = tid * 4; i < HW; i += 256 * 4) {
    float4 v = *reinterpret_cast<const float4*>(std_sum ? sub0 + i : base + i);
    for (int k = 1; std_sum && k < K; ++k) {
      const float4 u = *reinterpret_cast<const float4*>(sub0 + (size_t)k * HW + i);
      v.x = v.x + u.x; v.y = v.y + u.y; v.z = v.z + u.z; v.w = v.w + u.w;
    }
    *reinterpret_cast<float4*>(so + i) = v;
  }
  __syncthreads();                                  // std_out complete and visible to the block
  {
    const float s0 = pw_sum_wg(so, HW, part, &bc);
    if (tid == 0) sums[0] = s0;
  }
  for (int q = 0; q < K; ++q) {
    const float sq = pw_sum_wg(sub0 + (size_t)q * HW, HW, part, &bc);
    if (tid == 0) sums[1 + q] = sq;
  }
  __syncthreads();
  if (tid == 0) {
    sort_desc(sums, K, order);
    std_rel[b] = sums[0];
    for (int k = 0; k < K; ++k) {
      rel[(size_t)b * K + k] = sums[1 + order[k]];
      mask[(size_t)b * K + k] = order[k];
    }
  }
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    const float* src = sub0 + (size_t)order[k] * HW;
    float* dst = sub_out + ((size_t)b * K + k) * HW;
    for (int i = tid * 4; i < HW; i += 256 * 4)
      *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
  }
}

// The same split / sums / sort with every map read ONCE: at K = 4 and H*W = 16384 (GTZAN-128, the
// headline) each thread keeps its 16 float4 of the K subspace maps in registers (one workgroup per
// CU; the kernel is HBM-bound) and copies the standard map while loading it, so the sorted writes
// need no second read.  The numpy pairwise sums need each accumulator chain (stride-8 elements of
// one 128-element leaf) in one thread, so thread t = (leaf t/2, half t%2) loads the float4s
// 32 leaf + 2 i + half, i = 0..15: its four chains in order (a wave's load covers 32 B of each of
// 32 leaves; the four loads i..i+3 complete each 128-B line).  Outputs equal heatmap_sort_kernel's.
template <int KC, int NV4, bool SSUM>
__global__ __launch_bounds__(256) void heatmap_sort_cached_kernel(const float* __restrict__ hm, float* __restrict__ std_out,
                                                                  float* __restrict__ std_rel,
                                                                  float* __restrict__ sub_out, float* __restrict__ rel,
                                                                  int64_t* __restrict__ mask) {
  constexpr int HW = NV4 * 1024;
  static_assert(HW / 128 * 2 == 256 && NV4 == 16, "cached sort: one (leaf, half) per thread, 16 float4 each");
  __shared__ float red[KC + 1][4];
  __shared__ float sums[KC + 1];
  __shared__ int order[KC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = tid >> 1, hh = tid & 1;
  constexpr int NM = SSUM ? KC : KC + 1;            // maps per sample in hm
  const float4* base = reinterpret_cast<const float4*>(hm + (size_t)b * NM * HW) + 32 * L + hh;
  const float4* sub0 = base + (SSUM ? 0 : HW / 4);
  float4* so = reinterpret_cast<float4*>(std_out + (size_t)b * HW) + 32 * L + hh;
  float4 v[KC][NV4];
  float s[KC + 1];
  auto chain = [&](const float4* x) -> float {   // pw_half on registers, then the leaf
    float4 r = x[0];
#pragma unroll
    for (int i = 1; i < NV4; ++i) {
      r.x = r.x + x[i].x; r.y = r.y + x[i].y; r.z = r.z + x[i].z; r.w = r.w + x[i].w;
    }
    const float p = (r.x + r.y) + (r.z + r.w);
    return p + shfl_xor(p, 1);
  };
  {
    float4 w[NV4];
    if constexpr (!SSUM) {
#pragma unroll
      for (int i = 0; i < NV4; ++i) w[i] = base[2 * i];
    }
#pragma unroll
    for (int q = 0; q < KC; ++q)
#pragma unroll
      for (int i = 0; i < NV4; ++i) v[q][i] = sub0[(size_t)q * (HW / 4) + 2 * i];
    if constexpr (SSUM) {   // the standard map = the concept maps summed, k ascending
#pragma unroll
      for (int i = 0; i < NV4; ++i) {
        float4 t = v[0][i];
#pragma unroll
        for (int q = 1; q < KC; ++q) {
          t.x = t.x + v[q][i].x; t.y = t.y + v[q][i].y; t.z = t.z + v[q][i].z; t.w = t.w + v[q][i].w;
        }
        w[i] = t;
      }
    }
#pragma unroll
    for (int i = 0; i < NV4; ++i) so[2 * i] = w[i];
    s[0] = chain(w);
  }
#pragma unroll
  for (int q = 0; q < KC; ++q) s[1 + q] = chain(v[q]);
  // balanced tree over the leaves: lanes 2L, 2L+1 hold leaf L; in-wave butterfly over L; waves
  // 0-1 hold the first 8192-element chunk, 2-3 the second: (0 + (w0 + w1)) + (w2 + w3)
#pragma unroll
  for (int q = 0; q <= KC; ++q) {
    float a = s[q];
    for (int m = 2; m <= 32; m <<= 1) a = a + shfl_xor(a, m);
    if (lane_id() == 0) red[q][wave_id()] = a;
  }
  __syncthreads();
  if (tid == 0) {
    for (int q = 0; q <= KC; ++q) sums[q] = (0.f + (red[q][0] + red[q][1])) + (red[q][2] + red[q][3]);
    sort_desc(sums, KC, order);
    std_rel[b] = sums[0];
    for (int k = 0; k < KC; ++k) {
      rel[(size_t)b * KC + k] = sums[1 + order[k]];
      mask[(size_t)b * KC + k] = order[k];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const int src = order[k];   // uniform: the branch below is a scalar one
    float4* dst = reinterpret_cast<float4*>(sub_out + ((size_t)b * KC + k) * HW) + 32 * L + hh;
#pragma unroll
    for (int q = 0; q < KC; ++q)
      if (src == q) {
#pragma unroll
        for (int i = 0; i < NV4; ++i) dst[2 * i] = v[q][i];
      }
  }
}

// ===========================================================================
// AlphaBeta (zennit 0.5.1 AlphaBeta, reference pf.py:289) on a conv with non-negative input,
// around two plain backward convs (the x- terms vanish):
//   split:   gp = R / stab(den_p), gn = R / stab(den_n)          (per element of the conv output;
//            den per sample, R rows are sample*clones + clone)
//   combine: R_in = alpha * (x J^T_{W+} gp) - beta * (x J^T_{W-} gn)   (two roundings each, no fma)
//            then the post step of the layer below, as the conv epilogue: x > 0 ? R / stab(den) : 0
//            (POST_DIV), x > 0 ? R : 0 (POST_MASK) or R.
// ===========================================================================
__global__ __launch_bounds__(256) void ab_split_kernel(const float* __restrict__ g, const float* __restrict__ dp,
                                                       const float* __restrict__ dn, float* __restrict__ gp,
                                                       float* __restrict__ gn, int64_t n, int clones, int64_t total,
                                                       float eps) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t bq = i / n, j = i - bq * n;
    const int64_t o = (bq / clones) * n + j;
    const float r = g[i];
    gp[i] = div_nb(r, stab(dp[o], eps));
    gn[i] = div_nb(r, stab(dn[o], eps));
  }
}

// The post step of the layer below on one element, as the conv epilogue takes it (lrp_conv_kernel.h): the quotient
// by the stabilised denominator (POST_DIV; dv is not read otherwise), then the ReLU mask of the layer's input.  No fma.
__device__ __forceinline__ float post_value(float R, float xv, float dv, int post, float eps) {
  if (post == POST_DIV) R = div_nb(R, stab(dv, eps));
  return (xv > 0.f) ? R : 0.f;
}

__global__ __launch_bounds__(256) void ab_combine_kernel(const float* __restrict__ pos, const float* __restrict__ neg,
                                                         float alpha, float beta, const float* __restrict__ x,
                                                         const float* __restrict__ den, float* __restrict__ out,
                                                         int64_t n, int clones, int64_t total, int post, float eps) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t bq = i / n, j = i - bq * n;
    const int64_t o = (bq / clones) * n + j;
    const float a = alpha * pos[i];
    const float b = beta * neg[i];
    float R = a - b;
    if (post != POST_NONE) R = post_value(R, x[o], post == POST_DIV ? den[o] : 0.f, post, eps);
    out[i] = R;
  }
}

// ===========================================================================
// The post step alone (POST_DIV or POST_MASK), for a relevance R that a backward launch wrote raw (POST_NONE) so
// that it could be kept: out = post(R), R and out [Bq][n] (out may be R), x and den [Bq / clones][n].
// V4: four elements per thread (n % 4 == 0 and every pointer 16-byte aligned: a group never leaves its row).
// ===========================================================================
template <bool V4>
__global__ __launch_bounds__(256) void relevance_post_kernel(const float* R, const float* __restrict__ x,
                                                             const float* __restrict__ den, float* out, int64_t n,
                                                             int clones, int64_t total, int post, float eps) {
  constexpr int E = V4 ? 4 : 1;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t * E < total; t += (int64_t)gridDim.x * 256) {
    const int64_t i = t * E;
    const int64_t bq = i / n, j = i - bq * n;
    const int64_t o = (bq / clones) * n + j;
    if constexpr (V4) {
      const float4 r = *reinterpret_cast<const float4*>(R + i);
      const float4 xv = *reinterpret_cast<const float4*>(x + o);
      const float4 d = post == POST_DIV ? *reinterpret_cast<const float4*>(den + o) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(out + i) =
          make_float4(post_value(r.x, xv.x, d.x, post, eps), post_value(r.y, xv.y, d.y, post, eps),
                      post_value(r.z, xv.z, d.z, post, eps), post_value(r.w, xv.w, d.w, post, eps));
    } else {
      out[i] = post_value(R[i], x[o], post == POST_DIV ? den[o] : 0.f, post, eps);
    }
  }
}

unsigned ew_grid(int64_t total) {
  const int64_t g = (total + 255) / 256;
  return (unsigned)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

}  // namespace

extern "C" {

int drsa_amd_heatmap_sort(const float* hm, int B, int K, int HW, int std_from_sum, float* std_out, float* std_rel,
                          float* sub_out, float* rel, int64_t* mask, void* stream) {
  DRSA_REQUIRE(K >= 1 && K <= 64, "heatmap_sort: K must be in [1, 64]");
  DRSA_REQUIRE(HW % 4 == 0, "heatmap_sort: H*W must be a multiple of 4");
  if (K == 4 && HW == 16384) {
    auto kern = std_from_sum ? heatmap_sort_cached_kernel<4, 16, true> : heatmap_sort_cached_kernel<4, 16, false>;
    hipLaunchKernelGGL(kern, dim3(B), dim3(256), 0, (hipStream_t)stream, hm, std_out, std_rel, sub_out, rel, mask);
  } else {
    hipLaunchKernelGGL(heatmap_sort_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, hm, K, HW, std_from_sum ? 1 : 0,
                       std_out, std_rel, sub_out, rel, mask);
  }
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

int drsa_amd_ab_split(const float* g, const float* den_p, const float* den_n, float* gp, float* gn, int Bq,
                      int clones, int64_t n, float eps, void* stream) {
  DRSA_REQUIRE(g && den_p && den_n && gp && gn, "ab_split: null pointer");
  DRSA_REQUIRE(Bq > 0 && clones > 0 && Bq % clones == 0 && n > 0, "ab_split: bad shape");
  const int64_t total = (int64_t)Bq * n;
  hipLaunchKernelGGL(ab_split_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, g, den_p, den_n, gp, gn,
                     n, clones, total, eps);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

int drsa_amd_ab_combine(const float* pos, const float* neg, float alpha, float beta, const float* x, const float* den,
                        float* out, int Bq, int clones, int64_t n, int post, float eps, void* stream) {
  DRSA_REQUIRE(pos && neg && out, "ab_combine: null pointer");
  DRSA_REQUIRE(Bq > 0 && clones > 0 && Bq % clones == 0 && n > 0, "ab_combine: bad shape");
  DRSA_REQUIRE(post == POST_NONE || (x && (den || post == POST_MASK)), "ab_combine: post needs x (and den)");
  const int64_t total = (int64_t)Bq * n;
  hipLaunchKernelGGL(ab_combine_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, pos, neg, alpha,
                     beta, x, den, out, n, clones, total, post, eps);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

int drsa_amd_relevance_post(const float* R, const float* x, const float* den, float* out, int Bq, int clones,
                            int64_t n, int post, float eps, void* stream) {
  DRSA_REQUIRE(post == POST_DIV || post == POST_MASK, "relevance_post: post must be POST_DIV or POST_MASK");
  DRSA_REQUIRE(R && x && out && (den || post == POST_MASK), "relevance_post: null pointer");
  DRSA_REQUIRE(Bq > 0 && clones > 0 && Bq % clones == 0 && n > 0, "relevance_post: bad shape");
  const int64_t total = (int64_t)Bq * n;
  const uintptr_t bits = (uintptr_t)R | (uintptr_t)x | (uintptr_t)out | (post == POST_DIV ? (uintptr_t)den : 0);
  if (n % 4 == 0 && bits % 16 == 0) {
    hipLaunchKernelGGL(relevance_post_kernel<true>, dim3(ew_grid(total / 4)), dim3(256), 0, (hipStream_t)stream, R, x,
                       den, out, n, clones, total, post, eps);
  } else {
    hipLaunchKernelGGL(relevance_post_kernel<false>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, R, x,
                       den, out, n, clones, total, post, eps);
  }
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

}  // extern "C"
