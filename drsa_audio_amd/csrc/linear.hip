// LRP dense head (classifier Linear layers; Epsilon rule, reference constants.py:35-37):
// C[M][N] = A[M][K] B[K][N] on fp32 MFMA 16x16x4, 32x32 workgroup tile
//   forward : A = x,  B[k][n] = W[n][k];  z = acc + b;  optional a = relu(z)
//   backward: A[m][n] = g = prologue(R | seed, z), B[n][k] = W[n][k];  out = epilogue(acc, x, den)
#include "common.h"
#include "lrp_conv.h"

namespace {

constexpr int LT = 32;   // workgroup tile (M and N)
constexpr int LK = 32;   // K chunk

struct LinArgs {
  const float* A;        // fwd: x [M][K]; bwd: R [M][Kg] (ignored when seed)
  const float* W;        // [Nout][Kin] (torch Linear weight)
  const float* bias;     // fwd
  const float* z;        // bwd: forward output of this layer [M][Kg]
  const int* cls;        // bwd seed: class per row (nullable -> not seed)
  const float* x;        // bwd: forward input of this layer [M][N]
  const float* den;      // bwd POST_DIV: next (lower) layer denominator, same indexing as out
  float* out;            // fwd: z [M][N]; bwd: R_in or g_next [M][N]
  float* out_relu;       // fwd: relu(z) (nullable)
  int M, N, K;           // GEMM dims
  int bwd;
  int one_hot, relu_mask, rule_eps, xmode, post;
  float eps, eps_post;
};

__global__ __launch_bounds__(256) void linear_kernel(LinArgs a) {
  __shared__ float As[LT][LK + 1];
  __shared__ float Bs[LK][LT + 1];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int m0 = blockIdx.x * LT, n0 = blockIdx.y * LT;
  const int wm = (w & 1) * 16, wn = (w >> 1) * 16;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.K; k0 += LK) {
    __syncthreads();
    for (int idx = tid; idx < LT * LK; idx += 256) {
      const int r = idx / LK, c = idx % LK;
      const int m = m0 + r, k = k0 + c;
      float v = 0.f;
      if (m < a.M && k < a.K) {
        if (!a.bwd) {
          v = a.A[(size_t)m * a.K + k];
        } else {
          // g = [z > 0]? R / stab(z) (rule Epsilon) or R (plain); R = seed or incoming relevance
          const float zz = a.z[(size_t)m * a.K + k];
          float R;
          if (a.cls) {
            const bool hit = (k == a.cls[m]);
            R = hit ? (a.one_hot ? 1.f : zz) : 0.f;
          } else {
            R = a.A[(size_t)m * a.K + k];
          }
          if (a.relu_mask && !(zz > 0.f)) R = 0.f;
          v = a.rule_eps ? R / stab(zz, a.eps) : R;
        }
      }
      As[r][c] = v;
    }
    for (int idx = tid; idx < LK * LT; idx += 256) {
      const int r = idx / LT, c = idx % LT;
      const int k = k0 + r, n = n0 + c;
      float v = 0.f;
      if (k < a.K && n < a.N) v = a.bwd ? a.W[(size_t)k * a.N + n] : a.W[(size_t)n * a.K + k];
      Bs[r][c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < LK; kk += 4) {
      const float av = As[wm + (lane & 15)][kk + (lane >> 4)];
      const float bv = Bs[kk + (lane >> 4)][wn + (lane & 15)];
      acc = mfma16(av, bv, acc);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + wm + (lane >> 4) * 4 + r, n = n0 + wn + (lane & 15);
    if (m >= a.M || n >= a.N) continue;
    const size_t o = (size_t)m * a.N + n;
    if (!a.bwd) {
      const float zz = acc[r] + (a.bias ? a.bias[n] : 0.f);
      a.out[o] = zz;
      if (a.out_relu) a.out_relu[o] = zz > 0.f ? zz : (zz != zz ? zz : 0.f);
    } else {
      float R = acc[r];
      if (a.xmode == XM_MUL) R = a.x[o] * R;
      if (a.post == POST_DIV) {
        const float xv = a.x[o];
        const float q = div_nb(R, stab(a.den[o], a.eps_post));
        R = (xv > 0.f) ? q : 0.f;
      } else if (a.post == POST_MASK) {
        R = (a.x[o] > 0.f) ? R : 0.f;
      }
      a.out[o] = R;
    }
  }
}

// Long K (the classifier input, K = 2048) with few output tiles (GTZAN: 512 x 128 = 256 16 x 16
// tiles): one wave per 16 x 16 output tile, so the grid covers the chip instead of 64 four-wave
// workgroups; K in 128-wide chunks staged through the wave's own LDS (a wave barrier, no workgroup
// barrier), the next chunk's 16 float4 loads in flight under the current chunk's 32 MFMAs.  The
// same single k-ordered chain per output as linear_kernel (bias added last): the same bits.
// x and W are read as float4: K % 4 == 0 and both 16-byte aligned (drsa_amd_linear_fwd checks).
constexpr int L1K = 128;

__global__ __launch_bounds__(64) void linear_fwd_w1_kernel(LinArgs a) {
  __shared__ __attribute__((aligned(16))) float As[16][L1K + 4];   // [m][k]
  __shared__ float Bs[L1K][16 + 1];                                 // [k][n]
  const int lane = threadIdx.x;
  const int m0 = blockIdx.x * 16, n0 = blockIdx.y * 16;
  constexpr int NV = 16 * L1K / 4 / 64;   // float4 per lane per operand (8)
  float4 ra[NV], rb[NV];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = lane + i * 64, r = idx / (L1K / 4), k = k0 + (idx % (L1K / 4)) * 4;
      const int m = m0 + r, n = n0 + r;
      const bool oa = m < a.M && k < a.K, ob = n < a.N && k < a.K;
      const float4 va = *reinterpret_cast<const float4*>(a.A + (oa ? (size_t)m * a.K + k : 0));
      const float4 vb = *reinterpret_cast<const float4*>(a.W + (ob ? (size_t)n * a.K + k : 0));
      ra[i] = oa ? va : make_float4(0.f, 0.f, 0.f, 0.f);
      rb[i] = ob ? vb : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  load(0);
  for (int k0 = 0; k0 < a.K; k0 += L1K) {
    __builtin_amdgcn_wave_barrier();   // the previous chunk's LDS reads done (one wave: in order)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = lane + i * 64, r = idx / (L1K / 4), c = (idx % (L1K / 4)) * 4;
      *reinterpret_cast<float4*>(&As[r][c]) = ra[i];
      Bs[c][r] = rb[i].x; Bs[c + 1][r] = rb[i].y; Bs[c + 2][r] = rb[i].z; Bs[c + 3][r] = rb[i].w;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the stores landed before this wave reads them
    __builtin_amdgcn_wave_barrier();
    if (k0 + L1K < a.K) load(k0 + L1K);
    // every operand of the chunk read before its chain (left to the scheduler each MFMA waits on
    // its own LDS round trip: one wave per SIMD has nothing else to hide it behind)
    float av[L1K / 4], bv[L1K / 4];
#pragma unroll
    for (int q = 0; q < L1K / 4; ++q) {
      av[q] = As[lane & 15][4 * q + (lane >> 4)];
      bv[q] = Bs[4 * q + (lane >> 4)][lane & 15];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < L1K / 4; ++q) acc = mfma16(av[q], bv[q], acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + (lane >> 4) * 4 + r, n = n0 + (lane & 15);
    if (m >= a.M || n >= a.N) continue;
    const size_t o = (size_t)m * a.N + n;
    const float zz = acc[r] + (a.bias ? a.bias[n] : 0.f);
    a.out[o] = zz;
    if (a.out_relu) a.out_relu[o] = zz > 0.f ? zz : (zz != zz ? zz : 0.f);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int drsa_amd_linear_fwd(const float* x, const float* Wt, const float* bias, float* z_out, float* relu_out, int M,
                        int N, int K, void* stream) {
  DRSA_REQUIRE(M > 0 && N > 0 && K > 0, "linear_fwd: bad shape");
  DRSA_REQUIRE(x && Wt && z_out, "linear_fwd: x, W and z_out are required");
  LinArgs a{};
  a.A = x; a.W = Wt; a.bias = bias; a.out = z_out; a.out_relu = relu_out; a.M = M; a.N = N; a.K = K; a.bwd = 0;
  // long K with float4-aligned rows (K % 4 == 0, x and W on the 16-byte grid): the prefetching kernel;
  // anything else takes the scalar loads of linear_kernel.  Same chain order, same results
  if (K % 4 == 0 && K >= L1K && aligned16(x) && aligned16(Wt))
    hipLaunchKernelGGL(linear_fwd_w1_kernel, dim3((M + 15) / 16, (N + 15) / 16), dim3(64), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(linear_kernel, dim3((M + LT - 1) / LT, (N + LT - 1) / LT), dim3(256), 0, (hipStream_t)stream, a);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

// out[M][Kin] = epi( g[M][Nout] W[Nout][Kin] ),  g = prologue(R or seed, z)
int drsa_amd_linear_bwd(const float* R, const int* seed_cls, int one_hot, const float* z, int relu_mask, int rule_eps,
                        float eps, const float* Wt, const float* x, int xmode, const float* den, int post,
                        float eps_post, float* out, int M, int Nout, int Kin, void* stream) {
  DRSA_REQUIRE(M > 0 && Nout > 0 && Kin > 0, "linear_bwd: bad shape");
  DRSA_REQUIRE(R || seed_cls, "linear_bwd: need R or a seed");
  DRSA_REQUIRE(z && Wt && out, "linear_bwd: z, W and out are required");
  DRSA_REQUIRE(xmode == XM_NONE || xmode == XM_MUL, "linear_bwd: xmode must be XM_NONE or XM_MUL");
  DRSA_REQUIRE(post == POST_NONE || post == POST_DIV || post == POST_MASK,
               "linear_bwd: post must be POST_NONE, POST_DIV or POST_MASK");
  DRSA_REQUIRE(xmode == XM_NONE || x, "linear_bwd: xmode needs x");
  DRSA_REQUIRE(post == POST_NONE || (x && (den || post == POST_MASK)), "linear_bwd: POST_DIV needs x and den");
  LinArgs a{};
  a.A = R; a.cls = seed_cls; a.one_hot = one_hot; a.z = z; a.relu_mask = relu_mask; a.rule_eps = rule_eps;
  a.eps = eps; a.W = Wt; a.x = x; a.xmode = xmode; a.den = den; a.post = post; a.eps_post = eps_post; a.out = out;
  a.M = M; a.N = Kin; a.K = Nout; a.bwd = 1;
  hipLaunchKernelGGL(linear_kernel, dim3((M + LT - 1) / LT, (Kin + LT - 1) / LT), dim3(256), 0, (hipStream_t)stream, a);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

}  // extern "C"
