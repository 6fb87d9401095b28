// LRP dense head under Gamma / ZPlus / WSquare / Flat (reference pf.py:18-27, 257-292: the dense
// rule comes from the same rule_mapper as the conv rule; semantics oracle/lrp_ref.py
// rule_backward_analytic).  The Epsilon head stays on linear.hip; these are the same fp32 MFMA
// 16x16x4 tiles with several k-ordered chains per output that share one staged x (forward) or one
// staged g (backward).
//
// Forward chains (each its own accumulator, its bias added to it last):
//   c0 (x , W , b )  z, bit-identical to drsa_amd_linear_fwd
//   c1 (x+, Wp, bp)  \ den_p = c1 + c2
//   c2 (x-, Wn, 0 )  /            (SIGNED: the input may be negative)
//   c3 (x+, Wn, bn)  \ den_n = c3 + c4   (NEGDEN: no ReLU after the layer, so [z < 0] can hold)
//   c4 (x-, Wp, 0 )  /            (SIGNED and NEGDEN)
// Gamma: Wp/Wn = W + gamma W+-, ZPlus: Wp/Wn = W+-, bp = b+ (never NEGDEN).  The weight sets are
// plan constants (engine/plan.py dense_rule_params), not rebuilt here.
// Backward chains: t0 (g_p, Wp), t1 (g_p, Wn) [SIGNED], t2 (g_n, Wn) [NEGDEN], t3 (g_n, Wp) [both];
//   R_in = x+ t0 + x- t1 + x+ t2 + x- t3, left to right; WSquare / Flat: one chain over W2, no x.
#include "common.h"
#include "lrp_conv.h"

namespace {

constexpr int LT = 32;   // workgroup tile (M and N)
constexpr int LK = 32;   // K chunk

// torch clamp(min=0) / clamp(max=0): NaN stays NaN
__device__ __forceinline__ float pos_part(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float neg_part(float v) { return v > 0.f ? 0.f : v; }

struct RuleFwdArgs {
  const float* x;                 // [M][K]
  const float *W, *Wp, *Wn;       // [N][K] each (Wn only when SIGNED or NEGDEN)
  const float *b, *bp, *bn;       // [N], nullable (a layer without bias)
  float *z, *relu, *den_p, *den_n;
  int M, N, K;
};

template <bool SIGNED, bool NEGDEN>
__device__ __forceinline__ void rule_fwd_store(const RuleFwdArgs& a, int m, int n, float c0, float c1, float c2,
                                               float c3, float c4) {
  const size_t o = (size_t)m * a.N + n;
  const float zz = c0 + (a.b ? a.b[n] : 0.f);
  a.z[o] = zz;
  if (a.relu) a.relu[o] = zz > 0.f ? zz : (zz != zz ? zz : 0.f);
  const float z0 = c1 + (a.bp ? a.bp[n] : 0.f);
  const float z1 = SIGNED ? c2 + 0.f : 0.f;
  a.den_p[o] = z0 + z1;
  if (NEGDEN) {
    const float z2 = c3 + (a.bn ? a.bn[n] : 0.f);
    const float z3 = SIGNED ? c4 + 0.f : 0.f;
    a.den_n[o] = z2 + z3;
  }
}

// Short K (or K % 4 != 0): the 32 x 32 tile of linear_kernel, x staged once per chunk, the clamps
// taken as the operand leaves the staged tile.
template <bool SIGNED, bool NEGDEN>
__global__ __launch_bounds__(256) void rule_fwd_kernel(RuleFwdArgs a) {
  constexpr bool WN = SIGNED || NEGDEN;
  __shared__ float As[LT][LK + 1];
  __shared__ float Bs[WN ? 3 : 2][LK][LT + 1];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int m0 = blockIdx.x * LT, n0 = blockIdx.y * LT;
  const int wm = (w & 1) * 16, wn = (w >> 1) * 16;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0, acc4 = acc0;
  for (int k0 = 0; k0 < a.K; k0 += LK) {
    __syncthreads();
    for (int idx = tid; idx < LT * LK; idx += 256) {
      const int r = idx / LK, c = idx % LK;
      const int m = m0 + r, k = k0 + c;
      As[r][c] = (m < a.M && k < a.K) ? a.x[(size_t)m * a.K + k] : 0.f;
    }
    for (int idx = tid; idx < LK * LT; idx += 256) {
      const int r = idx / LT, c = idx % LT;
      const int k = k0 + r, n = n0 + c;
      const bool in = k < a.K && n < a.N;
      const size_t o = in ? (size_t)n * a.K + k : 0;
      Bs[0][r][c] = in ? a.W[o] : 0.f;
      Bs[1][r][c] = in ? a.Wp[o] : 0.f;
      if (WN) Bs[2][r][c] = in ? a.Wn[o] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < LK; kk += 4) {
      const float av = As[wm + (lane & 15)][kk + (lane >> 4)];
      const float xp = SIGNED ? pos_part(av) : av, xn = neg_part(av);
      const int br = kk + (lane >> 4), bc = wn + (lane & 15);
      const float b0 = Bs[0][br][bc], bp = Bs[1][br][bc];
      acc0 = mfma16(av, b0, acc0);
      acc1 = mfma16(xp, bp, acc1);
      if (SIGNED && NEGDEN) acc4 = mfma16(xn, bp, acc4);
      if (WN) {
        const float bn = Bs[2][br][bc];
        if (SIGNED) acc2 = mfma16(xn, bn, acc2);
        if (NEGDEN) acc3 = mfma16(xp, bn, acc3);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + wm + (lane >> 4) * 4 + r, n = n0 + wn + (lane & 15);
    if (m >= a.M || n >= a.N) continue;
    rule_fwd_store<SIGNED, NEGDEN>(a, m, n, acc0[r], acc1[r], acc2[r], acc3[r], acc4[r]);
  }
}

// Long K (the classifier input, K = 2048): linear_fwd_w1_kernel's structure, one wave per 16 x 16
// output tile, 128-wide K chunks through the wave's own LDS, the next chunk's loads in flight under
// the current chunk's MFMAs.  x is staged once per chunk and its 32 operands read once; every
// weight set's operands are read in turn and feed the (up to two) chains that use that set, which
// are independent of each other, so the MFMA pipe alternates between them.
constexpr int L1K = 128;

template <bool SIGNED, bool NEGDEN>
__global__ __launch_bounds__(64) void rule_fwd_w1_kernel(RuleFwdArgs a) {
  constexpr bool WN = SIGNED || NEGDEN;
  constexpr int NS = WN ? 3 : 2;
  __shared__ __attribute__((aligned(16))) float As[16][L1K + 4];   // [m][k]
  __shared__ float Bs[NS][L1K][16 + 1];                             // [set][k][n]
  const int lane = threadIdx.x;
  const int m0 = blockIdx.x * 16, n0 = blockIdx.y * 16;
  constexpr int NV = 16 * L1K / 4 / 64;   // float4 per lane per operand (8)
  float4 ra[NV], rb[NS][NV];
  const float* const ws[3] = {a.W, a.Wp, a.Wn};
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = lane + i * 64, r = idx / (L1K / 4), k = k0 + (idx % (L1K / 4)) * 4;
      const int m = m0 + r, n = n0 + r;
      const bool oa = m < a.M && k < a.K, ob = n < a.N && k < a.K;
      const float4 va = *reinterpret_cast<const float4*>(a.x + (oa ? (size_t)m * a.K + k : 0));
      ra[i] = oa ? va : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const float4 vb = *reinterpret_cast<const float4*>(ws[s] + (ob ? (size_t)n * a.K + k : 0));
        rb[s][i] = ob ? vb : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0, acc4 = acc0;
  load(0);
  for (int k0 = 0; k0 < a.K; k0 += L1K) {
    __builtin_amdgcn_wave_barrier();   // the previous chunk's LDS reads done (one wave: in order)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = lane + i * 64, r = idx / (L1K / 4), c = (idx % (L1K / 4)) * 4;
      *reinterpret_cast<float4*>(&As[r][c]) = ra[i];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        Bs[s][c][r] = rb[s][i].x; Bs[s][c + 1][r] = rb[s][i].y; Bs[s][c + 2][r] = rb[s][i].z;
        Bs[s][c + 3][r] = rb[s][i].w;
      }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the stores landed before this wave reads them
    __builtin_amdgcn_wave_barrier();
    if (k0 + L1K < a.K) load(k0 + L1K);
    float av[L1K / 4], bv[L1K / 4];
#pragma unroll
    for (int q = 0; q < L1K / 4; ++q) {
      av[q] = As[lane & 15][4 * q + (lane >> 4)];
      bv[q] = Bs[0][4 * q + (lane >> 4)][lane & 15];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < L1K / 4; ++q) acc0 = mfma16(av[q], bv[q], acc0);
#pragma unroll
    for (int q = 0; q < L1K / 4; ++q) bv[q] = Bs[1][4 * q + (lane >> 4)][lane & 15];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < L1K / 4; ++q) {
      acc1 = mfma16(SIGNED ? pos_part(av[q]) : av[q], bv[q], acc1);
      if (SIGNED && NEGDEN) acc4 = mfma16(neg_part(av[q]), bv[q], acc4);
    }
    if (WN) {
#pragma unroll
      for (int q = 0; q < L1K / 4; ++q) bv[q] = Bs[NS - 1][4 * q + (lane >> 4)][lane & 15];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < L1K / 4; ++q) {
        if (SIGNED) acc2 = mfma16(neg_part(av[q]), bv[q], acc2);
        if (NEGDEN) acc3 = mfma16(SIGNED ? pos_part(av[q]) : av[q], bv[q], acc3);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + (lane >> 4) * 4 + r, n = n0 + (lane & 15);
    if (m >= a.M || n >= a.N) continue;
    rule_fwd_store<SIGNED, NEGDEN>(a, m, n, acc0[r], acc1[r], acc2[r], acc3[r], acc4[r]);
  }
}

struct RuleBwdArgs {
  const float* R;          // [M][K] incoming relevance (ignored when cls)
  const int* cls;          // seed: class per row (nullable -> not seed)
  const float* z;          // [M][K] plain forward output of this layer
  const float *den_p, *den_n;   // [M][K], or [K] when den_bcast (WSquare / Flat plan constant)
  const float *Wp, *Wn;    // [K][N] (torch Linear weight layout [Nout][Kin])
  const float* x;          // [M][N] forward input of this layer
  const float* den;        // POST_DIV: last conv stage's denominator, indexed as out
  float* out;              // [M][N]
  int M, N, K;             // GEMM dims: N = Kin, K = Nout
  int one_hot, relu_mask, zsign, den_bcast, xmul, post;
  float eps, eps_post;
};

template <bool SIGNED, bool NEGDEN>
__global__ __launch_bounds__(256) void rule_bwd_kernel(RuleBwdArgs a) {
  constexpr bool WN = SIGNED || NEGDEN;
  __shared__ float As[NEGDEN ? 2 : 1][LT][LK + 1];
  __shared__ float Bs[WN ? 2 : 1][LK][LT + 1];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int m0 = blockIdx.x * LT, n0 = blockIdx.y * LT;
  const int wm = (w & 1) * 16, wn = (w >> 1) * 16;
  f32x4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = t0, t2 = t0, t3 = t0;
  for (int k0 = 0; k0 < a.K; k0 += LK) {
    __syncthreads();
    for (int idx = tid; idx < LT * LK; idx += 256) {
      const int r = idx / LK, c = idx % LK;
      const int m = m0 + r, k = k0 + c;
      float gp = 0.f, gn = 0.f;
      if (m < a.M && k < a.K) {
        // g_p = R [z > 0] / stab(den_p), g_n = R [z < 0] / stab(den_n)  (Gamma; ZPlus / WSquare / Flat:
        // g = R / stab(den));  R = seed or incoming relevance, through the ReLU mask
        const size_t o = (size_t)m * a.K + k;
        const float zz = a.z[o];
        float R;
        if (a.cls) {
          const bool hit = (k == a.cls[m]);
          R = hit ? (a.one_hot ? 1.f : zz) : 0.f;
        } else {
          R = a.R[o];
        }
        if (a.relu_mask && !(zz > 0.f)) R = 0.f;
        const size_t od = a.den_bcast ? (size_t)k : o;
        gp = ((a.zsign && !(zz > 0.f)) ? 0.f : R) / stab(a.den_p[od], a.eps);
        if (NEGDEN) gn = ((zz < 0.f) ? R : 0.f) / stab(a.den_n[od], a.eps);
      }
      As[0][r][c] = gp;
      if (NEGDEN) As[1][r][c] = gn;
    }
    for (int idx = tid; idx < LK * LT; idx += 256) {
      const int r = idx / LT, c = idx % LT;
      const int k = k0 + r, n = n0 + c;
      const bool in = k < a.K && n < a.N;
      const size_t o = in ? (size_t)k * a.N + n : 0;
      Bs[0][r][c] = in ? a.Wp[o] : 0.f;
      if (WN) Bs[1][r][c] = in ? a.Wn[o] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < LK; kk += 4) {
      const int ar = wm + (lane & 15), ac = kk + (lane >> 4);
      const int br = kk + (lane >> 4), bc = wn + (lane & 15);
      const float gp = As[0][ar][ac], bp = Bs[0][br][bc];
      t0 = mfma16(gp, bp, t0);
      if (WN) {
        const float bn = Bs[1][br][bc];
        if (SIGNED) t1 = mfma16(gp, bn, t1);
        if (NEGDEN) {
          const float gn = As[1][ar][ac];
          t2 = mfma16(gn, bn, t2);
          if (SIGNED) t3 = mfma16(gn, bp, t3);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + wm + (lane >> 4) * 4 + r, n = n0 + wn + (lane & 15);
    if (m >= a.M || n >= a.N) continue;
    const size_t o = (size_t)m * a.N + n;
    float R = t0[r];
    if (a.xmul) {
      const float xv = a.x[o];
      const float xp = SIGNED ? pos_part(xv) : xv, xn = neg_part(xv);
      R = xp * t0[r];
      if (SIGNED) R = R + xn * t1[r];
      if (NEGDEN) R = R + xp * t2[r];
      if (SIGNED && NEGDEN) R = R + xn * t3[r];
    }
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

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The long-K kernel reads x and every weight set it is given as float4: K % 4 == 0 and all of them on the
// 16-byte grid (a null Wn is); anything else takes rule_fwd_kernel's scalar loads (the same chains, the
// same bits).
template <bool SIGNED, bool NEGDEN>
void launch_fwd(const RuleFwdArgs& a, hipStream_t s) {
  const bool vec = aligned16(a.x) && aligned16(a.W) && aligned16(a.Wp) && aligned16(a.Wn);
  if (a.K % 4 == 0 && a.K >= L1K && vec)
    hipLaunchKernelGGL((rule_fwd_w1_kernel<SIGNED, NEGDEN>), dim3((a.M + 15) / 16, (a.N + 15) / 16), dim3(64), 0, s, a);
  else
    hipLaunchKernelGGL((rule_fwd_kernel<SIGNED, NEGDEN>), dim3((a.M + LT - 1) / LT, (a.N + LT - 1) / LT), dim3(256), 0,
                       s, a);
}

template <bool SIGNED, bool NEGDEN>
void launch_bwd(const RuleBwdArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((rule_bwd_kernel<SIGNED, NEGDEN>), dim3((a.M + LT - 1) / LT, (a.N + LT - 1) / LT), dim3(256), 0, s,
                     a);
}

}  // namespace

extern "C" {

int drsa_amd_linear_rule_fwd(const float* x, const float* W, const float* Wp, const float* Wn, const float* bias,
                             const float* bias_p, const float* bias_n, float* z_out, float* relu_out, float* den_p,
                             float* den_n, int x_signed, int M, int N, int K, void* stream) {
  DRSA_REQUIRE(M > 0 && N > 0 && K > 0, "linear_rule_fwd: bad shape");
  DRSA_REQUIRE(x && W && Wp && z_out && den_p, "linear_rule_fwd: x, W, Wp, z_out and den_p are required");
  DRSA_REQUIRE(Wn || (!x_signed && !den_n), "linear_rule_fwd: a signed input or den_n needs Wn");
  RuleFwdArgs a{};
  a.x = x; a.W = W; a.Wp = Wp; a.Wn = Wn; a.b = bias; a.bp = bias_p; a.bn = bias_n; a.z = z_out; a.relu = relu_out;
  a.den_p = den_p; a.den_n = den_n; a.M = M; a.N = N; a.K = K;
  hipStream_t s = (hipStream_t)stream;
  if (x_signed && den_n) launch_fwd<true, true>(a, s);
  else if (x_signed) launch_fwd<true, false>(a, s);
  else if (den_n) launch_fwd<false, true>(a, s);
  else launch_fwd<false, false>(a, s);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

int drsa_amd_linear_rule_bwd(const float* R, const int* seed_cls, int one_hot, const float* z, int relu_mask,
                             const float* den_p, const float* den_n, int den_bcast, int zsign, float eps,
                             const float* Wp, const float* Wn, const float* x, int xmul, int x_signed,
                             const float* den, int post, float eps_post, float* out, int M, int Nout, int Kin,
                             void* stream) {
  DRSA_REQUIRE(M > 0 && Nout > 0 && Kin > 0, "linear_rule_bwd: bad shape");
  DRSA_REQUIRE(R || seed_cls, "linear_rule_bwd: need R or a seed");
  DRSA_REQUIRE(z && den_p && Wp && out, "linear_rule_bwd: z, den_p, Wp and out are required");
  DRSA_REQUIRE(Wn || (!x_signed && !den_n), "linear_rule_bwd: a signed input or den_n needs Wn");
  DRSA_REQUIRE(!den_n || (zsign && !den_bcast), "linear_rule_bwd: den_n goes with the output-sign split only");
  DRSA_REQUIRE(xmul || (!x_signed && !den_n), "linear_rule_bwd: the x+ / x- terms need xmul");
  DRSA_REQUIRE(!xmul || x, "linear_rule_bwd: xmul needs x");
  DRSA_REQUIRE(post == POST_NONE || (post == POST_DIV && x && den) || (post == POST_MASK && x),
               "linear_rule_bwd: post must be POST_NONE, POST_DIV (x and den) or POST_MASK (x)");
  RuleBwdArgs a{};
  a.R = R; a.cls = seed_cls; a.one_hot = one_hot; a.z = z; a.relu_mask = relu_mask; a.den_p = den_p; a.den_n = den_n;
  a.den_bcast = den_bcast; a.zsign = zsign; a.eps = eps; a.Wp = Wp; a.Wn = Wn; a.x = x; a.xmul = xmul; a.den = den;
  a.post = post; a.eps_post = eps_post; a.out = out; a.M = M; a.N = Kin; a.K = Nout;
  hipStream_t s = (hipStream_t)stream;
  if (x_signed && den_n) launch_bwd<true, true>(a, s);
  else if (x_signed) launch_bwd<true, false>(a, s);
  else if (den_n) launch_bwd<false, true>(a, s);
  else launch_bwd<false, false>(a, s);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

}  // extern "C"
