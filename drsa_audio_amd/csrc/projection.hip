// LRP through the ProjectionModel virtual layers (reference modify_model.py:75-123) with the
// composite of explainer.py:198-203: Epsilon on invprojection, SubspaceHook mask, Epsilon on
// projection; SubspaceHook.backward = attribute.py:53-60.
#include "common.h"

#include <type_traits>

namespace {

// ===========================================================================
// projection forward: h = a_vec U, a' = h U^T, optional 2x2 max-pool of a'
//   a [B][d][H][W] -> h [B][d][H*W] (channel-major), ap [B][d][H][W], pooled + argmax
//   tile = 2 rows x 32 cols (64 pixels); a workgroup stages U once and walks PT tiles.
//   MFMA orientation D[channel][pixel]: lanes = pixels (coalesced I/O).
// Any d <= DP (DP = 16, 32, 64, 128): U and a are embedded in DP x DP / DP rows with zeros;
// the k chains run over d4 = round_up(d, 4) terms only, so for d % 4 == 0 (VGGish d = 100, 96)
// every value is the d-term chain of the unpadded product, bit for bit; outputs past d are
// computed (zeros) but not stored.
// ===========================================================================
// P = U U^T - I (d x d), the projection residual: each entry one float64 fma chain over k
// ascending (the products of two floats are exact in float64), minus the identity, rounded
// once to fp32.  P is symmetric bit for bit.  The projection kernels evaluate
//   a' = h U^T  as  a' = a + a P
// (equal in exact arithmetic): at a dead ReLU channel (a = 0) a' is then exact to its own
// rounding instead of carrying the O(1e-8) rounding noise of the d-term chain h U^T, which the
// invprojection's Epsilon(1e-6) amplifies into the subspace relevances.
__global__ __launch_bounds__(256) void projection_residual_kernel(const float* __restrict__ U, int d,
                                                                  float* __restrict__ P) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d * d) return;
  const int r = i / d, c = i % d;
  double acc = 0.0;
  for (int k = 0; k < d; ++k) acc = fma((double)U[r * d + k], (double)U[c * d + k], acc);
  P[i] = (float)(acc - (r == c ? 1.0 : 0.0));
}

// MFMA A operand P[c][k] of lane (c, k), read as the symmetric P[k][c] so that the 16 lanes of a
// row group load 16 consecutive floats; zero outside the d x d matrix (padded embedding).
// P is never staged in LDS: the forward holds its operands in registers (unpadded DP <= 64;
// 0.139 ms at B = 512, d = 64, vs 0.161 with P in LDS, which costs a workgroup per CU) and the
// backward reads them through L1 (0.524 vs 0.537 ms from LDS; registers would cost it a wave per
// SIMD).
__device__ __forceinline__ float p_operand(const float* __restrict__ P, int d, int c, int k) {
  const bool ok = c < d && k < d;
  const float v = P[ok ? k * d + c : 0];
  return ok ? v : 0.f;
}

constexpr int PT = 4;   // row-pair tiles per workgroup (forward)

template <int DP>
__device__ __forceinline__ void stage_u_padded(float* Us, const float* __restrict__ U, int d, int tid) {
  constexpr int LD = DP + 1;
  for (int i = tid; i < DP * DP; i += 256) {
    const int c = i / DP, j = i % DP;
    const bool ok = c < d && j < d;
    const float v = U[ok ? c * d + j : 0];
    Us[c * LD + j] = ok ? v : 0.f;
  }
}

// Multi-matrix entries (drsa_amd_projection_*_multi): sample b runs on matrix u_row[b] of a table
// [n_u][d][d].  The index is uniform in a workgroup (blockIdx.y is the sample): it is read once, as a
// scalar, clamped into the table, and moves the workgroup's matrix base; everything after it is the
// single-matrix kernel.  MULTI is a template parameter so that the single-matrix instantiations keep
// their code and registers (projection_bwd_rc_kernel at d = DP = 64 has 6 VGPRs to spare).
__device__ __forceinline__ size_t table_offset(const int* __restrict__ u_row, int n_u, int b, int d) {
  int u = __builtin_amdgcn_readfirstlane(u_row[b]);
  u = u < 0 ? 0 : u >= n_u ? n_u - 1 : u;
  return (size_t)u * d * d;
}

// HOUT = false (the plan's default: projection_bwd recomputes h): only the residual GEMM
// delta = a P runs and U is not staged -- h = a U is needed by nobody (a' = a + delta).
template <int DP, bool PAD, bool HOUT, bool MULTI>
__global__ __launch_bounds__(256) void projection_fwd_kernel(const float* __restrict__ a, const float* __restrict__ U,
                                                            const float* __restrict__ Pm,
                                                            float* __restrict__ h, float* __restrict__ ap,
                                                            float* __restrict__ pooled, uint8_t* __restrict__ amax,
                                                            int d_in, int H, int W, int pool,
                                                            const int* __restrict__ u_row, int n_u) {
  const int d = PAD ? d_in : DP;   // PAD = false: d == DP at compile time (no padding code)
  if constexpr (MULTI) {
    const size_t uo = table_offset(u_row, n_u, blockIdx.y, d);
    U += uo;
    Pm += uo;
  }
  constexpr int P = 64, LD = DP + 1, PL = P + 4;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Us = sm;               // [DP][LD]   U[c][j] (HOUT only)
  float* as = Us + (HOUT ? DP * LD : 0);   // [DP][PL]   a tile, then a' tile
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int b = blockIdx.y;
  const int TW = W < 32 ? W : 32, RPT = P / TW;      // tile = RPT rows x TW cols
  const int HW = H * W, xt = W / TW;
  const int d4 = (d + 3) & ~3;
  // per-sample bases + 32-bit per-lane offsets (saddr + voffset addressing; d * H * W < 2^31)
  const float* __restrict__ a_b = a + (size_t)b * d * HW;
  float* __restrict__ h_b = HOUT ? h + (size_t)b * d * HW : nullptr;
  float* __restrict__ ap_b = ap ? ap + (size_t)b * d * HW : nullptr;
  if constexpr (HOUT) stage_u_padded<DP>(Us, U, d, tid);
  constexpr int NB = DP / 16;
  // unpadded DP <= 64: the residual's MFMA A operands (P[c][k], read as the symmetric P[k][c]) live
  // in registers for the whole launch: NB * DP / 4 floats per lane
  constexpr bool PREG = !PAD && DP <= 64;
  float preg[PREG ? NB * (DP / 4) : 1];
  if constexpr (PREG) {
#pragma unroll
    for (int jb = 0; jb < NB; ++jb)
#pragma unroll
      for (int ks = 0; ks < DP / 4; ++ks) preg[jb * (DP / 4) + ks] = Pm[(ks * 4 + (lane >> 4)) * DP + jb * 16 + (lane & 15)];
  }
  static_assert(P / 16 == 4, "one 16-pixel block per wave");
  // the a tile goes HBM -> registers one tile ahead (issued before the current tile's GEMMs),
  // then registers -> LDS at the top of its own iteration
  // (DP <= 64; at DP = 128 the 32 registers would cost a wave per SIMD)
  constexpr bool PFT = DP <= 64;
  constexpr int NPF = PFT ? DP * P / 256 : 1;
  const int ntiles = (H / RPT) * xt;
  float pf[NPF];
  auto fetch_tile = [&](int tile) {
    const int y0 = (tile / xt) * RPT, x0 = (tile % xt) * TW;
#pragma unroll
    for (int u = 0; u < (PFT ? NPF : 0); ++u) {
      const int i = tid + 256 * u, c = i / P, p = i % P;
      const bool ok = c < d;
      const float v = a_b[(ok ? c : 0) * HW + (y0 + p / TW) * W + x0 + p % TW];
      pf[u] = ok ? v : 0.f;
    }
  };
  if constexpr (PFT)
    if (blockIdx.x * PT < ntiles) fetch_tile(blockIdx.x * PT);
  for (int t = 0; t < PT; ++t) {
    const int tile = blockIdx.x * PT + t;
    if (tile >= ntiles) break;
    const int y0 = (tile / xt) * RPT, x0 = (tile % xt) * TW;
    __syncthreads();
    if constexpr (PFT) {
#pragma unroll
      for (int u = 0; u < NPF; ++u) {
        const int i = tid + 256 * u;
        as[(i / P) * PL + i % P] = pf[u];
      }
    } else {
      for (int i = tid; i < DP * P; i += 256) {
        const int c = i / P, p = i % P;
        const bool ok = c < d;
        const float v = a_b[(ok ? c : 0) * HW + (y0 + p / TW) * W + x0 + p % TW];
        as[c * PL + p] = ok ? v : 0.f;
      }
    }
    __syncthreads();
    if constexpr (PFT)
      if (t + 1 < PT && tile + 1 < ntiles) fetch_tile(tile + 1);
    // h[j][p] = sum_c U[c][j] a[c][p] and delta[c][p] = sum_k P[c][k] a[k][p]: wave w owns pixel
    // block w and runs the 2 NB output blocks as independent MFMA chains sharing the B operand read
    // (per element the single-chain k order); then a' = a + delta (= h U^T, residual form above)
    {
      f32x4 acc[NB], dl[NB];
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) acc[jb] = dl[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (PREG) {
#pragma unroll
        for (int k0 = 0; k0 < DP; k0 += 4) {
          const int c = k0 + (lane >> 4);
          const float bv = as[c * PL + w * 16 + (lane & 15)];
#pragma unroll
          for (int jb = 0; jb < NB; ++jb) {
            if constexpr (HOUT) acc[jb] = mfma16(Us[c * LD + jb * 16 + (lane & 15)], bv, acc[jb]);
            dl[jb] = mfma16(preg[jb * (DP / 4) + k0 / 4], bv, dl[jb]);
          }
        }
      } else {
#pragma unroll 2
        for (int k0 = 0; k0 < d4; k0 += 4) {
          const int c = k0 + (lane >> 4);
          const float bv = as[c * PL + w * 16 + (lane & 15)];
#pragma unroll
          for (int jb = 0; jb < NB; ++jb) {
            if constexpr (HOUT) acc[jb] = mfma16(Us[c * LD + jb * 16 + (lane & 15)], bv, acc[jb]);
            dl[jb] = mfma16(p_operand(Pm, d, jb * 16 + (lane & 15), c), bv, dl[jb]);
          }
        }
      }
      // every wave reads and writes only its own 16 pixel columns of the tile
#pragma unroll
      for (int jb = 0; jb < NB; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = jb * 16 + (lane >> 4) * 4 + r, p = w * 16 + (lane & 15);
          const int og = j * HW + (y0 + p / TW) * W + x0 + p % TW;
          if (HOUT && j < d) h_b[og] = acc[jb][r];
          const float v = as[j * PL + p] + dl[jb][r];
          as[j * PL + p] = v;   // a tile no longer needed: holds a' now
          if (ap_b && j < d) ap_b[og] = v;
        }
    }
    if (pool) {
      __syncthreads();
      const int H2 = H / 2, W2 = W / 2;
      const int CXN = TW / 2;
      for (int i = tid; i < d * 16; i += 256) {
        const int c = i / 16, cell = i % 16, cy = cell / CXN, cx = cell % CXN;
        const int p00 = (2 * cy) * TW + 2 * cx;
        const float v[4] = {as[c * PL + p00], as[c * PL + p00 + 1], as[c * PL + p00 + TW],
                            as[c * PL + p00 + TW + 1]};
        int am = 0;
        float m = v[0];
        for (int s4 = 1; s4 < 4; ++s4)
          if (v[s4] > m || (v[s4] != v[s4] && m == m)) { m = v[s4]; am = s4; }
        const int o = c * H2 * W2 + (y0 / 2 + cy) * W2 + x0 / 2 + cx;
        pooled[(size_t)b * d * H2 * W2 + o] = m;
        amax[(size_t)b * d * H2 * W2 + o] = (uint8_t)am;
      }
    }
  }
}

// ===========================================================================
// projection backward (per sample, fans out to K+1 relevance clones):
//   R_a'  = pool-backward(gp, argmax)               (or dense R when no pool follows)
//   g1    = R_a' / stab(a', eps_proj)               Epsilon on invprojection
//   R_h   = h (.) (g1 U)
//   g2    = R_h / stab(h, eps_proj)                  Epsilon on projection (after the mask)
//   clone 0: v = g2 U^T ; clone k: v = g2[block k-1] U[:, block k-1]^T   (SubspaceHook mask)
//   G_q   = [a > 0] (a (.) v) / stab(den, eps_den)   ReLU-backward + the conv rule's division below
// Tiles of 64 pixels (RPT rows x TW cols), lanes = pixels; one tile per workgroup.
// ===========================================================================
constexpr int PT_BWD = 1;   // tiles per workgroup (stored-h backward)

template <int DP, bool PAD, bool MULTI>
__global__ __launch_bounds__(256) void projection_bwd_kernel(
    const float* __restrict__ gp, const uint8_t* __restrict__ amax, const float* __restrict__ ap,
    const float* __restrict__ h, const float* __restrict__ a, const float* __restrict__ den,
    const float* __restrict__ U, float* __restrict__ G, int d_in, int H, int W, int K, float eps_proj, float eps_den,
    int sparse, int has_den, int fanout, const int* __restrict__ u_row, int n_u) {
  const int d = PAD ? d_in : DP;
  if constexpr (MULTI) U += table_offset(u_row, n_u, blockIdx.y, d);
  constexpr int P = 64, LD = DP + 1, PL = P + 4;
  constexpr int NB = DP / 16, TILES = NB * (P / 16), QW = TILES / 4;   // 16x16 blocks; per wave
  // Per wave: pixel block pb = wave, channel blocks cb = 0..NB-1 (q = wave + 4 i).  Its h, a,
  // den values (MFMA output layout) are prefetched at the start, with the staging loads.
  // Rows c >= d (padded embedding) are zero in U and g1 and never stored.
  constexpr bool PF = DP <= 64;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Us = sm;               // [DP][LD]
  float* g1 = Us + DP * LD;     // [DP][PL]
  float* g2 = g1 + DP * PL;     // [DP][PL]
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int b = blockIdx.y;
  const int TW = W < 32 ? W : 32, RPT = P / TW;
  const int HW = H * W, xt = W / TW;
  const int dk = d / K, d4 = (d + 3) & ~3;
  // fanout 1: K+1 clones (standard + K subspaces); 2: the K subspace clones only; 0: replicated rows
  const int nq = fanout == 1 ? (K + 1) : fanout == 2 ? K : 1;
  for (int t = 0; t < PT_BWD; ++t) {
    const int tile = blockIdx.x * PT_BWD + t;
    if (tile >= (H / RPT) * xt) break;
    const int y0 = (tile / xt) * RPT, x0 = (tile % xt) * TW;
    // this lane's pixel in its wave's 16-pixel block, and the channel rows it owns
    const int pl = w * 16 + (lane & 15);
    const size_t pixl = (size_t)(y0 + pl / TW) * W + x0 + pl % TW;
    float hv[PF ? QW * 4 : 1], av[PF ? QW * 4 : 1], dv[PF ? QW * 4 : 1];
    if constexpr (PF) {
#pragma unroll
      for (int i = 0; i < QW; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = i * 16 + (lane >> 4) * 4 + r;
          const bool ok = c < d;
          const size_t os = ((size_t)b * d + (ok ? c : 0)) * HW + pixl;
          const float hh = h[os], aa = a[os], dd = has_den ? den[os] : 1.f;
          hv[i * 4 + r] = ok ? hh : 0.f;
          av[i * 4 + r] = ok ? aa : 0.f;
          dv[i * 4 + r] = dd;
        }
    }
    __syncthreads();
    if (t == 0) stage_u_padded<DP>(Us, U, d, tid);
#pragma unroll 1
    for (int i = tid; i < DP * P; i += 256) {
      const int c = i / P, p = i % P;
      const int y = y0 + p / TW, x = x0 + p % TW;
      const bool ok = c < d;
      const int cc = ok ? c : 0;
      float R;
      if (sparse) {
        const int H2 = H / 2, W2 = W / 2;
        const size_t q = ((size_t)b * d + cc) * H2 * W2 + (y >> 1) * W2 + (x >> 1);
        const float gv = gp[q];
        R = (amax[q] == (((y & 1) << 1) | (x & 1))) ? gv : 0.f;
      } else {
        R = gp[((size_t)b * d + cc) * HW + y * W + x];
      }
      const float v = R / stab(ap[((size_t)b * d + cc) * HW + y * W + x], eps_proj);
      g1[c * PL + p] = ok ? v : 0.f;
    }
    __syncthreads();
    // t[j][p] = sum_c U[c][j] g1[c][p];  R_h = h (.) t;  g2 = R_h / stab(h)
#pragma unroll
    for (int i = 0; i < QW; ++i) {
      const int jb = i, pb = w;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int k0 = 0; k0 < d4; k0 += 4) {
        const int c = k0 + (lane >> 4);
        acc = mfma16(Us[c * LD + jb * 16 + (lane & 15)], g1[c * PL + pb * 16 + (lane & 15)], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jb * 16 + (lane >> 4) * 4 + r, p = pb * 16 + (lane & 15);
        float hx;
        if constexpr (PF) {
          hx = hv[i * 4 + r];
        } else {
          const float hh = h[((size_t)b * d + (j < d ? j : 0)) * HW + pixl];
          hx = j < d ? hh : 0.f;
        }
        const float Rh = hx * acc[r];
        g2[j * PL + p] = Rh / stab(hx, eps_proj);
      }
    }
    __syncthreads();
    for (int qi = 0; qi < nq; ++qi) {
      const int q = fanout == 1 ? qi : fanout == 2 ? qi + 1 : b % (K + 1);
      const int j0 = q == 0 ? 0 : (q - 1) * dk, j1 = q == 0 ? d : q * dk;
      const size_t orow = fanout ? (size_t)b * nq + qi : (size_t)b;
#pragma unroll
      for (int i = 0; i < QW; ++i) {
        const int cb = i, pb = w;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int k0 = j0; k0 < j1; k0 += 4) {
          const int j = k0 + (lane >> 4);
          const bool ok = j < j1;
          const float ua = ok ? Us[(cb * 16 + (lane & 15)) * LD + j] : 0.f;
          const float gb = ok ? g2[j * PL + pb * 16 + (lane & 15)] : 0.f;
          acc = mfma16(ua, gb, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = cb * 16 + (lane >> 4) * 4 + r;
          const bool cok = c < d;
          const size_t os = ((size_t)b * d + (cok ? c : 0)) * HW + pixl;
          float ax, dx;
          if constexpr (PF) { ax = av[i * 4 + r]; dx = dv[i * 4 + r]; }
          else { ax = a[os]; dx = has_den ? den[os] : 1.f; }
          const float Rv = ax * acc[r];
          float gq;
          if (has_den) {
            const float qd = div_nb(Rv, stab(dx, eps_den));   // every lane, then the select
            gq = (ax > 0.f) ? qd : 0.f;
          } else {
            gq = (ax > 0.f) ? Rv : 0.f;
          }
          if (cok) G[(orow * d + c) * HW + pixl] = gq;
        }
      }
    }
  }
}

// ===========================================================================
// projection backward with h and a' recomputed from a (no h / a' buffers in HBM: the forward
// then writes only the pooled a' and its argmax).  Same math and the same MFMA operand order
// as projection_fwd_kernel (h, a') and projection_bwd_kernel (t, clones), so every value is
// bit-identical to the stored-buffer path.  Each wave owns one 16-pixel block of the 64-pixel
// tile end to end, so after U is staged no workgroup barrier is needed:
//   region A [DP][16]: a, then g1;  region B [DP][16]: h, then g2   (wave-private LDS)
// ===========================================================================
// tiles per workgroup (U staged once): 2 / 4 / 8 -> 0.332-0.334 / 0.337-0.338 / 0.378-0.385 ms in the step
constexpr int PT_RC = 2;

// 3 waves/SIMD at DP <= 64: the a' pass below is a separate GEMM so that its accumulators fit there.
// SPARSE (a 2x2 max-pool follows the projection: gp is pooled, amax selects) and DEN (the lower
// layer's denominator is given) are compile-time: tested per element at run time they cost the
// DP = 64 kernel 48 of its 71 branches.
template <int DP, bool PAD, bool SPARSE, bool DEN, bool MULTI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DP <= 64 ? 3 : 1))) void projection_bwd_rc_kernel(
    const float* __restrict__ gp, const uint8_t* __restrict__ amax, const float* __restrict__ a,
    const float* __restrict__ den, const float* __restrict__ U, const float* __restrict__ Pm, float* __restrict__ G,
    int d_in, int H, int W, int K, float eps_proj, float eps_den, int fanout, const int* __restrict__ u_row,
    int n_u) {
  const int d = PAD ? d_in : DP;
  if constexpr (MULTI) {
    const size_t uo = table_offset(u_row, n_u, blockIdx.y, d);
    U += uo;
    Pm += uo;
  }
  constexpr int P = 64, LD = DP + 1, PW = 16, NB = DP / 16;
  constexpr bool PF = DP <= 64;   // keep a / den of the output rows in registers
  // the tile's relevance gather (gp, and amax when SPARSE) as one batch of loads in flight across
  // the a' GEMM: 162 of the 168 VGPRs of 3 waves/SIMD at d = DP = 64.  Where its 2 NB * 4
  // registers do not fit without (more) scratch -- DP = 128, and d < DP = 64 with its padding
  // selects -- the gather stays per element, after that GEMM.
  constexpr bool GATHER = DP <= 32 || (DP == 64 && !PAD);
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  float* Us = sm;                                   // [DP][LD]
  float* RA = Us + DP * LD + w * 2 * DP * PW;       // [DP][PW]
  float* RB = RA + DP * PW;                         // [DP][PW]
  const int b = blockIdx.y;
  const int TW = W < 32 ? W : 32, RPT = P / TW;
  const int HW = H * W, xt = W / TW, H2 = H / 2, W2 = W / 2;
  // per-sample bases (uniform, 64-bit) + 32-bit per-lane offsets: saddr + voffset addressing
  // instead of a 64-bit multiply-add per element (the host keeps d * H * W < 2^31)
  const float* __restrict__ a_b = a + (size_t)b * d * HW;
  const float* __restrict__ den_b = DEN ? den + (size_t)b * d * HW : a_b;
  const float* __restrict__ gp_b = gp + (size_t)b * d * (SPARSE ? H2 * W2 : HW);
  const uint8_t* __restrict__ am_b = SPARSE ? amax + (size_t)b * d * H2 * W2 : nullptr;
  const int dk = d / K, d4 = (d + 3) & ~3;
  // fanout 1: K+1 clones (standard + K subspaces); 2: the K subspace clones only; 0: replicated rows.
  // Clone qi masks subspace q0 + qi (0 = none) and writes output row orow0 + qi.
  const int nq = fanout == 1 ? (K + 1) : fanout == 2 ? K : 1;
  const int q0 = fanout == 1 ? 0 : fanout == 2 ? 1 : b % (K + 1);
  const size_t orow0 = fanout ? (size_t)b * nq : (size_t)b;
  const int pc = lane & 15, rg = lane >> 4;         // pixel column / row group of the MFMA layouts
  stage_u_padded<DP>(Us, U, d, tid);
  __syncthreads();
  for (int t = 0; t < PT_RC; ++t) {
    const int tile = blockIdx.x * PT_RC + t;
    if (tile >= (H / RPT) * xt) break;
    const int y0 = (tile / xt) * RPT, x0 = (tile % xt) * TW;
    const int pl = w * 16 + pc;
    const int py = y0 + pl / TW, px = x0 + pl % TW;
    const int pixl = py * W + px;
    const int cell = (py >> 1) * W2 + (px >> 1);
    const int sub = ((py & 1) << 1) | (px & 1);       // this pixel's position in its pool cell
    // a (and den) at rows c = i*16 + 4 rg + r: the output layout of every GEMM below
    float av[NB * 4], dv[PF ? NB * 4 : 1];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = i * 16 + rg * 4 + r;
        const bool ok = c < d;
        const int os = (ok ? c : 0) * HW + pixl;
        const float aa = a_b[os];
        av[i * 4 + r] = ok ? aa : 0.f;
        if constexpr (PF) dv[i * 4 + r] = DEN ? den_b[os] : 1.f;
      }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < NB * 4; ++i) RA[(((i >> 2) * 16) + rg * 4 + (i & 3)) * PW + pc] = av[i];
    __builtin_amdgcn_wave_barrier();
    // Every GEMM below runs its NB output blocks as independent MFMA chains that share the B
    // operand read (per element the k order is the single-chain order of the stored path).
    // h[j][p] = sum_c U[c][j] a[c][p]        (projection_fwd_kernel order)
    {
      f32x4 acc[NB];
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) acc[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int k0 = 0; k0 < d4; k0 += 4) {
        const int c = k0 + rg;
        const float bv = RA[c * PW + pc];
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) acc[jb] = mfma16(Us[c * LD + jb * 16 + pc], bv, acc[jb]);
      }
#pragma unroll
      for (int jb = 0; jb < NB; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) RB[(jb * 16 + rg * 4 + r) * PW + pc] = acc[jb][r];
    }
    __builtin_amdgcn_wave_barrier();
    // a'[c][p] = a[c][p] + sum_k P[c][k] a[k][p]   (projection_fwd_kernel order; a separate pass:
    // folded into the h GEMM above, the second accumulator set spills at 3 waves/SIMD);
    // g1 = R_a' / stab(a')  -> region A (in place of a; a stays in registers)
    {
      // R_a' of the lane's NB * 4 (channel, pixel) elements: every load is issued here,
      // unconditionally (rows past d read row 0), ahead of the GEMM; the argmax select and the
      // divisions follow it, with no wait on memory between them
      float gv[GATHER ? NB * 4 : 1];
      int am[GATHER && SPARSE ? NB * 4 : 1];
      if constexpr (GATHER) {
#pragma unroll
        for (int i = 0; i < NB * 4; ++i) {
          const int c = (i >> 2) * 16 + rg * 4 + (i & 3);
          const int cc = c < d ? c : 0;
          gv[i] = gp_b[SPARSE ? cc * H2 * W2 + cell : cc * HW + pixl];
          if constexpr (SPARSE) am[i] = am_b[cc * H2 * W2 + cell];
        }
      }
      f32x4 acc[NB];
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int k0 = 0; k0 < d4; k0 += 4) {
        const int k = k0 + rg;
        const float bv = RA[k * PW + pc];
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) acc[cb] = mfma16(p_operand(Pm, d, cb * 16 + pc, k), bv, acc[cb]);
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int cb = 0; cb < NB; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = cb * 16 + rg * 4 + r;
          const bool ok = c < d;
          const int cc = ok ? c : 0;
          float R;
          if constexpr (GATHER) {
            R = SPARSE ? ((am[cb * 4 + r] == sub) ? gv[cb * 4 + r] : 0.f) : gv[cb * 4 + r];
          } else if constexpr (SPARSE) {
            const int q = cc * H2 * W2 + cell;
            const float g = gp_b[q];   // unconditional load, then the argmax select
            R = (am_b[q] == sub) ? g : 0.f;
          } else {
            R = gp_b[cc * HW + pixl];
          }
          const float apv = av[cb * 4 + r] + acc[cb][r];
          const float v = R / stab(apv, eps_proj);
          RA[c * PW + pc] = ok ? v : 0.f;
        }
    }
    __builtin_amdgcn_wave_barrier();
    // t[j][p] = sum_c U[c][j] g1[c][p];  g2 = h (.) t / stab(h)  -> region B (in place of h)
    {
      f32x4 acc[NB];
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) acc[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int k0 = 0; k0 < d4; k0 += 4) {
        const int c = k0 + rg;
        const float bv = RA[c * PW + pc];
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) acc[jb] = mfma16(Us[c * LD + jb * 16 + pc], bv, acc[jb]);
      }
#pragma unroll
      for (int jb = 0; jb < NB; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* e = RB + (jb * 16 + rg * 4 + r) * PW + pc;   // this lane's own h element
          const float hx = *e;
          *e = (hx * acc[jb][r]) / stab(hx, eps_proj);
        }
    }
    __builtin_amdgcn_wave_barrier();
    // the clones share a and den: stabilise the denominators once per tile (without den the
    // quotient is x / 1 = x exactly), so the clone epilogue below is branch-free
    if constexpr (PF) {
#pragma unroll
      for (int i = 0; i < NB * 4; ++i) dv[i] = DEN ? stab(dv[i], eps_den) : 1.f;
    }
    for (int qi = 0; qi < nq; ++qi) {
      const int q = q0 + qi;
      const int j0 = q == 0 ? 0 : (q - 1) * dk, j1 = q == 0 ? d : q * dk;
      float* __restrict__ G_q = G + (orow0 + qi) * d * HW;
      f32x4 acc[NB];
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      // operands read unconditionally from an in-range row and zeroed afterwards: one LDS round
      // trip per k-step instead of an exec branch and a wait per read
      if (j1 - j0 == 16) {
        // d_k = 16 (GTZAN j = 7: d = 64, K = 4): all four k-steps' operands in one round trip
        float g0[4], u0[4][NB];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int j = j0 + 4 * s + rg;
          g0[s] = RB[j * PW + pc];
#pragma unroll
          for (int cb = 0; cb < NB; ++cb) u0[s][cb] = Us[(cb * 16 + pc) * LD + j];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int cb = 0; cb < NB; ++cb) acc[cb] = mfma16(u0[s][cb], g0[s], acc[cb]);
      } else
#pragma unroll 2
      for (int k0 = j0; k0 < j1; k0 += 4) {
        const int j = k0 + rg;
        const bool ok = j < j1;
        const int jc = ok ? j : j0;
        const float g0 = RB[jc * PW + pc];
        float u0[NB];
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) u0[cb] = Us[(cb * 16 + pc) * LD + jc];
        const float gb = ok ? g0 : 0.f;
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) acc[cb] = mfma16(ok ? u0[cb] : 0.f, gb, acc[cb]);
      }
#pragma unroll
      for (int cb = 0; cb < NB; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = cb * 16 + rg * 4 + r;
          const bool cok = c < d;
          const int os = (cok ? c : 0) * HW + pixl;
          const float ax = av[cb * 4 + r];
          float sd;
          if constexpr (PF) {
            sd = dv[cb * 4 + r];
          } else {
            const float dx = den_b[os];   // den_b is a valid row (a) without den
            sd = DEN ? stab(dx, eps_den) : 1.f;
          }
          const float qd = div_nb(ax * acc[cb][r], sd);   // every lane, then the select
          const float gq = (ax > 0.f) ? qd : 0.f;
          if (cok) G_q[c * HW + pixl] = gq;
        }
    }
  }
}

// padded projection width: the smallest instantiated DP >= d (0 = unsupported)
int proj_dp(int d) { return d < 1 ? 0 : d <= 16 ? 16 : d <= 32 ? 32 : d <= 64 ? 64 : d <= 128 ? 128 : 0; }

// f(integral_constant<int, DP>) for the padded width of d; owns the one "unsupported d" error
template <class F>
int with_proj_dp(int d, const char* who, F&& f) {
  switch (proj_dp(d)) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
  }
  drsa::set_error("%s: unsupported d=%d", who, d);
  return DRSA_EUNSUPPORTED;
}

// a runtime flag as a template argument: f(std::true_type) or f(std::false_type)
template <class F>
int with_flag(bool on, F&& f) { return on ? f(std::true_type{}) : f(std::false_type{}); }

template <class Kern, class... Args>
int launch_proj(Kern kern, dim3 grid, size_t lds, hipStream_t s, Args... args) {
  DRSA_SMEM(kern, lds);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, args...);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

// dynamic LDS: U [D][D + 1] where staged, plus the kernel's tile regions
template <int D>
size_t proj_fwd_lds(bool hout) { return ((hout ? (size_t)D * (D + 1) : 0) + (size_t)D * 68) * sizeof(float); }
template <int D>
size_t proj_bwd_lds() { return ((size_t)D * (D + 1) + 2 * (size_t)D * 68) * sizeof(float); }
template <int D>
size_t proj_bwd_rc_lds() { return ((size_t)D * (D + 1) + 4 * 2 * (size_t)D * 16) * sizeof(float); }

// The single-matrix and the multi-matrix entries share their checks and their dispatch: u_row == nullptr is the
// single-matrix form (U, P one matrix each), otherwise U and P are tables [n_u][D][D] and u_row [B] names each
// row's matrix.  ``who`` prefixes every message.
int projection_fwd_impl(const char* who, const float* a, const float* U, const float* P, const int* u_row, int n_u,
                        float* h, float* ap, float* pooled, uint8_t* amax, int B, int D, int H, int W, int pool,
                        void* stream) {
  const int TW = W < 32 ? W : 32;
  DRSA_REQUIRE((W == 8 || W == 16 || W % 32 == 0) && H % (64 / TW) == 0,
               "%s: W must be 8, 16 or a multiple of 32 and H a multiple of 64/min(W,32) (got %dx%d)", who, H, W);
  DRSA_REQUIRE(!pool || (pooled && amax), "%s: pool needs outputs", who);
  DRSA_REQUIRE((int64_t)D * H * W < ((int64_t)1 << 31), "%s: one sample's d x H x W must stay below 2^31", who);
  DRSA_REQUIRE(pool || ap, "%s: without pool a' (ap) is the output", who);
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (H / (64 / TW)) * (W / TW);
  const dim3 grid((tiles + PT - 1) / PT, B);
  return with_proj_dp(D, who, [&](auto dp) -> int {
    constexpr int DP = decltype(dp)::value;
    return with_flag(D != DP, [&](auto pad) -> int {
      return with_flag(h != nullptr, [&](auto hout) -> int {
        return with_flag(u_row != nullptr, [&](auto multi) -> int {
          return launch_proj(
              projection_fwd_kernel<DP, decltype(pad)::value, decltype(hout)::value, decltype(multi)::value>, grid,
              proj_fwd_lds<DP>(h != nullptr), s, a, U, P, h, ap, pooled, amax, D, H, W, pool, u_row, n_u);
        });
      });
    });
  });
}

int projection_bwd_impl(const char* who, const float* gp, const uint8_t* amax, const float* ap, const float* h,
                        const float* a, const float* den, const float* U, const float* P, const int* u_row, int n_u,
                        float* G, int B, int D, int H, int W, int K, float eps_proj, float eps_den, int fanout,
                        void* stream) {
  const int TW = W < 32 ? W : 32;
  DRSA_REQUIRE(fanout >= 0 && fanout <= 2, "%s: fanout must be 0, 1 or 2", who);
  DRSA_REQUIRE((int64_t)D * H * W < ((int64_t)1 << 31), "%s: one sample's d x H x W must stay below 2^31", who);
  DRSA_REQUIRE(gp && a && U && G && ((ap && h) || P),
               "%s: gp, a, U, G and P (when h / a' are recomputed) are required", who);
  DRSA_REQUIRE((W == 8 || W == 16 || W % 32 == 0) && H % (64 / TW) == 0,
               "%s: W must be 8, 16 or a multiple of 32 and H a multiple of 64/min(W,32) (got %dx%d)", who, H, W);
  DRSA_REQUIRE(K > 0 && D % K == 0, "%s: K must divide d", who);
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (H / (64 / TW)) * (W / TW);
  const int sparse = amax != nullptr, has_den = den != nullptr;
  const bool recompute = !ap || !h;   // h and a' rebuilt from a
  return with_proj_dp(D, who, [&](auto dp) -> int {
    constexpr int DP = decltype(dp)::value;
    return with_flag(D != DP, [&](auto pad) -> int {
      constexpr bool PAD = decltype(pad)::value;
      return with_flag(u_row != nullptr, [&](auto multi) -> int {
        constexpr bool MULTI = decltype(multi)::value;
        if (recompute)
          return with_flag(sparse, [&](auto sp) -> int {
            return with_flag(has_den, [&](auto dn) -> int {
              return launch_proj(projection_bwd_rc_kernel<DP, PAD, decltype(sp)::value, decltype(dn)::value, MULTI>,
                                 dim3((tiles + PT_RC - 1) / PT_RC, B), proj_bwd_rc_lds<DP>(), s, gp, amax, a, den, U, P,
                                 G, D, H, W, K, eps_proj, eps_den, fanout, u_row, n_u);
            });
          });
        return launch_proj(projection_bwd_kernel<DP, PAD, MULTI>, dim3((tiles + PT_BWD - 1) / PT_BWD, B),
                           proj_bwd_lds<DP>(), s, gp, amax, ap, h, a, den, U, G, D, H, W, K, eps_proj, eps_den, sparse,
                           has_den, fanout, u_row, n_u);
      });
    });
  });
}

}  // namespace

extern "C" {

int drsa_amd_projection_residual(const float* U, int D, float* P, void* stream) {
  DRSA_REQUIRE(U && P && D >= 1 && D <= 128, "projection_residual: need U, P and 1 <= d <= 128");
  hipLaunchKernelGGL(projection_residual_kernel, dim3((D * D + 255) / 256), dim3(256), 0, (hipStream_t)stream, U, D, P);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

int drsa_amd_projection_fwd(const float* a, const float* U, const float* P, float* h, float* ap, float* pooled,
                            uint8_t* amax, int B, int D, int H, int W, int pool, void* stream) {
  DRSA_REQUIRE(a && U && P, "projection_fwd: a, U and P (drsa_amd_projection_residual) are required");
  return projection_fwd_impl("projection_fwd", a, U, P, nullptr, 0, h, ap, pooled, amax, B, D, H, W, pool, stream);
}

int drsa_amd_projection_bwd(const float* gp, const uint8_t* amax, const float* ap, const float* h, const float* a,
                            const float* den, const float* U, const float* P, float* G, int B, int D, int H, int W,
                            int K, float eps_proj, float eps_den, int fanout, void* stream) {
  return projection_bwd_impl("projection_bwd", gp, amax, ap, h, a, den, U, P, nullptr, 0, G, B, D, H, W, K, eps_proj,
                             eps_den, fanout, stream);
}

int drsa_amd_projection_fwd_multi(const float* a, const float* U_tab, const float* P_tab, const int* u_row, int n_u,
                                  float* h, float* ap, float* pooled, uint8_t* amax, int B, int D, int H, int W,
                                  int pool, void* stream) {
  const char* who = "projection_fwd_multi";
  DRSA_REQUIRE(a && U_tab && P_tab && u_row,
               "%s: a, U_tab, P_tab (drsa_amd_projection_residual per matrix) and u_row are required", who);
  DRSA_REQUIRE(n_u >= 1, "%s: the table needs at least one matrix (n_u=%d)", who, n_u);
  DRSA_REQUIRE(D >= 1 && D <= 128, "%s: need 1 <= d <= 128 (got %d)", who, D);
  return projection_fwd_impl(who, a, U_tab, P_tab, u_row, n_u, h, ap, pooled, amax, B, D, H, W, pool, stream);
}

int drsa_amd_projection_bwd_multi(const float* gp, const uint8_t* amax, const float* ap, const float* h,
                                  const float* a, const float* den, const float* U_tab, const float* P_tab,
                                  const int* u_row, int n_u, float* G, int B, int D, int H, int W, int K,
                                  float eps_proj, float eps_den, int fanout, void* stream) {
  const char* who = "projection_bwd_multi";
  DRSA_REQUIRE(U_tab && P_tab && u_row, "%s: U_tab, P_tab and u_row are required", who);
  DRSA_REQUIRE(n_u >= 1, "%s: the table needs at least one matrix (n_u=%d)", who, n_u);
  DRSA_REQUIRE(D >= 1 && D <= 128, "%s: need 1 <= d <= 128 (got %d)", who, D);
  return projection_bwd_impl(who, gp, amax, ap, h, a, den, U_tab, P_tab, u_row, n_u, G, B, D, H, W, K, eps_proj, eps_den,
                             fanout, stream);
}

}  // extern "C"

