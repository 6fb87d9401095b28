// DRSA step: the partial kernel of the natural (unpadded) geometry -- every K | d at d <= 128.
#pragma once
#include "common.h"
#include "drsa_geom.h"
#include "drsa_partial.h"

namespace {

// ---------------------------------------------------------------------------
// ragged partial kernel
// ---------------------------------------------------------------------------
// The padded kernels (drsa_partial.h) form a concept's sum s = sum_j XA_nj XC_nj with shfl_xor trees
// over aligned power-of-two lane groups.  Here concept k owns the real columns [k dk, (k + 1) dk)
// of a DP = pow2ceil(max(16, d)) wide problem, for any dk = d / K: a concept may start at any lane
// and straddle 16-wide column blocks and waves, so the sums go through LDS instead.
//
// Tiles, waves and the prefetch are PCfg<DP, 16>'s: wave w owns the 16-wide column block w % CG
// and the row blocks w / CG, w / CG + WPG, ... of a staged tile; the CG waves of one "wave row"
// w / CG work on one 16-row block together:
//   1. GEMM1 (XA = A U, XC = C U, k-ascending 16x16x4 fp32 MFMA chains) for the wave's 16 columns;
//      p = XA (.) XC (one rounded product per entry) -> strip[16][DP] of the wave row       | barrier
//   2. thread e of the wave row, e = 16 k + row (k < K; up to four e per thread):
//      s = ((+0 + p[row][k dk]) + p[row][k dk + 1]) + ... in ascending column order, r = max(s, 0)
//      -> rbuf[e], and r^2 added to the thread's private S partial of e                     | barrier
//   3. each lane reads r of its column's concept (column / dk) for its four rows; GEMM2
//      (Gt += A^T (r XC) + C^T (r XA)) as in rowblock_step.
// The two barriers are workgroup-wide, so every wave runs the same ceil(nrb / WPG) passes over a
// tile and idles in a pass that has no row block for its wave row.  Waves whose 16 columns all lie
// at or beyond d skip the MFMAs (their U block is zero) but take part in step 2.
// Columns >= d and rows >= N are staged as zeros: p, r and every Gt term there are exact zeros.
//
// Combine (fixed order, no atomics): Gt as drsa_partial_kernel -- for each column block the left
// fold from +0 over its waves w = cg, cg + CG, ...; S_k = the left fold from +0 over the wave rows
// (ascending) of the left fold over rows 0..15 of the S partials of (k, row).
template <int DP>
struct NCfg {
  using P = PCfg<DP, 16>;
  static constexpr int CG = P::CG, NIB = P::NIB, NW = P::NW, NT = P::NT;
  static constexpr int RT = P::RT, LDA = P::LDA, NV = P::NV, PFN = P::PFN;
  static constexpr int WPG = NW / CG;              // wave rows = row blocks in flight
  static constexpr int GT = CG * 64;               // threads of a wave row (= 4 DP)
  static constexpr int SPT = 16 * DP / GT;         // (row, concept) slots per thread: 4
  static constexpr int SP = DP + 1;                // strip row stride: the 16 rows on 16 banks
  static constexpr size_t tile_floats = P::tile_floats;
  static constexpr size_t strip_floats = (size_t)WPG * 16 * SP;
  static constexpr size_t rbuf_floats = (size_t)WPG * 16 * DP;
  static constexpr size_t work_floats = tile_floats + strip_floats + rbuf_floats;   // the strips do not alias the tiles
  static constexpr size_t red_floats = (size_t)NW * DP * 16 + (size_t)WPG * 16 * DP;
  static constexpr size_t lds_bytes = (work_floats > red_floats ? work_floats : red_floats) * sizeof(float);
  static_assert(P::CW == 16 && P::NCB == 1, "natural partial: 16-wide column groups");
  static_assert(SPT * GT == 16 * DP && NW % CG == 0, "natural partial: slots");
  static_assert(lds_bytes <= 160 * 1024, "natural partial: LDS");
};

template <int DP, bool VEC>
__global__ __launch_bounds__((NCfg<DP>::NT)) void drsa_partial_nat_kernel(
    const float* __restrict__ A, const float* __restrict__ C, int64_t N, int d, int K, int dk,
    const float* __restrict__ U, float* __restrict__ partials, int64_t rb_total, int slab_stride_floats) {
  using Cfg = NCfg<DP>;
  constexpr int CG = Cfg::CG, NIB = Cfg::NIB, NW = Cfg::NW, NT = Cfg::NT, RT = Cfg::RT, LDA = Cfg::LDA;
  constexpr int NV = Cfg::NV, PFN = Cfg::PFN, WPG = Cfg::WPG, GT = Cfg::GT, SPT = Cfg::SPT, SP = Cfg::SP;
  constexpr int NQ = DP / 16, RB = RT / 16;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = lane_id(), w = __builtin_amdgcn_readfirstlane(wave_id());
  const int l15 = lane & 15, lg = lane >> 4;
  const int cg = w % CG, wg = w / CG;
  const int tg = cg * 64 + lane;                          // thread within the wave row
  float* As = smem;                                       // [RT][LDA]
  float* Cs = smem + RT * LDA;                            // [RT][LDA]
  float* strip = smem + Cfg::tile_floats + (size_t)wg * 16 * SP;               // [16][SP]  p of this wave row
  float* rbuf = smem + Cfg::tile_floats + Cfg::strip_floats + (size_t)wg * 16 * DP;   // [K][16]   r of this wave row
  const int nblk = (int)gridDim.x;
  const int64_t rb0 = (int64_t)blockIdx.x * rb_total / nblk;
  const int64_t rb1 = (int64_t)(blockIdx.x + 1) * rb_total / nblk;
  const int ntile = (int)((rb1 - rb0 + RB - 1) / RB);

  // ---- tile staging: partial_core's (fp32) ----
  float4 pa[PFN], pc[PFN];
  uint32_t okm = 0;
  static_assert(PFN <= 32, "prefetch mask");
  auto load_tile = [&](int t) {
    const int64_t r0 = (rb0 + (int64_t)t * RB) * 16;
    const int64_t rmax = rb1 * 16 < N ? rb1 * 16 : N;
    const float* Ab = A + r0 * d;
    const float* Cb = C + r0 * d;
#pragma unroll
    for (int p = 0; p < PFN; ++p) {
      const int i = tid + p * NT;
      const int row = (i / (DP / 4)) % RT, col = 4 * (i % (DP / 4));
      const bool ok = i < NV && r0 + row < rmax && col < d;
      const unsigned off = ok ? (unsigned)(row * d + col) : 0u;
      float4 a, c;
      if constexpr (VEC) {
        a = *reinterpret_cast<const float4*>(Ab + off);
        c = *reinterpret_cast<const float4*>(Cb + off);
      } else {
        float va[4], vc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned o = (ok && col + u < d) ? off + u : 0u;
          const float xa = Ab[o], xc = Cb[o];
          va[u] = keep_or_zero(xa, col + u < d);
          vc[u] = keep_or_zero(xc, col + u < d);
        }
        a = make_float4(va[0], va[1], va[2], va[3]);
        c = make_float4(vc[0], vc[1], vc[2], vc[3]);
      }
      pa[p] = a;
      pc[p] = c;
      okm = (okm & ~(1u << p)) | ((ok ? 1u : 0u) << p);
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int p = 0; p < PFN; ++p) {
      const int i = tid + p * NT;
      if (i < NV) {
        const int row = i / (DP / 4), col = 4 * (i % (DP / 4));
        const bool ok = (okm >> p) & 1u;
        *reinterpret_cast<float4*>(As + row * LDA + col) = keep_or_zero4(pa[p], ok);
        *reinterpret_cast<float4*>(Cs + row * LDA + col) = keep_or_zero4(pc[p], ok);
      }
    }
  };
  if (ntile > 0) load_tile(0);

  // ---- U for this wave's 16 columns in MFMA B-operand order: ureg[q][t] = U[16 q + 4 lg + t][16 cg + l15] ----
  const int col = 16 * cg + l15;
  const bool real = col < d;
  const bool live = 16 * cg < d;                           // uniform: the wave has a real column
  float ureg[NQ][4];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = 16 * q + 4 * lg + t;
      const float v = U[(size_t)(k < d ? k : 0) * d + (real ? col : 0)];   // clamped address, masked after
      ureg[q][t] = keep_or_zero(v, real && k < d);
    }
  const int roff = (real ? col / dk : 0) * 16 + 4 * lg;   // this lane's r in rbuf: concept col / dk, rows 4 lg + tt

  f32x4 g[NIB];
#pragma unroll
  for (int ib = 0; ib < NIB; ++ib) g[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sacc[SPT];
#pragma unroll
  for (int i = 0; i < SPT; ++i) sacc[i] = 0.f;
  const int nq_live = (d + 15) / 16;   // k chunks / Gt row blocks that can be nonzero

  if (ntile > 0) store_tile();
  __syncthreads();
  for (int t = 0; t < ntile; ++t) {
    if (t + 1 < ntile) load_tile(t + 1);
    const int64_t rbt = rb0 + (int64_t)t * RB;
    const int nrb = (int)((rb1 - rbt) < RB ? (rb1 - rbt) : RB);
    for (int rbase = 0; rbase < nrb; rbase += WPG) {     // uniform trip count: barriers inside
      const int rbl = rbase + wg;
      const bool act = rbl < nrb;                        // uniform per wave
      const float* Ar = As + 16 * rbl * LDA;
      const float* Cr = Cs + 16 * rbl * LDA;
      // ---- 1. GEMM1 and p -> strip ----
      f32x4 xa = {0.f, 0.f, 0.f, 0.f}, xc = xa;
      if (act && live) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          if (q >= nq_live) break;
          const float4 a4 = *reinterpret_cast<const float4*>(Ar + l15 * LDA + 16 * q + 4 * lg);
          const float4 c4 = *reinterpret_cast<const float4*>(Cr + l15 * LDA + 16 * q + 4 * lg);
          const float av[4] = {a4.x, a4.y, a4.z, a4.w}, cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) {
            xa = mfma16(av[tt], ureg[q][tt], xa);
            xc = mfma16(cv[tt], ureg[q][tt], xc);
          }
        }
        // lane holds rows 4 lg + r, column 16 cg + l15
#pragma unroll
        for (int r = 0; r < 4; ++r) strip[(4 * lg + r) * SP + col] = xa[r] * xc[r];
      }
      __syncthreads();
      // ---- 2. s, r = relu(s), S partials ----
      if (act) {
#pragma unroll
        for (int i = 0; i < SPT; ++i) {
          const int e = tg + i * GT, k = e >> 4, row = e & 15;
          if (k < K) {
            const float* p = strip + row * SP + k * dk;
            float s = 0.f;
#pragma unroll 4
            for (int c = 0; c < dk; ++c) s += p[c];
            const float rv = s > 0.f ? s : 0.f;
            rbuf[e] = rv;
            sacc[i] += rv * rv;
          }
        }
      }
      __syncthreads();
      // ---- 3. GEMM2: Gt[i][j] += sum_n A[n][i] P[n][j] + C[n][i] Q[n][j]  (P = r XC, Q = r XA) ----
      if (act && live) {
        float pv[4], qv[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const float rr = keep_or_zero(rbuf[roff + tt], real);
          pv[tt] = rr * xc[tt];
          qv[tt] = rr * xa[tt];
        }
#pragma unroll
        for (int ib = 0; ib < NIB; ++ib) {
          if (ib >= nq_live) break;
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) {
            const float av = Ar[(4 * lg + tt) * LDA + 16 * ib + l15];
            const float cv = Cr[(4 * lg + tt) * LDA + 16 * ib + l15];
            g[ib] = mfma16(av, pv[tt], g[ib]);
            g[ib] = mfma16(cv, qv[tt], g[ib]);
          }
        }
      }
    }
    if (t + 1 < ntile) {
      __syncthreads();
      store_tile();
      __syncthreads();
    }
  }

  // ---- combine the waves of each column block in a fixed order -> slab ----
  __syncthreads();
  float* red = smem;                                  // [NW][DP][16]
  float* sred = smem + (size_t)NW * DP * 16;          // [WPG][16 DP]: S partial of e = 16 k + row per wave row
#pragma unroll
  for (int ib = 0; ib < NIB; ++ib)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[((size_t)w * DP + 16 * ib + 4 * lg + r) * 16 + l15] = g[ib][r];
#pragma unroll
  for (int i = 0; i < SPT; ++i) sred[(size_t)wg * 16 * DP + tg + i * GT] = sacc[i];
  __syncthreads();
  float* slab = partials + (size_t)blockIdx.x * slab_stride_floats;
  for (int e = tid; e < DP * DP; e += NT) {
    const int i = e / DP, j = e % DP, gcg = j / 16, jj = j % 16;
    float acc = 0.f;
    for (int ww = gcg; ww < NW; ww += CG) acc += red[((size_t)ww * DP + i) * 16 + jj];
    slab[e] = acc;
  }
  for (int k = tid; k < K; k += NT) {
    float acc = 0.f;
    for (int q = 0; q < WPG; ++q) {
      float rows = 0.f;
      for (int row = 0; row < 16; ++row) rows += sred[(size_t)q * 16 * DP + 16 * k + row];
      acc += rows;
    }
    slab[DP * DP + k] = acc;
  }
}

}  // namespace
