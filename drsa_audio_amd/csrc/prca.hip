// Principal Relevant Component Analysis on gfx950: the relevance cross-covariance of the DRSA rows
// and a symmetric eigensolver for it, both on device (the closed-form companion of DRSA in the
// same paper: the orthonormal U maximising tr(U^T M U), M = (A^T C + C^T A) / (2N), is the
// eigenvectors of the symmetric indefinite M by descending eigenvalue).
//
//   prca_partial_kernel   G_l = A_l^T C_l for the rows of leaf l, fp32 MFMA 32x32x2.  Both operands
//                         of A^T C are "row n, 32 consecutive columns", so the row-major tiles feed
//                         the MFMA as they lie in LDS (no transpose).  Rows >= N and columns >= d are
//                         staged as exact +0.
//   prca_reduce_kernel    fixed-order sum of the leaf slabs -> the un-normalised G [d][d].
//   prca_finish_kernel    M[i][j] = (G[i][j] + G[j][i]) / (2 N_total): symmetric bit for bit.
//   syevj_kernel          one workgroup, M in LDS and V in registers: parallel cyclic two-sided
//                         Jacobi in round-robin order, then V re-orthogonalised by the Newton-Schulz
//                         polar (polar_ns.h), eigenvalues recomputed as Rayleigh quotients against
//                         the input, stable descending sort, sign rule.
//
// Determinism (the rule of the DRSA gradient, drsa_step.hip): the rows are cut into
// L = min(256, ceil(N / 16)) leaves of whole 16-row blocks, leaf l = blocks [l R / L, (l + 1) R / L);
// a leaf is summed by its workgroup's fixed wave order into its own slab, and the slabs are folded
// left to right in groups of 8, the groups left to right.  Constants, not the CU count, and no
// atomics: the bits do not depend on the device or the grid.
#include "common.h"
#include "drsa_amd.h"
#include "polar_ns.h"

#include <type_traits>

namespace {

inline int pow2ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}
inline int padded_dim(int d) { return pow2ceil(d < 32 ? 32 : d); }

__device__ __forceinline__ float keep_or_zero(float v, bool keep) {
  return __uint_as_float(__float_as_uint(v) & (keep ? 0xffffffffu : 0u));
}
__device__ __forceinline__ float4 keep_or_zero4(float4 v, bool keep) {
  return make_float4(keep_or_zero(v.x, keep), keep_or_zero(v.y, keep), keep_or_zero(v.z, keep),
                     keep_or_zero(v.w, keep));
}

constexpr int kLeaves = 256;
constexpr int kLeafGroup = 8;
constexpr int kMaxGroups = kLeaves / kLeafGroup;

inline int64_t row_blocks(int64_t N) { return (N + 15) / 16; }
inline int leaves(int64_t N) {
  const int64_t R = row_blocks(N);
  return (int)(R < kLeaves ? R : kLeaves);
}

// ---------------------------------------------------------------------------
// cross-covariance
// ---------------------------------------------------------------------------
template <int DP>
struct CovCfg {
  static constexpr int NB = DP / 32;               // 32-wide blocks per side
  static constexpr int NTILE = NB * NB;            // 32x32 output tiles
  // below DP = 128 a tile's rows are split over KS waves (summed kq ascending through LDS)
  static constexpr int KS = NTILE >= 16 ? 1 : 4;
  static constexpr int NW = NTILE * KS;
  static constexpr int NT = NW * 64;
  static constexpr int RT = 64;                    // rows per staged tile
  static constexpr int LDA = DP + 4;               // 16-B aligned rows; a 32-lane operand read is one row
  static constexpr int NV = RT * DP / 4;           // float4 slots per matrix per tile
  static constexpr int PFN = (NV + NT - 1) / NT;
  static constexpr size_t tile_floats = 2 * (size_t)RT * LDA;
  static constexpr size_t red_floats = (size_t)NW * 1024;
  static constexpr size_t lds_bytes = (tile_floats > red_floats ? tile_floats : red_floats) * sizeof(float);
  static_assert(RT % (2 * KS) == 0, "whole k-steps per wave");
};

// Workgroup l = leaf l.  All threads stage RT rows of A and C into LDS (the next tile's loads are
// in flight in registers while the current one is multiplied); wave w owns output tile w / KS
// (G rows 32 ib.., columns 32 jb..) and the tile rows [kq RT / KS, (kq + 1) RT / KS), kq = w % KS.
// VEC (d % 4 == 0 and 16-B aligned bases): float4 row loads.  Every load is from a clamped, valid
// address and masked afterwards: nothing is read past A + N d.
template <int DP, bool VEC>
__global__ __launch_bounds__(CovCfg<DP>::NT) void prca_partial_kernel(const float* __restrict__ A,
                                                                      const float* __restrict__ C, int64_t N, int d,
                                                                      int64_t rb_total, int L,
                                                                      float* __restrict__ leaf_slabs) {
  using Cfg = CovCfg<DP>;
  constexpr int NB = Cfg::NB, KS = Cfg::KS, NT = Cfg::NT, RT = Cfg::RT, LDA = Cfg::LDA, NV = Cfg::NV, PFN = Cfg::PFN;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;
  float* Cs = smem + RT * LDA;
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int lo = lane & 31, hi = lane >> 5;
  const int tile = w / KS, kq = w % KS, ib = tile / NB, jb = tile % NB;

  const int64_t rb0 = (int64_t)blockIdx.x * rb_total / L, rb1 = (int64_t)(blockIdx.x + 1) * rb_total / L;
  const int64_t row0 = rb0 * 16, row1 = rb1 * 16 < N ? rb1 * 16 : N;
  const int ntile = (int)((row1 - row0 + RT - 1) / RT);

  float4 pa[PFN], pc[PFN];
  uint32_t okm = 0;
  auto load_tile = [&](int t) {
    const int64_t r0 = row0 + (int64_t)t * RT;
#pragma unroll
    for (int p = 0; p < PFN; ++p) {
      const int i = tid + p * NT;
      const int row = (i / (DP / 4)) % RT, col = 4 * (i % (DP / 4));
      const bool ok = i < NV && r0 + row < row1 && col < d;
      const size_t off = ok ? (size_t)(r0 + row) * d + col : 0;
      float4 a, c;
      if constexpr (VEC) {
        a = *reinterpret_cast<const float4*>(A + off);
        c = *reinterpret_cast<const float4*>(C + off);
      } else {
        float va[4], vc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool oku = ok && col + u < d;
          const size_t o = oku ? off + u : 0;
          va[u] = keep_or_zero(A[o], oku);
          vc[u] = keep_or_zero(C[o], oku);
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

  f32x16 acc = {};
  if (ntile > 0) {
    load_tile(0);
    store_tile();
  }
  __syncthreads();
  for (int t = 0; t < ntile; ++t) {
    if (t + 1 < ntile) load_tile(t + 1);
    constexpr int KR = RT / KS;
#pragma unroll 8
    for (int k0 = kq * KR; k0 < (kq + 1) * KR; k0 += 2) {
      const int kk = k0 + hi;
      acc = mfma32(As[kk * LDA + 32 * ib + lo], Cs[kk * LDA + 32 * jb + lo], acc);
    }
    if (t + 1 < ntile) {
      __syncthreads();
      store_tile();
      __syncthreads();
    }
  }

  // the waves of a tile in kq order -> the leaf's slab (padded coordinates [DP][DP])
  __syncthreads();
  float* red = smem;   // [NW][16][64]
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(size_t)w * 1024 + r * 64 + lane] = acc[r];
  __syncthreads();
  float* slab = leaf_slabs + (size_t)blockIdx.x * DP * DP;
  for (int e = tid; e < DP * DP; e += NT) {
    const int i = e / DP, j = e % DP, tt = (i / 32) * NB + j / 32, ri = i % 32;
    const int r = (ri & 3) | ((ri >> 3) << 2), ln = (j % 32) + 32 * ((ri >> 2) & 1);
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < KS; ++q) v += red[(size_t)(tt * KS + q) * 1024 + r * 64 + ln];
    slab[e] = v;
  }
}

// out[i][j] (unpadded [d][d]) = the left fold over leaf groups of the left fold over each group's
// leaf slabs, both from +0.  Thread group grp of a block sums the groups grp, grp + 4, ... with the
// eight slab loads of a group issued together; one thread per element then folds the group sums.
__global__ __launch_bounds__(256) void prca_reduce_kernel(const float* __restrict__ leaf_slabs, int L, int DP, int d,
                                                          float* __restrict__ out) {
  __shared__ float part[kMaxGroups][64];
  const int l = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + l, E = d * d;
  const int ec = e < E ? e : 0;
  const size_t src = (size_t)(ec / d) * DP + ec % d, ES = (size_t)DP * DP;
  const int ng = (L + kLeafGroup - 1) / kLeafGroup;
#pragma unroll
  for (int q0 = 0; q0 < kMaxGroups; q0 += 4) {
    const int qq = q0 + grp;
    if (q0 >= ng) break;   // uniform
    float v[kLeafGroup];
#pragma unroll
    for (int i = 0; i < kLeafGroup; ++i) {
      const int p = qq * kLeafGroup + i;
      v[i] = leaf_slabs[(size_t)(qq < ng && p < L ? p : 0) * ES + src];
    }
    float G = 0.f;
#pragma unroll
    for (int i = 0; i < kLeafGroup; ++i)
      if (qq * kLeafGroup + i < L) G += v[i];
    if (qq < ng) part[qq][l] = G;
  }
  __syncthreads();
  if (grp == 0 && e < E) {
    float T = 0.f;
    for (int qq = 0; qq < ng; ++qq) T += part[qq][l];
    out[e] = T;
  }
}

__global__ __launch_bounds__(256) void prca_finish_kernel(const float* __restrict__ G, int d, float inv2n,
                                                          float* __restrict__ M) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= d * d) return;
  const int i = e / d, j = e % d;
  M[e] = (G[i * d + j] + G[j * d + i]) * inv2n;   // a + b == b + a: M is symmetric bit for bit
}

// ---------------------------------------------------------------------------
// symmetric eigensolver
// ---------------------------------------------------------------------------
constexpr int kMaxSweeps = 30;
// A pair rests when |m_pq| <= kSkipTol * max_k |m_kk| (the diagonal at the start of the sweep):
// one float32 rounding of the matrix's scale, which also bounds sqrt|m_pp m_qq|.  A zero diagonal
// gives a zero threshold, so [[0, 1], [1, 0]] still rotates.
constexpr float kSkipTol = 5.9604644775390625e-8f;   // 2^-24
constexpr float kPolarTol = 4e-7f;                    // as drsa_amd_polar
constexpr int kPolarMaxIter = 40;

template <int PD>
constexpr size_t syevj_lds() {
  return (2 * (size_t)PD * ns_ld<PD>() + 64 + ns_scratch_floats<PD>()) * sizeof(float);
}

// total order for the sort: NaN below every number, so every rank stays a permutation
__device__ __forceinline__ bool sorts_before(float a, int ia, float b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an == bn ? ia < ib : bn;
  return a > b || (a == b && ia < ib);
}

// wave-wide lane shifts (DPP): lane l takes lane l + 1 (shl) or l - 1 (shr); a lane without a
// source gets 0
__device__ __forceinline__ float wave_shl1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shr1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
}

// One plane rotation applied to (x, y): (c x - s y, s x + c y), each a product and one fused
// multiply-add (written out: the library is built without contraction).  The float2 forms rotate two
// rows at once on the packed fp32 pipe.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float rot_a(float c, float s, float x, float y) { return __builtin_fmaf(c, x, -(s * y)); }
__device__ __forceinline__ float rot_b(float c, float s, float x, float y) { return __builtin_fmaf(s, x, c * y); }
__device__ __forceinline__ f32x2 rot_a(float c, float s, f32x2 x, f32x2 y) {
  const f32x2 cc = {c, c};
  return __builtin_elementwise_fma(cc, x, -(s * y));
}
__device__ __forceinline__ f32x2 rot_b(float c, float s, f32x2 x, f32x2 y) {
  const f32x2 ss = {s, s};
  return __builtin_elementwise_fma(ss, x, c * y);
}

// M lives in LDS (T, the polar's row stride; the sweeps read and write its upper triangle only, so
// it stays symmetric by construction), V in registers.  m = d rounded up to even players, hm = m / 2
// pairs per step, mm = m - 1 steps per sweep; d odd: index d is a dummy player whose pair rests.
//
// Round robin: at step s pair k holds (top, bot) = ((s + k) mod mm, (s - k) mod mm) for k >= 1 and
// (mm, s) for k = 0.  From one step to the next top moves from pair k + 1 to pair k and bot from
// pair k - 1 to pair k (with bot_0 <- top_1 and top_{hm-1} <- bot_{hm-1}): a systolic ring.  So lane k
// of a PD/2-lane segment keeps its pair's two columns of V for VR rows in registers, rotates them
// and passes them on with two wave shifts per row: V never touches LDS during the sweeps.
//
// One step:
//   A  thread k < hm: the Rutishauser rotation of pair k from its own 2x2 diagonal block
//      (theta = (m_qq - m_pp) / (2 m_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), t = 1 at
//      theta = 0; p = top, q = bot), the block's new diagonal m_pp - t m_pq, m_qq + t m_pq, m_pq = 0;
//   B  one thread per pair of pairs a < b: the 2x2 block J_a^T M_ab J_b, in place (a block is read
//      and written by its own thread only); every lane: its columns of V J, then the ring shift.
template <int PD>
__global__ __launch_bounds__(fin_threads<PD>()) void syevj_kernel(const float* __restrict__ Min, int d,
                                                                  float* __restrict__ w_out, float* __restrict__ V_out,
                                                                  int* __restrict__ sweeps_out,
                                                                  int* __restrict__ status) {
  constexpr int NT = fin_threads<PD>(), LD = ns_ld<PD>(), TPC = NT / PD;
  constexpr int HMP = PD / 2, NG = NT / HMP, VR = PD / NG;       // lanes per segment, row groups, rows per thread
  constexpr int NI = ((HMP / 2) * (HMP - 1) + NT - 1) / NT;      // off-diagonal blocks per thread
  static_assert(HMP <= 64 && 64 % HMP == 0 && PD % NG == 0 && VR % 2 == 0, "a segment lies inside one wave");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* X = smem;
  float* T = X + PD * LD;
  float* red = T + PD * LD;   // 64 floats
  float* scr = red + 64;
  __shared__ float2 par[64];  // (c, s) of the step's pairs
  __shared__ float wv[128], sg[128];
  __shared__ int rnk[128];
  __shared__ int rotflag;
  const int tid = threadIdx.x;

  auto load_m = [&]() {   // the upper triangle of the input, mirrored; zero padding
    for (int e = tid; e < PD * PD; e += NT) {
      const int i = e / PD, j = e % PD;
      const bool real = i < d && j < d;
      const int a = i < j ? i : j, b = i < j ? j : i;
      T[i * LD + j] = keep_or_zero(Min[real ? (size_t)a * d + b : 0], real);
    }
  };
  load_m();
  for (int e = tid; e < PD * PD; e += NT) X[(e / PD) * LD + e % PD] = (e / PD == e % PD) ? 1.f : 0.f;

  const int m = d + (d & 1), hm = m / 2, mm = m - 1;
  // (s + k) mod mm and (s - k) mod mm for 0 <= s, k < mm: the wrapped candidate is the smaller one
  // as an unsigned number (bot_of(0, s) = s comes out by itself)
  auto top_of = [&](int k, int s) {
    const unsigned v = (unsigned)(s + k);
    return k == 0 ? mm : (int)min(v, v - (unsigned)mm);
  };
  auto bot_of = [&](int k, int s) {
    const unsigned v = (unsigned)(s - k);
    return (int)min(v, v + (unsigned)mm);
  };
  auto at = [&](int i, int j) { return min(i, j) * LD + max(i, j); };   // upper triangle

  // this thread's off-diagonal blocks (a < b), fixed for the whole run: the hm (hm - 1) / 2 blocks
  // densely numbered by folding row r onto row he - 1 - r (he = hm rounded up to even)
  int ia[NI], ib[NI];
  {
    const int he = hm + (hm & 1);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int e = tid + j * NT;
      const int r = e / (he - 1), c = e % (he - 1);
      const bool first = c < he - 1 - r;
      const int a = first ? r : he - 1 - r, b = first ? r + 1 + c : c + 1;
      const bool ok = e < (he / 2) * (he - 1) && b < hm;
      ia[j] = ok ? a : -1;
      ib[j] = ok ? b : 0;
    }
  }
  // this lane's pair k and rows g, g + NG, ...: V = I in the arrangement of step 0
  const int k = tid % HMP, g = tid / HMP;
  const bool live = k < hm;
  const int t0 = top_of(live ? k : 0, 0), b0 = bot_of(live ? k : 0, 0);
  f32x2 vt[VR / 2], vb[VR / 2];   // .x: row g + 2 j NG, .y: row g + (2 j + 1) NG
#pragma unroll
  for (int j = 0; j < VR; ++j) {
    vt[j / 2][j % 2] = (live && g + j * NG == t0) ? 1.f : 0.f;
    vb[j / 2][j % 2] = (live && g + j * NG == b0) ? 1.f : 0.f;
  }

  int sweeps = 0, rotated = 0;
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    __syncthreads();   // T complete; the previous sweep's rotflag read
    if (tid == 0) rotflag = 0;
    const float maxdiag = block_max<NT>(tid < d ? fabsf(T[tid * LD + tid]) : 0.f, red);
    const float thr = kSkipTol * maxdiag;
    for (int step = 0; step < mm; ++step) {
      if (tid < hm) {
        const int p = top_of(tid, step), q = bot_of(tid, step);
        float c = 1.f, s = 0.f;
        if (p < d && q < d) {
          const float mpq = T[at(p, q)], mpp = T[p * LD + p], mqq = T[q * LD + q];
          if (!(fabsf(mpq) <= thr)) {
            const float theta = (mqq - mpp) / (2.f * mpq);
            float t = (theta < 0.f ? -1.f : 1.f) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
            if (theta == 0.f) t = 1.f;
            c = 1.f / sqrtf(t * t + 1.f);
            s = t * c;
            T[p * LD + p] = mpp - t * mpq;
            T[q * LD + q] = mqq + t * mpq;
            T[at(p, q)] = 0.f;
            rotflag = 1;
          }
        }
        par[tid] = make_float2(c, s);
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        if (ia[j] >= 0) {
          const float2 ra = par[ia[j]], rb = par[ib[j]];
          if (!(ra.y == 0.f && rb.y == 0.f)) {   // s == 0: the identity (c == 1)
            const float ca = ra.x, sa = ra.y, cb = rb.x, sb = rb.y;
            const int pa = top_of(ia[j], step), qa = bot_of(ia[j], step);
            const int pb = top_of(ib[j], step), qb = bot_of(ib[j], step);
            const int e00 = at(pa, pb), e01 = at(pa, qb), e10 = at(qa, pb), e11 = at(qa, qb);
            const float x00 = T[e00], x01 = T[e01], x10 = T[e10], x11 = T[e11];
            const float y00 = rot_a(cb, sb, x00, x01), y01 = rot_b(cb, sb, x00, x01);
            const float y10 = rot_a(cb, sb, x10, x11), y11 = rot_b(cb, sb, x10, x11);
            T[e00] = rot_a(ca, sa, y00, y10);
            T[e10] = rot_b(ca, sa, y00, y10);
            T[e01] = rot_a(ca, sa, y01, y11);
            T[e11] = rot_b(ca, sa, y01, y11);
          }
        }
      }
      {
        const float2 rk = par[live ? k : 0];
#pragma unroll
        for (int j = 0; j < VR / 2; ++j) {   // two rows per packed operation
          const f32x2 nt = rot_a(rk.x, rk.y, vt[j], vb[j]), nb = rot_b(rk.x, rk.y, vt[j], vb[j]);
          vt[j] = nt;
          vb[j] = nb;
          if (hm > 1) {   // the ring shift to the next step's arrangement
            const f32x2 st = {wave_shl1(nt.x), wave_shl1(nt.y)}, sb = {wave_shr1(nb.x), wave_shr1(nb.y)};
            vt[j] = k == 0 ? nt : (k == hm - 1 ? nb : st);
            vb[j] = k == 0 ? st : sb;
          }
        }
      }
      __syncthreads();
    }
    sweeps = sweep + 1;
    rotated = rotflag;
    if (!rotated) break;   // uniform: read behind the step's last barrier
  }
  // whole sweeps only: the registers are back in the arrangement of step 0.  X: V, embedded in the
  // identity (rows and columns >= d are never rotated)
  if (live) {
#pragma unroll
    for (int j = 0; j < VR; ++j) {
      X[(g + j * NG) * LD + t0] = vt[j / 2][j % 2];
      X[(g + j * NG) * LD + b0] = vb[j / 2][j % 2];
    }
  }

  // V <- polar(V): the drift of ~d/2 rotations per column per sweep goes; X may move to scr
  polar_run<PD>(X, T, red, scr, kPolarTol, kPolarMaxIter);
  load_m();            // T: the original M again (the polar used it as scratch)
  __syncthreads();

  // w_k = v_k^T M v_k in double: TPC threads per column, rows part, part + TPC, ...; fixed-order sum
  {
    const int k = tid / TPC, part = tid % TPC;
    double acc = 0.0;
    for (int i = part; i < d; i += TPC) {
      double y = 0.0;
      for (int j = 0; j < d; ++j) y += (double)T[i * LD + j] * (double)X[j * LD + k];
      acc += (double)X[i * LD + k] * y;
    }
    for (int mk = 1; mk < TPC; mk <<= 1) acc += __shfl_xor(acc, mk, 64);
    if (part == 0 && k < d) wv[k] = (float)acc;
  }
  __syncthreads();
  if (tid < d) {
    const float wk = wv[tid];
    int r = 0;
    for (int j = 0; j < d; ++j) r += (j != tid && sorts_before(wv[j], j, wk, tid)) ? 1 : 0;
    rnk[tid] = r;
    float best = -1.f;
    int bi = 0;
    for (int i = 0; i < d; ++i) {
      const float a = fabsf(X[i * LD + tid]);
      if (a > best) {
        best = a;
        bi = i;
      }
    }
    sg[tid] = X[bi * LD + tid] < 0.f ? -1.f : 1.f;
    w_out[r] = wk;
  }
  __syncthreads();
  for (int e = tid; e < d * d; e += NT) {
    const int i = e / d, k = e % d;
    V_out[(size_t)i * d + rnk[k]] = sg[k] * X[i * LD + k];
  }
  if (tid == 0) {
    if (sweeps_out) *sweeps_out = sweeps;
    status[0] = sweeps;
    status[1] = rotated ? 0 : 1;   // 1: the last sweep made no rotation
    status[2] = 0;
    status[3] = 0;
  }
}

template <int V>
using Int = std::integral_constant<int, V>;

template <class F>
int with_pd(int PD, F&& f) {
  switch (PD) {
    case 32: return f(Int<32>{});
    case 64: return f(Int<64>{});
    case 128: return f(Int<128>{});
  }
  drsa::set_error("prca: no kernel for padded size %d", PD);
  return DRSA_EUNSUPPORTED;
}

constexpr size_t kSyevjStatusBytes = 4 * sizeof(int);

}  // namespace

extern "C" {

size_t drsa_amd_prca_workspace_bytes(int64_t N, int d) {
  if (N <= 0 || d <= 0 || d > 128) return 0;
  const size_t DP = (size_t)padded_dim(d);
  return (size_t)leaves(N) * DP * DP * sizeof(float);
}

int drsa_amd_prca_partial(const float* A, const float* C, int64_t N, int d, float* slab, void* ws, size_t ws_bytes,
                          void* stream) {
  DRSA_REQUIRE(A && C, "prca_partial: null pointer (A or C)");
  DRSA_REQUIRE(slab, "prca_partial: null pointer (slab)");
  DRSA_REQUIRE(N > 0, "prca_partial: N=%lld must be positive", (long long)N);
  DRSA_REQUIRE(d > 0, "prca_partial: d=%d must be positive", d);
  if (d > 128) {
    drsa::set_error("prca_partial: unsupported d=%d (1..128)", d);
    return DRSA_EUNSUPPORTED;
  }
  const size_t need = drsa_amd_prca_workspace_bytes(N, d);
  DRSA_REQUIRE(ws, "prca_partial: null pointer (ws)");
  if (ws_bytes < need) {
    drsa::set_error("prca_partial: ws_bytes=%zu is short of the %zu bytes drsa_amd_prca_workspace_bytes gives", ws_bytes,
                    need);
    return DRSA_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int L = leaves(N), DP = padded_dim(d);
  const int64_t R = row_blocks(N);
  float* leaf_slabs = (float*)ws;
  const bool vec = d % 4 == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)C % 16) == 0;
  int rc = with_pd(DP, [&](auto dp) -> int {
    constexpr int P = decltype(dp)::value;
    using Cfg = CovCfg<P>;
    if (vec) {
      DRSA_SMEM((prca_partial_kernel<P, true>), Cfg::lds_bytes);
      hipLaunchKernelGGL((prca_partial_kernel<P, true>), dim3(L), dim3(Cfg::NT), Cfg::lds_bytes, s, A, C, N, d, R, L,
                         leaf_slabs);
    } else {
      DRSA_SMEM((prca_partial_kernel<P, false>), Cfg::lds_bytes);
      hipLaunchKernelGGL((prca_partial_kernel<P, false>), dim3(L), dim3(Cfg::NT), Cfg::lds_bytes, s, A, C, N, d, R, L,
                         leaf_slabs);
    }
    DRSA_LAUNCH_CHECK();
    return DRSA_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(prca_reduce_kernel, dim3((d * d + 63) / 64), dim3(256), 0, s, leaf_slabs, L, DP, d, slab);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

int drsa_amd_prca_finish(const float* slab, int64_t N_total, int d, float* M_out, void* stream) {
  DRSA_REQUIRE(slab && M_out, "prca_finish: null pointer (slab or M_out)");
  DRSA_REQUIRE(N_total > 0, "prca_finish: N_total=%lld must be positive", (long long)N_total);
  DRSA_REQUIRE(d > 0, "prca_finish: d=%d must be positive", d);
  if (d > 128) {
    drsa::set_error("prca_finish: unsupported d=%d (1..128)", d);
    return DRSA_EUNSUPPORTED;
  }
  const float inv2n = (float)(1.0 / (2.0 * (double)N_total));
  hipLaunchKernelGGL(prca_finish_kernel, dim3((d * d + 255) / 256), dim3(256), 0, (hipStream_t)stream, slab, d, inv2n,
                     M_out);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

size_t drsa_amd_syevj_workspace_bytes(int d) { return (d <= 0 || d > 128) ? 0 : kSyevjStatusBytes; }

int drsa_amd_syevj(const float* M, int d, float* w_out, float* V_out, int* sweeps_out, void* ws, size_t ws_bytes,
                   void* stream) {
  DRSA_REQUIRE(M, "syevj: null pointer (M)");
  DRSA_REQUIRE(w_out && V_out, "syevj: null pointer (w_out or V_out)");
  DRSA_REQUIRE(d > 0, "syevj: d=%d must be positive", d);
  if (d > 128) {
    drsa::set_error("syevj: unsupported d=%d (1..128)", d);
    return DRSA_EUNSUPPORTED;
  }
  DRSA_REQUIRE(ws, "syevj: null pointer (ws)");
  if (ws_bytes < kSyevjStatusBytes) {
    drsa::set_error("syevj: ws_bytes=%zu is short of the %zu bytes drsa_amd_syevj_workspace_bytes gives", ws_bytes,
                    kSyevjStatusBytes);
    return DRSA_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  return with_pd(padded_dim(d), [&](auto dp) -> int {
    constexpr int PD = decltype(dp)::value;
    const size_t lds = syevj_lds<PD>();
    DRSA_SMEM(syevj_kernel<PD>, lds);
    hipLaunchKernelGGL(syevj_kernel<PD>, dim3(1), dim3(fin_threads<PD>()), lds, s, M, d, w_out, V_out, sweeps_out,
                       (int*)ws);
    DRSA_LAUNCH_CHECK();
    return DRSA_OK;
  });
}

}  // extern "C"
