// DRSA step: the slab reduces, the finish (f, c, polar), the fused step and the polar kernel.
#pragma once
#include "common.h"
#include "polar_ns.h"
#include "drsa_geom.h"
#include "drsa_partial.h"

namespace {

// ---------------------------------------------------------------------------
// reduce: out[e] = the left fold over leaf groups q (ascending) of G_q[e], G_q[e] = the left fold
// over the group's slabs (at most LG of them, ascending), both from +0 -- the kLeaves partition's
// fixed order (deterministic, no atomics).  LG = kLeafGroup for per-leaf slabs (drsa_partial_kernel,
// the fused step), 1 for the grouped kernel's per-group slabs: the same additions either way.
// Thread group grp of a block computes G_q for q = grp, grp + 4, ... with every slab load of its
// groups issued before the adds (the slabs were just written by every CU: one memory round trip per
// batch of loads), then one thread per element folds the G_q in order.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void reduce_grouped(const float* __restrict__ partials, int P, int LG, int ES, int E,
                                               float* __restrict__ out) {
  __shared__ float part[kMaxGroups][64];
  const int l = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + l;
  const int ng = (P + LG - 1) / LG;
  const int ec = e < E ? e : 0;
#pragma unroll
  for (int q0 = 0; q0 < kMaxGroups; q0 += 4) {
    const int qq = q0 + grp;
    if (q0 >= ng) break;                  // uniform
    float v[kLeafGroup];
#pragma unroll
    for (int i = 0; i < kLeafGroup; ++i) {
      const int p = qq * LG + i;
      const bool ok = i < LG && qq < ng && p < P;
      v[i] = partials[(size_t)(ok ? p : 0) * ES + ec];
    }
    float G = 0.f;
#pragma unroll
    for (int i = 0; i < kLeafGroup; ++i)
      if (i < LG && qq * LG + i < P) G += v[i];
    if (qq < ng) part[qq][l] = G;
  }
  __syncthreads();
  if (grp == 0 && e < E) {
    float T = 0.f;
    for (int qq = 0; qq < ng; ++qq) T += part[qq][l];
    out[e] = T;
  }
}

// The per-leaf slab reduce of drsa_run / the fused and sharded steps (LG = kLeafGroup), spread over
// the chip: RW = 256 / CW thread rows per workgroup of CW columns, each thread computing the group
// sums G_q of QPT = kMaxGroups / RW groups with all QPT * kLeafGroup slab loads issued first; the
// same additions in the same order as reduce_grouped (bit-identical), on E / CW workgroups instead of
// E / 64 (C3: 129 instead of 65 CUs, 32 loads per thread in flight instead of 8 rounds of 8;
// A/B at C3 (gpurun_out/r6e): CW 8 / 16 / 32 = 33.9 / 32.4 / 31.7 us per step).
#ifndef DRSA_REDUCE_CW
#define DRSA_REDUCE_CW 32
#endif
// (CW = 64 for the DP = 128 slabs: E / 16 = 1025 workgroups measured slower than E / 64 = 257)
template <int CW>
__global__ __launch_bounds__(256) void drsa_reduce_kernel(const float* __restrict__ partials, int P, int E, int ES,
                                                          float* __restrict__ out) {
  constexpr int RW = 256 / CW, QPT = kMaxGroups / RW;
  static_assert(kMaxGroups % RW == 0, "groups per thread");
  __shared__ float part[kMaxGroups][CW];
  const int c = threadIdx.x % CW, r = threadIdx.x / CW;
  const int e = blockIdx.x * CW + c;
  const int ng = (P + kLeafGroup - 1) / kLeafGroup;
  const int ec = e < E ? e : 0;
  float v[QPT][kLeafGroup];
#pragma unroll
  for (int j = 0; j < QPT; ++j)
#pragma unroll
    for (int i = 0; i < kLeafGroup; ++i) {
      const int p = (r + RW * j) * kLeafGroup + i;
      v[j][i] = partials[(size_t)(p < P ? p : 0) * ES + ec];
    }
#pragma unroll
  for (int j = 0; j < QPT; ++j) {
    const int qq = r + RW * j;
    float G = 0.f;
#pragma unroll
    for (int i = 0; i < kLeafGroup; ++i)
      if (qq * kLeafGroup + i < P) G += v[j][i];
    if (qq < ng) part[qq][c] = G;
  }
  __syncthreads();
  if (r == 0 && e < E) {
    float T = 0.f;
    for (int qq = 0; qq < ng; ++qq) T += part[qq][c];
    out[e] = T;
  }
}

// the polar runs at PD = max(32, DP) (32x32 MFMA tiles; a d <= 16 problem is embedded once more)
template <int DP>
constexpr int polar_dim() { return DP < 32 ? 32 : DP; }
template <int DP>
constexpr size_t finish_lds() {
  // polar_ns16 (DP <= 64): the second X buffer; polar_ns: the k-split scratch
  constexpr int PD = polar_dim<DP>();
  constexpr size_t scr = ns_scratch_floats<PD>();
  return (2 * (size_t)PD * ns_ld<PD>() + 64 + scr) * sizeof(float);
}
// the carve-up of that dynamic LDS for polar_run<PD> (which may return with X on its other buffer:
// read the result through X, never through smem)
template <int PD>
struct PolarLds {
  float *X, *T;   // [PD][ns_ld<PD>()] each
  float* red;     // 64 floats
  float* scr;     // k-split partial tiles (polar_ns)
  __device__ __forceinline__ explicit PolarLds(float* smem)
      : X(smem), T(X + PD * ns_ld<PD>()), red(T + PD * ns_ld<PD>()), scr(red + 64) {}
};

// one thread: f_out[slot] = value, slot = the step counter (advanced past it if `advance`) or 0
__device__ __forceinline__ void store_f_counted(float* __restrict__ f_out, int* __restrict__ step_counter,
                                                bool by_counter, float value, bool advance = true) {
  const int slot = by_counter ? *step_counter : 0;
  f_out[slot] = value;
  if (by_counter && advance) *step_counter = slot + 1;
}

// U_out [d, d] = the real entries of the embedded X (PD x PD, concept blocks DKP wide), all threads
template <int PD>
__device__ __forceinline__ void unembed_store(const float* X, int d, int dk, int DKP, float* __restrict__ U_out) {
  for (int e = threadIdx.x; e < d * d; e += fin_threads<PD>()) {
    const int i = e / d, j = e % d;
    U_out[e] = X[i * ns_ld<PD>() + (j / dk) * DKP + j % dk];
  }
}

// finish prologue: f = (mean_k sqrt(M_k))^2, M_k = sqrt(S_k / N) (evaluated in double from the fp32
// sums), c_k = sqrt(f) / (K N M_k^1.5), and X = embed(U + Gt diag(c)): padded rows pair with the
// padded columns through an identity block.  Returns f; X is built only when build_x.
template <int DP>
__device__ __forceinline__ double finish_prologue(const float* __restrict__ gs, double n_total, int d, int K, int DKP,
                                                  const float* __restrict__ U, float* X, bool build_x,
                                                  double* dterm, float* cvec, double* fsh) {
  constexpr int PD = polar_dim<DP>(), NT = fin_threads<PD>(), LD = ns_ld<PD>();
  constexpr int NQ = (PD * PD + NT - 1) / NT;
  const int tid = threadIdx.x;
  const int dk = d / K;
  // X's U and G entries are loaded first, so their memory latency overlaps the f / c stages
  // (loads from clamped addresses, pinned, so all of them are in flight at once: no exec branches)
  float uq[NQ], gq[NQ];
  if (build_x) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int e = tid + q * NT;
      const int ip = e / PD, jp = e % PD, kc = jp / DKP, l = jp % DKP;
      const bool real = e < PD * PD && ip < d && jp < DP && kc < K && l < dk;
      uq[q] = U[real ? (size_t)ip * d + kc * dk + l : 0];
      gq[q] = gs[real ? ip * DP + jp : 0];
    }
  }
  if (tid < K) dterm[tid] = sqrt(sqrt((double)gs[DP * DP + tid] / n_total));
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int k = 0; k < K; ++k) sum += dterm[k];
    const double mean = sum / K;
    *fsh = mean * mean;
  }
  __syncthreads();
  const double f = *fsh;
  if (tid < K) {
    const double Mk = sqrt((double)gs[DP * DP + tid] / n_total);
    cvec[tid] = (float)((Mk > 0.0) ? sqrt(f) / (K * n_total * Mk * sqrt(Mk)) : 0.0);
  }
  if (!build_x) return f;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = tid + q * NT;
    const int ip = e / PD, jp = e % PD, kc = jp / DKP, l = jp % DKP;
    const bool real = e < PD * PD && ip < d && jp < DP && kc < K && l < dk;
    const float u = uq[q], gv = gq[q];
    const float rv = keep_or_zero(u + gv * cvec[kc < K ? kc : 0], real);
    const float v = ip < d ? rv : ((jp == pad_col(ip - d, K, dk, DKP)) ? 1.f : 0.f);
    if (e < PD * PD) X[ip * LD + jp] = v;
  }
  return f;
}

// mode 0: full step (f, U_out = polar(U + G)); mode 1: objective only
template <int DP>
__device__ __forceinline__ void finish_body(const float* __restrict__ gs, double n_total, int d, int K, int DKP,
                                            const float* __restrict__ U, float* __restrict__ U_out,
                                            float* __restrict__ f_out, int* __restrict__ step_counter,
                                            int f_stride_by_counter, int mode, float tol, int max_iter,
                                            int* __restrict__ iters_out) {
  constexpr int PD = polar_dim<DP>();
  extern __shared__ __attribute__((aligned(16))) float smem[];
  PolarLds<PD> lds(smem);
  __shared__ double dterm[128];
  __shared__ float cvec[128];
  __shared__ double fsh;
  const int tid = threadIdx.x;
  const double f = finish_prologue<DP>(gs, n_total, d, K, DKP, U, lds.X, mode == 0, dterm, cvec, &fsh);
  // (the objective-only mode writes f at the counter and leaves it there)
  if (tid == 0) store_f_counted(f_out, step_counter, f_stride_by_counter, (float)f, mode == 0);
  if (mode == 1) return;
  const int it = polar_run<PD>(lds.X, lds.T, lds.red, lds.scr, tol, max_iter);
  unembed_store<PD>(lds.X, d, d / K, DKP, U_out);
  if (tid == 0 && iters_out) *iters_out = it;
}

template <int DP>
__global__ __launch_bounds__(fin_threads<polar_dim<DP>()>()) void drsa_finish_kernel(
    const float* __restrict__ gs, double n_total, int d, int K, int DKP, const float* __restrict__ U,
    float* __restrict__ U_out, float* __restrict__ f_out, int* __restrict__ step_counter, int f_stride_by_counter,
    int mode, float tol, int max_iter, int* __restrict__ iters_out) {
  finish_body<DP>(gs, n_total, d, K, DKP, U, U_out, f_out, step_counter, f_stride_by_counter, mode, tol, max_iter,
                  iters_out);
}

// ---------------------------------------------------------------------------
// batched independent problems (task-parallel DRSA grid, optsubspaces.py:17-23): one launch per
// phase for every problem of a batch that shares the padded geometry.  Problem p's partial runs
// on G workgroups (blockIdx.y = p; drsa_partial_grouped_kernel, whole leaf groups each), its reduce
// on blockIdx.y = p, its finish on workgroup p.  U ping-pongs between U_io and U_tmp by step parity.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void drsa_reduce_batched_kernel(const BatchDesc* __restrict__ bd, int E, int ES) {
  const BatchDesc& q = bd[blockIdx.y];
  if (q.m > 0) reduce_grouped(q.partials, (q.L + kLeafGroup - 1) / kLeafGroup, 1, ES, E, q.gs);
  else reduce_grouped(q.partials, q.L, kLeafGroup, ES, E, q.gs);
}

// mode 0: U_in -> U_out = polar(U_in + G c), f(U_in) -> f_traj[counter++]; mode 1: f only
template <int DP>
__global__ __launch_bounds__(fin_threads<polar_dim<DP>()>()) void drsa_finish_batched_kernel(
    const BatchDesc* __restrict__ bd, int parity, int mode, float tol, int max_iter) {
  const BatchDesc& q = bd[blockIdx.x];
  const float* U = parity ? q.U_tmp : q.U_io;
  float* U_out = parity ? q.U_io : q.U_tmp;
  finish_body<DP>(q.gs, (double)q.N, q.d, q.K, q.DKP, U, U_out, q.f_traj, q.counter, 1, mode, tol, max_iter,
                  nullptr);
}

// One fused DRSA step for DP = 64 (C3, C4): every workgroup first finishes the PREVIOUS step
// redundantly -- f and c from the reduced slab gs, X = embed(U + Gt diag(c)), the same polar -- so
// U_next never leaves the CU before its partial uses it; workgroup 0 stores U_next and f(U).  The
// first tile's A/C loads are issued before the polar and land under it; U_next goes from LDS into
// the partial's registers.  Bit-identical to drsa_finish_kernel followed by drsa_partial_kernel
// (same code, same inputs in every workgroup); one launch and the U round trip fewer per step.
template <int DP, int DKP, bool VEC>
__global__ __launch_bounds__(fin_threads<polar_dim<DP>()>()) void drsa_fused_step_kernel(
    const float* __restrict__ A, const float* __restrict__ C, int64_t N, int d, int K, int dk,
    const float* __restrict__ gs, double n_total, const float* __restrict__ U, float* __restrict__ U_out,
    float* __restrict__ f_out, int* __restrict__ step_counter, float* __restrict__ partials, int64_t rb_total,
    float tol, int max_iter) {
  constexpr int PD = polar_dim<DP>(), LD = ns_ld<PD>();
  static_assert(PCfg<DP, DKP>::NT == fin_threads<PD>(), "fused step: the partial and the polar use one thread count");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  PolarLds<PD> lds(smem);
  __shared__ double dterm[128];
  __shared__ float cvec[128];
  __shared__ double fsh;
  auto pre = [&] {
    const double f = finish_prologue<DP>(gs, n_total, d, K, DKP, U, lds.X, true, dterm, cvec, &fsh);
    polar_run<PD>(lds.X, lds.T, lds.red, lds.scr, tol, max_iter);   // ends with a barrier: X complete
    if (blockIdx.x == 0) {
      unembed_store<PD>(lds.X, d, dk, DKP, U_out);
      if (threadIdx.x == 0) store_f_counted(f_out, step_counter, step_counter != nullptr, (float)f);   // no counter: f_out[0]
    }
  };
  partial_core<DP, DKP, 0, VEC>(
      A, C, N, d, K, dk, partials, rb_total, pre, [&](int k, int, int jp) { return lds.X[k * LD + jp]; },
      [] { __syncthreads(); }, (int)gridDim.x);   // mid: every wave has read U from X before the tile store overwrites it
}

template <int DP, int DKP>
constexpr size_t fused_lds() {
  return PCfg<DP, DKP>::lds_bytes > finish_lds<DP>() ? PCfg<DP, DKP>::lds_bytes : finish_lds<DP>();
}

// polar only (orthogonalize API): any d <= 128, embedded as diag(V, I) in DP = pow2ceil(max(32, d))
template <int DP>
__global__ __launch_bounds__(fin_threads<DP>()) void polar_kernel(const float* __restrict__ V, int d,
                                                                  float* __restrict__ U_out, float tol, int max_iter,
                                                                  int* iters_out) {
  constexpr int NT = fin_threads<DP>(), LD = ns_ld<DP>();
  extern __shared__ __attribute__((aligned(16))) float smem[];
  PolarLds<DP> lds(smem);
#pragma unroll
  for (int q = 0; q < (DP * DP + NT - 1) / NT; ++q) {
    const int e = threadIdx.x + q * NT;
    const int i = e / DP, j = e % DP;
    const bool real = e < DP * DP && i < d && j < d;
    const float v = keep_or_zero(V[real ? (size_t)i * d + j : 0], real);
    if (e < DP * DP) lds.X[i * LD + j] = (i < d && j < d) ? v : (i == j ? 1.f : 0.f);
  }
  const int it = polar_run<DP>(lds.X, lds.T, lds.red, lds.scr, tol, max_iter);
  for (int e = threadIdx.x; e < d * d; e += NT) U_out[e] = lds.X[(e / d) * LD + e % d];
  if (iters_out && threadIdx.x == 0) *iters_out = it;
}

}  // namespace
