// DRSA step: the cooperative finish at DP = 128 (the polar split over eight workgroups).
#pragma once
#include "common.h"
#include "polar_ns.h"
#include "drsa_geom.h"
#include "drsa_finish.h"

namespace {

// ---------------------------------------------------------------------------
// Cooperative finish at DP = 128 (drsa_run / run_multi, the C5 shapes): the polar's two 128^3
// products per Newton-Schulz iteration split over kCoopWG = 8 workgroups on as many CUs, workgroup j
// owning the 16 columns [16 j, 16 j + 16) of X.  Per iteration workgroup j forms P_j = X^T X[:, j]
// (8 16x16 tiles, one wave each, two per SIMD), T_j = 1.5 I - 0.5 P_j with its max |P_j - I|, and
// X'[:, j] = X T_j (8 tiles); the new
// column blocks and the error maxima are exchanged through the workspace (one hand-off per
// iteration: agent-scope stores, a ticket counter, agent-scope loads), so every workgroup holds
// the whole X' for the next P.  Bit-identical to drsa_finish_kernel's single-workgroup polar_ns:
//   * every P / X T entry is the same full-k fp32 fma chain (k ascending from +0: the 32x32x2 MFMA
//     there, 16x16x4 here, both exact chains; P's lower tiles there are mirrored from the upper
//     ones, here computed directly: x_k y_k = y_k x_k exactly);
//   * tr(P) from P's diagonal (each workgroup hands its diagonal tile's 32 entries over), folded in
//     the same order; the inf-norm row sums as column sums of workgroup j's block (P is exactly
//     symmetric), in the same order; maxima are order-free;
//   * the X T of an iteration whose error stops the loop is computed speculatively (the error is
//     exchanged with its result) and dropped, so the returned X is the one polar_ns returns.
// The workgroups spin on each other: the launch needs kCoopWG co-resident workgroups (one per CU,
// 141 KB of LDS each), which the callers guarantee by launching nothing else that waits on them.
// Failure is loud, never a hang and never silent: a spin that outlives both the wall-clock budget
// (100 ms) and kCoopMinPolls polls (so a queue preempted mid-spin, whose wall clock jumps, still
// polls ~20 ms after it resumes) gives up, sets the workspace's sticky status word, and poisons
// U_out and f with NaN; every later finish of the run sees the word at its start and skips straight
// to the poison (no further spinning, no diverged ticket to wait on).  drsa_amd_drsa_run /
// _run_multi read the word back and return DRSA_ETIMEOUT; drsa_amd_drsa_coop_status reads it for a
// run the caller captured into its own graph.  coop_reset clears ticket and status per run.
// ---------------------------------------------------------------------------
constexpr int kCoopWG = 8;
constexpr int kCoopBW = 128 / kCoopWG;   // columns per workgroup (16x16x4 MFMA tiles)
constexpr long long kCoopSpinTicks = 10000000;   // s_memrealtime runs at 100 MHz: 100 ms
constexpr int kCoopMinPolls = 20000;             // >= ~20 ms of polling (one sc1 load + s_sleep each)

// diagnostic build (-DDRSA_COOP_STAMP, scripts/probe_coop.py): phase times of the last launch's
// workgroups, read back by drsa_amd_debug_coop_stamps; nothing in the kernel reads them
#ifdef DRSA_COOP_STAMP
__device__ unsigned long long g_coop_stamps[kCoopWG][64];
#define COOP_STAMP(slot) do { if (threadIdx.x == 0 && (slot) < 64) g_coop_stamps[blockIdx.x][(slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define COOP_STAMP(slot)
#endif

struct CoopXchg {
  float xb[2][128 * 128];        // X' by iteration parity (column block j written by workgroup j)
  float sc[2][kCoopWG][4];       // per parity and workgroup: error max, inf-norm partial
  unsigned ticket;               // hand-off counter: kCoopWG arrivals per exchange, reset per run
  unsigned status;               // sticky: 1 once any hand-off of the run timed out, reset per run
  unsigned pad[62];
};

__device__ __forceinline__ void coop_st(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float coop_ld(const float* p) {
  return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every thread calls after its agent-scope stores; returns false if the other workgroups did not
// arrive within the spin budget (then the run's status word is set).
// Visibility without release/acquire fences (MI355X_MICROARCH.md "Valid forms besides Guideline
// 16's R1/R2" and the sc1 hand-off table's first row, which this matches cell for cell): every byte
// handed over is stored by coop_st (a relaxed agent-scope atomic store = global_store_dword sc1,
// 4 B) and read by coop_ld (global_load_dword sc1 to registers); every storing wave waits
// vmcnt(0) before the workgroup barrier; ONE lane per workgroup then signals for all its stores
// with one agent-scope atomic add on the ticket and polls it with relaxed agent-scope (sc1) loads;
// the other waves load only after the barrier that lane joins; one workgroup per CU, hipMalloc'd
// workspace.  (An agent release fence costs ~1.7 us and an acquire ~1.7 us per exchange here,
// 5 exchanges per finish, for no change in what the table guarantees.)
__device__ bool coop_exchange(unsigned* ticket, unsigned* status, int* ok_sh, long long spin_ticks,
                              int min_polls) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned target = (old / kCoopWG + 1) * kCoopWG;
    const long long t0 = wall_clock64();
    int ok = 1;
    for (int polls = 0;; ++polls) {
      const unsigned v = __hip_atomic_load(ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((int)(v - target) >= 0) break;
      if (polls >= min_polls && wall_clock64() - t0 > spin_ticks) { ok = 0; break; }
      __builtin_amdgcn_s_sleep(1);
    }
    if (!ok) __hip_atomic_store(status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *ok_sh = ok;
  }
  __syncthreads();
  return *ok_sh != 0;
}

constexpr int kCoopTLD = kCoopBW;   // T_j row stride (one column block)
constexpr size_t coop_lds_bytes() {
  return ((size_t)2 * 128 * ns_ld<128>() + (size_t)128 * kCoopTLD + 64) * sizeof(float);
}

__global__ __launch_bounds__(1024) void drsa_finish_coop_kernel(
    const float* __restrict__ gs, double n_total, int d, int K, int DKP, const float* __restrict__ U,
    float* __restrict__ U_out, float* __restrict__ f_out, int* __restrict__ step_counter, int f_stride_by_counter,
    float tol, int max_iter, CoopXchg* __restrict__ xc, long long spin_ticks, int min_polls) {
  constexpr int DP = 128, LD = ns_ld<DP>(), NT = 1024, TLD = kCoopTLD, TPR = NT / DP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* X = smem;                 // current X (full)
  float* Xn = X + DP * LD;         // X' being assembled
  float* Tj = Xn + DP * LD;        // T_j = 1.5 I - 0.5 P[:, j-block]
  float* red = Tj + DP * TLD;      // 64 floats
  __shared__ double dterm[128];
  __shared__ float cvec[128];
  __shared__ double fsh;
  __shared__ float diag[128];
  __shared__ int ok_sh;
  constexpr int BW = kCoopBW, NB = DP / BW;   // 16-row / 16-column tiles, NB = 8 per column block
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id(), j = blockIdx.x;
  const int lo = lane & 15, hi = lane >> 4;   // 16x16x4: A/B lane l -> index l & 15 at k = k0 + (l >> 4)
  const int dk = d / K;
  // a hand-off of an earlier step of this run timed out: poison this step too, without spinning
  if (tid == 0) ok_sh = __hip_atomic_load(&xc->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
  __syncthreads();
  if (!ok_sh) {
    for (int e = tid; e < DP * BW; e += NT) {
      const int i = e / BW, pc = BW * j + e % BW, kc = pc / DKP, l = pc % DKP;
      if (i < d && kc < K && l < dk) U_out[i * d + kc * dk + l] = __builtin_nanf("");
    }
    if (j == 0 && tid == 0) store_f_counted(f_out, step_counter, f_stride_by_counter, __builtin_nanf(""));
    return;   // uniform per workgroup
  }
  COOP_STAMP(0);
  const double f = finish_prologue<DP>(gs, n_total, d, K, DKP, U, X, true, dterm, cvec, &fsh);
  bool ok = true;
  COOP_STAMP(1);

  // P_j tile (ib = w) of X^T X[:, j-block] for waves 0..7: Tj[row][col - BW j] = raw P (it == 0) or
  // 1.5 I - 0.5 P with err (it > 0).  16x16 D layout: lane l, reg r -> row 4 (l >> 4) + r, col l & 15.
  auto gram_block = [&](int it, float& err) {
    __syncthreads();   // X complete
    if (w < NB) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
      for (int k0 = 0; k0 < DP; k0 += 4) {
        const int kk = k0 + hi;
        acc = mfma16(X[kk * LD + BW * w + lo], X[kk * LD + BW * j + lo], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = BW * w + 4 * hi + r;
        float v = acc[r];
        if (it > 0) {
          const bool dg = row == BW * j + lo;
          err = fmaxf(err, fabsf(v - (dg ? 1.f : 0.f)));
          v = (dg ? 1.5f : 0.f) - 0.5f * v;
        }
        Tj[row * TLD + lo] = v;
      }
    }
  };
  // X'[:, j-block] = X T_j for waves 0..7 (tile ib = w): into Xn and the exchange buffer
  auto xt_block = [&](int par) {
    __syncthreads();   // T_j complete
    if (w < NB) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
      for (int k0 = 0; k0 < DP; k0 += 4) {
        const int kk = k0 + hi;
        acc = mfma16(X[(BW * w + lo) * LD + kk], Tj[kk * TLD + lo], acc);
      }
      float* xg = xc->xb[par];
      int l = lane;
      asm volatile("" : "+v"(l));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = BW * w + 4 * (l >> 4) + r, col = BW * j + (l & 15);
        Xn[row * LD + col] = acc[r];
        coop_st(&xg[row * DP + col], acc[r]);
      }
    }
  };
  // the other workgroups' column blocks of X' (after the exchange)
  // (all loads issued before the first LDS store: one memory round trip, not 12)
  auto gather_blocks = [&](int par) {
    constexpr int NQ = (kCoopWG - 1) * BW * DP / NT;
    const float* xg = xc->xb[par];
    unsigned t = (unsigned)tid;
    asm volatile("" : "+v"(t));   // addresses per call: hoisted out of the iteration loop they spill
    float v[NQ];
    unsigned lds[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const unsigned e = t + (unsigned)q * NT;  // over the foreign blocks, BW-float runs
      const unsigned bi = e / (BW * DP), rem = e % (BW * DP);
      const unsigned blk = bi < (unsigned)j ? bi : bi + 1;
      const unsigned row = rem / BW, col = BW * blk + rem % BW;
      v[q] = coop_ld(&xg[row * DP + col]);
      lds[q] = row * LD + col;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) Xn[lds[q]] = v[q];
  };

  // ---- iteration 0: raw P_j, scaling a^2 = DP / tr(P) unless a^2 ||P||_inf >= 2.9 ----
  float err = 0.f, rowmax_all;
  gram_block(0, err);
  __syncthreads();   // Tj (raw P) complete
  COOP_STAMP(2);
  // row sums of |P| for the rows of block j, as column sums of P[:, j-block] (polar_ns's order)
  float rs = 0.f;
  if (tid < BW * TPR) {
    const int cl = tid / TPR, part = tid % TPR;
#pragma unroll
    for (int c = part; c < DP; c += TPR) rs += fabsf(Tj[c * TLD + cl]);
  }
  for (int m = 1; m < TPR; m <<= 1) rs += shfl_xor(rs, m);
  const float rmax_j = block_max<NT>(tid < BW * TPR ? rs : 0.f, red);
  // hand-off 0: block j's diagonal of P (its own diagonal tile) and its inf-norm partial
  if (tid < BW) {
    const int i = BW * j + tid;
    coop_st(&xc->xb[0][i * DP + i], Tj[i * TLD + tid]);
  }
  if (tid == 0) coop_st(&xc->sc[0][j][1], rmax_j);
  COOP_STAMP(3);
  ok = coop_exchange(&xc->ticket, &xc->status, &ok_sh, spin_ticks, min_polls);
  COOP_STAMP(4);
  {
    const float dv = coop_ld(&xc->xb[0][(tid & (DP - 1)) * (DP + 1)]);
    float rm[kCoopWG];
#pragma unroll
    for (int i = 0; i < kCoopWG; ++i) rm[i] = coop_ld(&xc->sc[0][i][1]);
    if (tid < DP) diag[tid] = dv;
    rowmax_all = rm[0];
#pragma unroll
    for (int i = 1; i < kCoopWG; ++i) rowmax_all = fmaxf(rowmax_all, rm[i]);
  }
  const float rowmax = rowmax_all;
  __syncthreads();   // diag complete
  float tr = 0.f;
  for (int i = lane; i < DP; i += 64) tr += diag[i];
  for (int m = 32; m >= 1; m >>= 1) tr += shfl_xor(tr, m);
  float a2 = (float)DP / tr;
  if (a2 * rowmax >= 2.9f) a2 = 1.f / rowmax;
  const float a = sqrtf(a2);
  for (int e = tid; e < DP * DP; e += NT) {
    const int r = e / DP, c = e % DP;
    X[r * LD + c] *= a;
  }
  for (int e = tid; e < DP * BW; e += NT) {
    const int r = e / BW, cl = e % BW;
    const float pv = Tj[r * TLD + cl] * a2;
    const bool dg = r == BW * j + cl;
    err = fmaxf(err, fabsf(pv - (dg ? 1.f : 0.f)));
    Tj[r * TLD + cl] = (dg ? 1.5f : 0.f) - 0.5f * pv;
  }
  err = block_max<NT>(err, red);
  COOP_STAMP(5);

  int it = 0;
  float err_prev = 1.f;
  for (; ok; ++it) {
    const int par = (it + 1) & 1;   // parity 0 carried iteration 0's scalars
    xt_block(par);                   // speculative: dropped below if err stops the loop
    if (tid == 0) coop_st(&xc->sc[par][j][0], err);
    COOP_STAMP(6 + 5 * it);
    ok = coop_exchange(&xc->ticket, &xc->status, &ok_sh, spin_ticks, min_polls);
    COOP_STAMP(7 + 5 * it);
    if (!ok) break;
    float ev[kCoopWG];
#pragma unroll
    for (int i = 0; i < kCoopWG; ++i) ev[i] = coop_ld(&xc->sc[par][i][0]);
    gather_blocks(par);
    float e_all = ev[0];
#pragma unroll
    for (int i = 1; i < kCoopWG; ++i) e_all = fmaxf(e_all, ev[i]);
    if (e_all < tol || it >= max_iter) break;   // X stays (polar_ns breaks before the update)
    const bool last = (float)DP * e_all < DRSA_NS_LAST || (it > 0 && err_prev < 1e-4f && e_all > 0.25f * err_prev);
    err_prev = e_all;
    float* t = X; X = Xn; Xn = t;
    if (last) { ++it; break; }
    COOP_STAMP(8 + 5 * it);
    err = 0.f;
    gram_block(it + 1, err);
    COOP_STAMP(9 + 5 * it);
    err = block_max<NT>(err, red);
    COOP_STAMP(10 + 5 * it);
  }
  __syncthreads();
  COOP_STAMP(60);
  // U_out: workgroup j writes the real entries of its padded column block
#pragma unroll
  for (int q = 0; q < DP * BW / NT; ++q) {
    const int e = tid + q * NT, i = e / BW, pc = BW * j + e % BW;
    const int kc = pc / DKP, l = pc % DKP;
    if (i < d && kc < K && l < dk) U_out[i * d + kc * dk + l] = ok ? X[i * LD + pc] : __builtin_nanf("");
  }
  if (j == 0 && tid == 0)
    store_f_counted(f_out, step_counter, f_stride_by_counter, ok ? (float)f : __builtin_nanf(""));
  COOP_STAMP(61);
}

}  // namespace
