// Polar factor by Newton-Schulz in one workgroup (shared by drsa_finish.h, drsa_coop.h and
// scripts/probe_ns.hip).
//   X0 = a V (a from the first Gram matrix: sqrt(DP / tr) unless that overshoots the inf-norm);
//   P = X^T X (upper 32x32 block triangle, mirrored), T = 1.5 I - 0.5 P, X <- X T until max|P - I| < tol
//   or until the next update provably lands there / rounding has become the floor.
// fp32 MFMA 32x32x2 (exact f32 fma chains): per MFMA 2 LDS operand reads for 2048 MACs, and its
// dependent-accumulator latency equals its issue time, so one wave per SIMD keeps the pipe busy.
#pragma once
#include "common.h"

#ifndef DRSA_NS16
#define DRSA_NS16 1
#endif
#ifndef DRSA_NS_STAMP
#define DRSA_NS_STAMP(slot)
#endif

namespace {

template <int DP>
constexpr int fin_threads() { return DP >= 64 ? 1024 : 256; }
// row stride == 2 (mod 64): the row-direction operand reads (X in X T) hit 64 distinct banks, the
// column-direction ones 2-way at worst
template <int DP>
constexpr int ns_ld() { return DP + 2; }

// wave max in lane 63 by DPP row shifts and row broadcasts (a max is order-free, so this equals the
// xor-shuffle tree it replaces bit for bit; 6 dependent VALU ops instead of 6 ds_bpermute round trips)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max_step(float v) {
  const int o = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
  return fmaxf(v, __int_as_float(o));
}
__device__ __forceinline__ float wave_max63(float v) {
  v = dpp_max_step<0x111, 0xf>(v);   // row_shr:1
  v = dpp_max_step<0x112, 0xf>(v);   // row_shr:2
  v = dpp_max_step<0x114, 0xf>(v);   // row_shr:4
  v = dpp_max_step<0x118, 0xf>(v);   // row_shr:8   -> lane 15 of each row: the row's max
  v = dpp_max_step<0x142, 0xa>(v);   // row_bcast:15 (rows 1, 3)
  v = dpp_max_step<0x143, 0xc>(v);   // row_bcast:31 (rows 2, 3) -> lane 63: the wave's max
  return v;
}

// single-barrier block max: red must be a slot nobody reads or writes between two calls that are
// separated by at least one other __syncthreads (the per-iteration error uses alternating slots)
template <int NT>
__device__ float block_max1(float v, float* red) {
  v = wave_max63(v);
  if (lane_id() == 63) red[wave_id()] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) r = fmaxf(r, red[i]);
  return r;
}

template <int NT>
__device__ float block_max(float v, float* red) {
  v = wave_max63(v);
  __syncthreads();
  if (lane_id() == 63) red[wave_id()] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) r = fmaxf(r, red[i]);
  return r;
}

// 32x32x2 f32 MFMA tile accumulate: C/D lane l, reg r -> row (r&3) + 8(r>>2) + 4(l>>5), col l&31
__device__ __forceinline__ int t32_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// k-split of the 32x32 tiles: below DP = 128 there are too few tiles to keep 16 waves busy, so each
// tile's k range is split over KS waves and the partial tiles are summed in a fixed order (kq
// ascending) through LDS scratch.
template <int DP>
constexpr int ns_ks() { return DP >= 128 ? 1 : 4; }
// scratch after X, T and the 64-float reduction slots: the k-split partial tiles of polar_ns, or
// the second X buffer of polar_ns16 (DP <= 64)
template <int DP>
constexpr size_t ns_scratch_floats() {
  return (DP <= 64 && DRSA_NS16) ? (size_t)DP * ns_ld<DP>()
         : ns_ks<DP>() == 1      ? 0
                                 : (size_t)(DP / 32) * (DP / 32) * ns_ks<DP>() * 1024;
}

// (So the caller's tol does not bound the returned U after such a last update; the bound below does,
// and the tests gate the result's orthogonality directly.)
// Stop after the update once DP * err (a bound on the spectral error e = |1 - sigma^2|; loose by
// ~sqrt(DP) for the spread-out errors of V = U + G) is below this: the update then leaves at most
// 0.75 e^2 (1 + e/3) < 7.6e-5.  1e-2 instead of 1e-4 saves one Newton-Schulz iteration per step
// at C3 (5 -> 4) and at d = 128 (4 -> 3): 0.0391 -> 0.0358 ms (C3), 0.166 -> 0.155 ms (C5 joint),
// with the 2 000-step C3 and 5 000-step C5 trajectories still inside their 1e-4 gates.
// The second "last" clause of the loops below (err_prev < 1e-4 and err > err_prev / 4: rounding is the
// floor) is unreachable at DP <= 64 with this value: err_prev < 1e-4 already gives DP * err_prev <
// 6.4e-3 < 1e-2, so the loop ended one iteration earlier.  At DP = 128 it can fire only for err_prev
// in [1e-2 / 128, 1e-4) = [7.8e-5, 1e-4).  No case of tests/polar_ref.py's tables reaches it
// (tests/test_polar_cases_cpu.py asserts that of the float32 model).
#ifndef DRSA_NS_LAST
#define DRSA_NS_LAST 1e-2f
#endif
template <int DP>
__device__ __forceinline__ int polar_ns(float* X, float* T, float* red, float* scr, float tol, int max_iter) {
  constexpr int NT = fin_threads<DP>(), LD = ns_ld<DP>(), NB = DP / 32, NWV = NT / 64, KS = ns_ks<DP>();
  constexpr int NSYM = NB * (NB + 1) / 2, NFULL = NB * NB;
  constexpr int KR = DP / KS;                       // k range per task
  constexpr int TPR = NT / DP;   // threads per row in the inf-norm pass (8 or 16)
  static_assert(DP >= 32, "polar_ns: DP >= 32 (callers embed smaller problems)");
  static_assert(KS == 1 || (NSYM * KS <= NWV && NFULL * KS <= NWV), "one k-split task per wave");
  constexpr int NTW = (NFULL * KS + NWV - 1) / NWV;
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int lo = lane & 31, hi = lane >> 5;
  auto sym_tile = [](int t, int& ib, int& jb) {
    ib = 0;
    int rem = t;
    while (rem >= NB - ib) { rem -= NB - ib; ++ib; }
    jb = ib + rem;
  };
  // P element epilogue: raw (it == 0, scaling follows) or T = 1.5 I - 0.5 P with the error
  auto put_p = [&](int it, int row, int col, float v, float& err) {
    if (it > 0) {
      const bool dg = row == col;
      err = fmaxf(err, fabsf(v - (dg ? 1.f : 0.f)));
      v = (dg ? 1.5f : 0.f) - 0.5f * v;
    }
    T[row * LD + col] = v;
    if (row / 32 != col / 32) T[col * LD + row] = v;   // X^T X is exactly symmetric (products commute)
  };
  int it = 0;
  float err_prev = 1.f;
  for (;; ++it) {
    __syncthreads();   // X complete
    DRSA_NS_STAMP(4 * it + 0);
    // ---- P = X^T X on the upper block triangle ----
    float err = 0.f;
    for (int t = w; t < NSYM * KS; t += NWV) {
      int ib, jb;
      sym_tile(t / KS, ib, jb);
      const int kq = t % KS;
      f32x16 acc = {};
#pragma unroll 8
      for (int k0 = kq * KR; k0 < (kq + 1) * KR; k0 += 2) {
        const int kk = k0 + hi;
        acc = mfma32(X[kk * LD + 32 * ib + lo], X[kk * LD + 32 * jb + lo], acc);
      }
      if constexpr (KS == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) put_p(it, 32 * ib + t32_row(r, hi), 32 * jb + lo, acc[r], err);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) scr[(size_t)t * 1024 + r * 64 + lane] = acc[r];
      }
    }
    if constexpr (KS > 1) {
      __syncthreads();
      for (int e = tid; e < NSYM * 1024; e += NT) {
        const int tt = e / 1024, r = (e / 64) % 16, ln = e % 64;
        int ib, jb;
        sym_tile(tt, ib, jb);
        float v = 0.f;
#pragma unroll
        for (int kq = 0; kq < KS; ++kq) v += scr[(size_t)(tt * KS + kq) * 1024 + r * 64 + ln];
        put_p(it, 32 * ib + t32_row(r, ln >> 5), 32 * jb + (ln & 31), v, err);
      }
    }
    if (it == 0) {
      __syncthreads();
      DRSA_NS_STAMP(4 * it + 1);
      // scaling a^2 = DP / tr(P) if a^2 ||P||_inf < 2.9 else 1 / ||P||_inf (fixed-order sums)
      float tr = 0.f;
      for (int i = lane; i < DP; i += 64) tr += T[i * LD + i];
      for (int m = 32; m >= 1; m >>= 1) tr += shfl_xor(tr, m);   // every wave gets the same value
      const int row = tid / TPR, part = tid % TPR;
      float rs = 0.f;
      for (int c = part; c < DP; c += TPR) rs += fabsf(T[row * LD + c]);
      for (int m = 1; m < TPR; m <<= 1) rs += shfl_xor(rs, m);
      const float rowmax = block_max<NT>(rs, red);
      float a2 = (float)DP / tr;
      if (a2 * rowmax >= 2.9f) a2 = 1.f / rowmax;
      const float a = sqrtf(a2);
      for (int e = tid; e < DP * DP; e += NT) {
        const int r = e / DP, c = e % DP;
        X[r * LD + c] *= a;
        const float pv = T[r * LD + c] * a2;
        err = fmaxf(err, fabsf(pv - (r == c ? 1.f : 0.f)));
        T[r * LD + c] = (r == c ? 1.5f : 0.f) - 0.5f * pv;
      }
    }
    err = block_max1<NT>(err, red + 32 + 16 * (it & 1));
    DRSA_NS_STAMP(4 * it + 2);
    if (err < tol || it >= max_iter) break;
    // Stop after this update when it lands within 0.75 DRSA_NS_LAST^2 of orthogonal (see above), or
    // when fp32 rounding has become the floor: from a spectral error e = |1 - sigma^2| one iteration leaves 0.75 e^2 (1 + e/3),
    // and e <= DP * err (entrywise max of the symmetric P - I); a quadratic step from err_prev <
    // 1e-4 would be far below err_prev / 4, so a smaller drop is rounding noise, not convergence.
    const bool last = (float)DP * err < DRSA_NS_LAST || (it > 0 && err_prev < 1e-4f && err > 0.25f * err_prev);
    err_prev = err;
    // ---- X <- X T (all reads before any write) ----
    f32x16 acc[NTW];
#pragma unroll
    for (int q = 0; q < NTW; ++q) acc[q] = f32x16{};
#pragma unroll 4
    for (int kr = 0; kr < KR; kr += 2) {
#pragma unroll
      for (int q = 0; q < NTW; ++q) {
        const int t = w + NWV * q;
        if (t < NFULL * KS) {
          const int tile = t / KS, kq = t % KS, ib = tile / NB, jb = tile % NB;
          const int kk = kq * KR + kr + hi;
          acc[q] = mfma32(X[(32 * ib + lo) * LD + kk], T[kk * LD + 32 * jb + lo], acc[q]);
        }
      }
    }
    if constexpr (KS > 1) {
#pragma unroll
      for (int q = 0; q < NTW; ++q) {
        const int t = w + NWV * q;
        if (t < NFULL * KS)
#pragma unroll
          for (int r = 0; r < 16; ++r) scr[(size_t)t * 1024 + r * 64 + lane] = acc[q][r];
      }
    }
    __syncthreads();
    DRSA_NS_STAMP(4 * it + 3);
    if constexpr (KS == 1) {
#pragma unroll
      for (int q = 0; q < NTW; ++q) {
        const int t = w + NWV * q;
        if (t < NFULL) {
          const int ib = t / NB, jb = t % NB;
#pragma unroll
          for (int r = 0; r < 16; ++r) X[(32 * ib + t32_row(r, hi)) * LD + 32 * jb + lo] = acc[q][r];
        }
      }
    } else {
      for (int e = tid; e < NFULL * 1024; e += NT) {
        const int tt = e / 1024, r = (e / 64) % 16, ln = e % 64, ib = tt / NB, jb = tt % NB;
        float v = 0.f;
#pragma unroll
        for (int kq = 0; kq < KS; ++kq) v += scr[(size_t)(tt * KS + kq) * 1024 + r * 64 + ln];
        X[(32 * ib + t32_row(r, ln >> 5)) * LD + 32 * jb + (ln & 31)] = v;
      }
    }
    if (last) { ++it; break; }
  }
  __syncthreads();
  return it;
}

// DP <= 64: the same iteration on 16x16x4 MFMA tiles, one output tile per wave (no k-split, so no
// LDS scratch round trip and no extra barrier per product).  16x16 D layout: lane l, reg r ->
// row 4(l>>4) + r, col l&15; A/B operands: lane l holds k = k0 + (l>>4), row/col l&15.
// X is double-buffered (X, Xn swap per update): X T goes straight into the buffer nobody reads in
// this iteration, so an iteration has two barriers (X complete; T and the error complete) instead of
// three; on return X points at the buffer holding the result.  Same arithmetic, same bits.
template <int DP>
__device__ __forceinline__ int polar_ns16(float*& X, float* Xn, float* T, float* red, float tol, int max_iter) {
  constexpr int NT = fin_threads<DP>(), LD = ns_ld<DP>(), NB = DP / 16, NWV = NT / 64;
  constexpr int NSYM = NB * (NB + 1) / 2, NFULL = NB * NB;
  constexpr int TPR = NT / DP;
  static_assert(DP == 32 || DP == 64, "polar_ns16: DP 32 or 64");
  static_assert(NFULL <= NWV && NSYM <= NWV, "one tile per wave");
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int lo = lane & 15, hi = lane >> 4;
  int sib = 0, sjb = 0;            // this wave's upper-triangle tile of P
  {
    int rem = w;
    while (sib < NB && rem >= NB - sib) { rem -= NB - sib; ++sib; }
    sjb = sib + rem;
  }
  const int fib = w / NB, fjb = w % NB;   // this wave's tile of X T
  auto put_p = [&](int it, int row, int col, float v, float& err) {
    if (it > 0) {
      const bool dg = row == col;
      err = fmaxf(err, fabsf(v - (dg ? 1.f : 0.f)));
      v = (dg ? 1.5f : 0.f) - 0.5f * v;
    }
    T[row * LD + col] = v;
    if (row / 16 != col / 16) T[col * LD + row] = v;
  };
  int it = 0;
  float err_prev = 1.f;
  for (;; ++it) {
    __syncthreads();   // X complete
    DRSA_NS_STAMP(4 * it + 0);
    float err = 0.f;
    if (w < NSYM) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k0 = 0; k0 < DP; k0 += 4) {
        const int k = k0 + hi;
        acc = mfma16(X[k * LD + 16 * sib + lo], X[k * LD + 16 * sjb + lo], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) put_p(it, 16 * sib + 4 * hi + r, 16 * sjb + lo, acc[r], err);
    }
    if (it == 0) {
      __syncthreads();
      DRSA_NS_STAMP(4 * it + 1);
      float tr = 0.f;
      for (int i = lane; i < DP; i += 64) tr += T[i * LD + i];
      for (int m = 32; m >= 1; m >>= 1) tr += shfl_xor(tr, m);
      const int row = tid / TPR, part = tid % TPR;
      float rs = 0.f;
      for (int c = part; c < DP; c += TPR) rs += fabsf(T[row * LD + c]);
      for (int m = 1; m < TPR; m <<= 1) rs += shfl_xor(rs, m);
      const float rowmax = block_max<NT>(rs, red);
      float a2 = (float)DP / tr;
      if (a2 * rowmax >= 2.9f) a2 = 1.f / rowmax;
      const float a = sqrtf(a2);
      for (int e = tid; e < DP * DP; e += NT) {
        const int r = e / DP, c = e % DP;
        X[r * LD + c] *= a;
        const float pv = T[r * LD + c] * a2;
        err = fmaxf(err, fabsf(pv - (r == c ? 1.f : 0.f)));
        T[r * LD + c] = (r == c ? 1.5f : 0.f) - 0.5f * pv;
      }
    }
    err = block_max1<NT>(err, red + 32 + 16 * (it & 1));
    DRSA_NS_STAMP(4 * it + 2);
    if (err < tol || it >= max_iter) break;
    const bool last = (float)DP * err < DRSA_NS_LAST || (it > 0 && err_prev < 1e-4f && err > 0.25f * err_prev);
    err_prev = err;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (w < NFULL) {
#pragma unroll
      for (int k0 = 0; k0 < DP; k0 += 4) {
        const int k = k0 + hi;
        acc = mfma16(X[(16 * fib + lo) * LD + k], T[k * LD + 16 * fjb + lo], acc);
      }
      // no barrier: Xn was last read in the previous iteration, before this one's first barrier
#pragma unroll
      for (int r = 0; r < 4; ++r) Xn[(16 * fib + 4 * hi + r) * LD + 16 * fjb + lo] = acc[r];
    }
    DRSA_NS_STAMP(4 * it + 3);
    {
      float* t = X;
      X = Xn;
      Xn = t;
    }
    if (last) { ++it; break; }
  }
  __syncthreads();
  return it;
}

// the production polar: 16x16 tiles below DP = 128, 32x32 (k-split where needed) otherwise
// (DP <= 64: scr holds the second X buffer, ns_scratch_floats; X may come back pointing at it)
template <int DP>
__device__ __forceinline__ int polar_run(float*& X, float* T, float* red, float* scr, float tol, int max_iter) {
  if constexpr (DP <= 64 && DRSA_NS16) return polar_ns16<DP>(X, scr, T, red, tol, max_iter);
  else return polar_ns<DP>(X, T, red, scr, tol, max_iter);
}

}  // namespace
