// DRSA step: the padded geometry of a problem (d, K) and the leaf partition of its rows.
#pragma once
#include "common.h"

namespace {

inline int pow2ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

struct Geom {
  int d, K, dk;     // real problem
  int DKp, DP, Kp;  // padded concept width, padded size, concept slots (K real + phantom)
  bool ok;
};

Geom geom(int d, int K) {
  Geom g{d, K, 0, 0, 0, 0, false};
  if (d <= 0 || d > 128 || K <= 0 || d % K) return g;
  g.dk = d / K;
  g.DKp = pow2ceil(g.dk);
  if (g.DKp > 64) return g;
  const int need = K * g.DKp;
  g.DP = pow2ceil(need < 16 ? 16 : need);
  if (g.DP > 128) return g;
  g.Kp = g.DP / g.DKp;
  g.ok = true;
  return g;
}

// The natural geometry: any K | d at d <= 128.  Concept blocks sit at their real columns (DKp = dk,
// no per-block padding, no phantom concepts), DP = pow2ceil(max(16, d)); the slab is
// gs[i DP + j] = Gt[i][j] (i, j < d), gs[DP DP + k] = S_k (k < K), +0 elsewhere.  The finish
// kernels take the block stride as a run-time value and work at DKp = dk; the partial is
// drsa_partial_nat_kernel (the padded partial kernels need power-of-two blocks).
Geom geom_nat(int d, int K) {
  Geom g{d, K, 0, 0, 0, 0, false};
  if (d <= 0 || d > 128 || K <= 0 || d % K) return g;
  g.dk = g.DKp = d / K;
  g.DP = pow2ceil(d < 16 ? 16 : d);
  g.Kp = K;
  g.ok = true;
  return g;
}

inline size_t slab_floats(const Geom& g) { return (size_t)g.DP * g.DP + g.Kp; }
// per-workgroup slab stride in the workspace: 16-B aligned rows for the float4 reduce
inline size_t slab_stride(const Geom& g) { return (slab_floats(g) + 3) / 4 * 4; }

// v if keep else +0.f, by bit mask: a use that is unconditional, so the compiler neither sinks the
// load that produced v into a branch nor has to wait for it before the use
__device__ __forceinline__ float keep_or_zero(float v, bool keep) {
  return __uint_as_float(__float_as_uint(v) & (keep ? 0xffffffffu : 0u));
}
__device__ __forceinline__ float4 keep_or_zero4(float4 v, bool keep) {
  return make_float4(keep_or_zero(v.x, keep), keep_or_zero(v.y, keep), keep_or_zero(v.z, keep),
                     keep_or_zero(v.w, keep));
}

// m-th padded column of the embedding (pairs with padded row d + m in the identity block)
__device__ __forceinline__ int pad_col(int m, int K, int dk, int DKp) {
  const int per = DKp - dk;
  if (per > 0 && m < K * per) return (m / per) * DKp + dk + m % per;
  return K * DKp + (m - K * per);
}

// The row partition of every fp32 gradient (drsa_run, drsa_partial, the fused and sharded steps,
// run_multi, the batched grid): L = min(kLeaves, ceil(N / 16)) LEAVES, leaf l = row blocks
// [l R / L, (l + 1) R / L) of the R 16-row blocks, each reduced by the partial's fixed wave order
// into a leaf slab; leaves form groups of kLeafGroup (ascending); the gradient is the left fold over
// groups of the left fold over each group's leaves.  drsa_partial_kernel runs one workgroup per
// leaf; drsa_partial_grouped_kernel (the batched grid) runs whole groups per workgroup and folds
// them on chip -- the same leaf slabs added in the same order, so the same bits for any number of
// workgroups per problem.  Fixed constants (not the CU count): results do not depend on the device.
constexpr int kLeaves = 256;
constexpr int kLeafGroup = 8;
constexpr int kMaxGroups = kLeaves / kLeafGroup;

}  // namespace
