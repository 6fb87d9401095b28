// DRSA optimiser on gfx950: one Stiefel gradient-ascent step + polar retraction.
//
// Reference semantics (cxai/xai/drsa/drsa.py):
//   obj_val        drsa.py:122-155   s = relu(sum_{j in k} (AU)_nj (CU)_nj)   [N, K]
//   objective_fn   drsa.py:224-238   f = (mean_k sqrt( sqrt(mean_n s_nk^2) ))^2
//   run            drsa.py:84-106    U <- orthogonalize(U + grad f(U)), log f(U)
//   orthogonalize  drsa.py:201-221   U (U^T U)^{-1/2}  (reference: fp64 eigh on the host)
//
// One step = three launches (a dependent kernel boundary costs ~1.5 us on MI355X, less than a
// hand-rolled grid barrier, MI355X_MICROARCH.md "boundary" / "barrier-xcd"):
//   drsa_partial_kernel  row blocks of A, C spread over every CU.  Per 16-row block a wave runs
//                        XA = A_b U, XC = C_b U (fp32 MFMA, U held in registers), s, r = relu(s),
//                        S_k += r^2 and Gt += A_b^T (r (.) XC) + C_b^T (r (.) XA) straight from the
//                        MFMA output registers (no LDS round trip for P, Q); one [DP^2 + Kp] slab
//                        per workgroup, waves combined in a fixed order.
//   drsa_reduce_kernel   fixed-order sum of the slabs (deterministic, no atomics).
//   drsa_finish_kernel   M_k = sqrt(S_k/N), f, c_k = sqrt(f)/(K N M_k^1.5), V = U + Gt diag(c),
//                        polar(V) by Newton-Schulz on fp32 MFMA in one 16-wave workgroup (the Gram
//                        matrix from its upper block triangle, scaling from the first Gram).
// The closed-form gradient equals autograd's (checked in float64 in tests/test_oracle_drsa.py).
//
// Any d <= 128 with K | d runs through an exact embedding into a padded problem (DP, DKp):
// concept block k of width dk = d/K occupies padded columns [k DKp, k DKp + dk) with DKp the next
// power of two >= dk; padded columns and rows hold zeros in A, C, U, so every sum gets only exact
// +0 terms, and the polar step pairs the DP - d padded rows with the padded columns through an
// identity block (polar(diag(V, I)) = diag(polar(V), I)).  E.g. VGGish layer 19 (d = 100, K = 4,
// getdrsadata.py:119) runs as DP = 128, DKp = 32.  The gradient slab that crosses the ABI (and the
// all-reduce of the sharded path) is in padded coordinates: drsa_amd_drsa_slab_floats(d, K).
// That embedding needs DKp <= 64 and K DKp <= 128.  Every other K | d (d = 100 with K = 5, 10, 20;
// K = 1 at d > 64; ...) runs on the natural geometry -- blocks at their real columns, geom_nat,
// drsa_partial_nat.h -- through the drsa_amd_drsa_any_* entry points at the end of this file.
#include "common.h"
#include "drsa_amd.h"
#include "polar_ns.h"
#include "drsa_geom.h"
#include "drsa_partial.h"
#include "drsa_partial_nat.h"
#include "drsa_finish.h"
#include "drsa_coop.h"

#include <type_traits>
#include <vector>

namespace {

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------
// The template dispatch: f(std::integral_constant<int, V>{}) for the run-time padded size / concept
// width.  A value outside the set (and so outside the instantiated kernels) is DRSA_EUNSUPPORTED.
template <int V>
using Int = std::integral_constant<int, V>;

template <class F>
int with_dp(int DP, F&& f) {
  switch (DP) {
    case 16: return f(Int<16>{});
    case 32: return f(Int<32>{});
    case 64: return f(Int<64>{});
    case 128: return f(Int<128>{});
  }
  return DRSA_EUNSUPPORTED;
}

// a concept is at most as wide as the padded problem: no DKp = 32 at DP = 16, no DKp = 64 below DP = 64
template <int DP, class F>
int with_dkp(int DKp, F&& f) {
  switch (DKp) {
    case 1: return f(Int<1>{});
    case 2: return f(Int<2>{});
    case 4: return f(Int<4>{});
    case 8: return f(Int<8>{});
    case 16: return f(Int<16>{});
    case 32: if constexpr (DP >= 32) return f(Int<32>{}); break;
    case 64: if constexpr (DP >= 64) return f(Int<64>{}); break;
  }
  return DRSA_EUNSUPPORTED;
}

struct PartialPlan {
  int grid;
  int64_t rb_total;
};

PartialPlan plan_partial(int64_t N) {
  const int64_t rbt = (N + 15) / 16;
  int64_t grid = kLeaves;            // one workgroup per leaf (= per CU on MI355X); 16-row blocks
  if (grid > rbt) grid = rbt;
  if (grid < 1) grid = 1;
  return {(int)grid, rbt};
}

template <int DP, int DKP, int DT>
int launch_partial(const void* A, const void* C, int64_t N, const Geom& g, const float* U, float* partials,
                   const PartialPlan& pl, hipStream_t s) {
  using Cfg = PCfg<DP, DKP>;
  auto kern = (g.d & 3) == 0 ? drsa_partial_kernel<DP, DKP, DT, true> : drsa_partial_kernel<DP, DKP, DT, false>;
  DRSA_SMEM(kern, Cfg::lds_bytes);
  hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(Cfg::NT), Cfg::lds_bytes, s, A, C, N, g.d, g.K, g.dk, U, partials,
                     pl.rb_total);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

// no 16-bit A, C at DP = 16 (the 16-bit MFMA tiles are 32 deep)
int dispatch_partial(const void* A, const void* C, int64_t N, const Geom& g, const float* U, float* partials,
                     const PartialPlan& pl, hipStream_t s, int dt) {
  const int rc = with_dp(g.DP, [&](auto dp) -> int {
    constexpr int DP = decltype(dp)::value;
    return with_dkp<DP>(g.DKp, [&](auto dkp) -> int {
      constexpr int DKP = decltype(dkp)::value;
      if constexpr (DP >= 32) {
        if (dt == 1) return launch_partial<DP, DKP, 1>(A, C, N, g, U, partials, pl, s);
        if (dt == 2) return launch_partial<DP, DKP, 2>(A, C, N, g, U, partials, pl, s);
      } else if (dt) {
        return DRSA_EUNSUPPORTED;
      }
      return launch_partial<DP, DKP, 0>(A, C, N, g, U, partials, pl, s);
    });
  });
  if (rc == DRSA_EUNSUPPORTED)
    drsa::set_error("drsa_partial: unsupported d=%d K=%d%s", g.d, g.K, dt == 1 ? " (bf16)" : dt == 2 ? " (fp16)" : "");
  return rc;
}

template <int DP>
int launch_finish(const float* gs, double n_total, const Geom& g, const float* U, float* U_out, float* f_out,
                  int* counter, int by_counter, int mode, float tol, int max_iter, int* iters, hipStream_t s) {
  const size_t lds = finish_lds<DP>();
  DRSA_SMEM(drsa_finish_kernel<DP>, lds);
  hipLaunchKernelGGL(drsa_finish_kernel<DP>, dim3(1), dim3(fin_threads<polar_dim<DP>()>()), lds, s, gs, n_total, g.d,
                     g.K, g.DKp,
                     U, U_out, f_out, counter, by_counter, mode, tol, max_iter, iters);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

int dispatch_finish(const float* gs, double n_total, const Geom& g, const float* U, float* U_out, float* f_out,
                    int* counter, int by_counter, int mode, float tol, int max_iter, int* iters, hipStream_t s) {
  return with_dp(g.DP, [&](auto dp) -> int {
    return launch_finish<decltype(dp)::value>(gs, n_total, g, U, U_out, f_out, counter, by_counter, mode, tol, max_iter,
                                              iters, s);
  });
}

constexpr float kPolarTol = 4e-7f;
constexpr int kPolarMaxIter = 40;

int launch_reduce(const float* partials, const PartialPlan& pl, const Geom& g, float* gs_out, hipStream_t s) {
  const size_t E = slab_floats(g), ES = slab_stride(g);
  if (E <= 8192) {
    constexpr int CW = DRSA_REDUCE_CW;
    hipLaunchKernelGGL(drsa_reduce_kernel<CW>, dim3((unsigned)((E + CW - 1) / CW)), dim3(256), 0, s, partials, pl.grid,
                       (int)E, (int)ES, gs_out);
    DRSA_LAUNCH_CHECK();
    return DRSA_OK;
  }
  hipLaunchKernelGGL(drsa_reduce_kernel<64>, dim3((unsigned)((E + 63) / 64)), dim3(256), 0, s, partials, pl.grid, (int)E,
                     (int)ES, gs_out);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

// the fused step (drsa_fused_step_kernel) covers DP = 64 with concept blocks <= 16 wide (one
// 1024-thread workgroup shape for the partial and the polar): C3 and C4.
bool fused_ok(const Geom& g) {
  return g.DP == 64 && g.DKp <= 16;
}

template <int DKP>
int launch_fused(const float* A, const float* C, int64_t N, double n_total, const Geom& g, const float* gs,
                 const float* U, float* U_out, float* f_out, int* counter, float* partials, const PartialPlan& pl,
                 hipStream_t s) {
  auto kern = (g.d & 3) == 0 ? drsa_fused_step_kernel<64, DKP, true> : drsa_fused_step_kernel<64, DKP, false>;
  const size_t lds = fused_lds<64, DKP>();
  DRSA_SMEM(kern, lds);
  hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(fin_threads<64>()), lds, s, A, C, N, g.d, g.K, g.dk, gs, n_total, U,
                     U_out, f_out, counter, partials, pl.rb_total, kPolarTol, kPolarMaxIter);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

// one fused step: gs (gradient slab at U over n_total rows) -> U_out = polar(U + G c), f(U) ->
// f_out[counter++] (f_out[0] without a counter), partial slabs of the N local rows at U_out ->
// reduce -> gs_out (gs_out may be gs: the reduce runs after every workgroup has read gs)
int fused_step(const float* A, const float* C, int64_t N, double n_total, const Geom& g, const float* gs,
               float* gs_out, const float* U, float* U_out, float* f_out, int* counter, void* ws, hipStream_t s) {
  const PartialPlan pl = plan_partial(N);
  float* partials = (float*)ws;
  const int rc = with_dkp<64>(g.DKp, [&](auto dkp) -> int {
    constexpr int DKP = decltype(dkp)::value;
    if constexpr (DKP <= 16)   // fused_ok
      return launch_fused<DKP>(A, C, N, n_total, g, gs, U, U_out, f_out, counter, partials, pl, s);
    return DRSA_EUNSUPPORTED;
  });
  if (rc == DRSA_EUNSUPPORTED) drsa::set_error("drsa fused step: unsupported d=%d K=%d", g.d, g.K);
  if (rc) return rc;
  return launch_reduce(partials, pl, g, gs_out, s);
}

// workspace layout: [partials grid*E] [gs E] [16 B pad]; DP = 128 adds the cooperative finish's
// exchange area (CoopXchg) at the next 256-B boundary after gs
size_t ws_bytes(int64_t N, const Geom& g) {
  const PartialPlan pl = plan_partial(N);
  const size_t base = ((size_t)pl.grid * slab_stride(g) + slab_floats(g)) * sizeof(float) + 64;
  return g.DP == 128 ? base + 256 + sizeof(CoopXchg) : base;
}

// The argument check of every entry point (`who` in front of each message): the geometry is
// supported and N > 0, plus what `need` asks for.  Sets g; DRSA_EINVAL with the error set otherwise.
enum : unsigned {
  kEmptyOk = 1,   // N = 0 is allowed (and then needs neither workspace nor alignment)
  kWs = 2,        // ws holds ws_bytes(N, g)
  kAlign = 4,     // A and C are 16-byte aligned (float4 loads)
  kNoAlias = 8,   // U != U_out
  kDtype = 16,    // dtype is 0 (fp32), or 1 / 2 (bf16 / fp16) at padded d >= 32
};

struct ProblemArgs {   // what the needs look at
  const void *U = nullptr, *U_out = nullptr, *ws = nullptr;
  size_t ws_size = 0;
  const void *A = nullptr, *C = nullptr;
  int dtype = 0;
};

int check_problem(const char* who, Geom& g, int d, int K, int64_t N, unsigned need, const ProblemArgs& a = {},
                  bool natural = false) {
  g = natural ? geom_nat(d, K) : geom(d, K);
  if (natural) {   // the drsa_any_* entry points
    if (!g.ok) {
      drsa::set_error("%s: unsupported d=%d K=%d (need 0 < d <= 128 and K | d)", who, d, K);
      return DRSA_EUNSUPPORTED;
    }
  }
  DRSA_REQUIRE(g.ok, "%s: unsupported d=%d K=%d (need d <= 128, K | d, padded concept width <= 64 and "
               "K * padded width <= 128)", who, d, K);
  DRSA_REQUIRE(N > 0 || (N == 0 && (need & kEmptyOk)), "%s: N must be %s 0", who, (need & kEmptyOk) ? ">=" : ">");
  DRSA_REQUIRE(!(need & kDtype) || (a.dtype >= 0 && a.dtype <= 2), "%s: dtype must be 0 (fp32) or 1/2 (bf16/fp16)",
               who);
  if ((need & kDtype) && a.dtype && g.DP < 32) {   // a valid request with no kernel: the 16-bit MFMA tiles are 32 deep
    drsa::set_error("%s: unsupported d=%d K=%d for 16-bit A, C (needs padded d >= 32)", who, d, K);
    return DRSA_EUNSUPPORTED;
  }
  DRSA_REQUIRE(!(need & kNoAlias) || a.U != a.U_out, "%s: U and U_out must not alias", who);
  if (N == 0) return DRSA_OK;
  DRSA_REQUIRE(!(need & kWs) || (a.ws && a.ws_size >= ws_bytes(N, g)), "%s: workspace too small", who);
  DRSA_REQUIRE(!(need & kAlign) || (((uintptr_t)a.A % 16) == 0 && ((uintptr_t)a.C % 16) == 0),
               "%s: A/C must be 16B aligned", who);
  return DRSA_OK;
}

// one drsa_amd_problem_t of run_multi / run_batched
int check_run_problem(const char* entry, int p, const drsa_amd_problem_t& q, Geom& g, unsigned need) {
  char who[64];
  snprintf(who, sizeof(who), "%s: problem %d", entry, p);
  const ProblemArgs a{q.U_io, q.U_tmp, q.ws, q.ws_size, q.A, q.C, q.dtype};
  if (int rc = check_problem(who, g, q.d, q.K, q.N, need | kWs, a)) return rc;
  DRSA_REQUIRE(q.A && q.C && q.U_io && q.U_tmp && q.f_traj && q.counter, "%s: null pointer", who);
  return DRSA_OK;
}

// both fused-step entry points: DP = 64 geometry, the N local rows of N_total, workspace, alignment
int check_fused(const char* who, Geom& g, const void* A, const void* C, int64_t N, int d, int K, int64_t N_total,
                const void* U, const void* U_out, const void* ws, size_t ws_size) {
  if (int rc = check_problem(who, g, d, K, N, kNoAlias | kWs | kAlign, {U, U_out, ws, ws_size, A, C})) return rc;
  DRSA_REQUIRE(fused_ok(g), "%s: unsupported d=%d K=%d (drsa_amd_drsa_fused_supported)", who, d, K);
  DRSA_REQUIRE(N_total >= N, "%s: need N <= N_total", who);
  return DRSA_OK;
}

int partial_impl(const void* A, const void* C, int64_t N, int d, int K, const float* U, float* gs_out, void* ws,
                 size_t ws_size, void* stream, int dtype) {
  Geom g;
  if (int rc = check_problem("drsa_partial", g, d, K, N, kEmptyOk | kDtype | kWs | kAlign,
                             {U, nullptr, ws, ws_size, A, C, dtype}))
    return rc;
  DRSA_REQUIRE(A && C && U && gs_out, "drsa_partial: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const size_t E = slab_floats(g);
  if (N == 0) {
    DRSA_HIP(hipMemsetAsync(gs_out, 0, E * sizeof(float), s));
    return DRSA_OK;
  }
  const PartialPlan pl = plan_partial(N);
  float* partials = (float*)ws;
  int rc = dispatch_partial(A, C, N, g, U, partials, pl, s, dtype);
  if (rc) return rc;
  return launch_reduce(partials, pl, g, gs_out, s);
}

float* ws_gs(void* ws, int64_t N, const Geom& g) {
  return (float*)ws + (size_t)plan_partial(N).grid * slab_stride(g);
}

CoopXchg* ws_xchg(void* ws, int64_t N, const Geom& g) {
  if (g.DP != 128) return nullptr;
  const uintptr_t e = (uintptr_t)(ws_gs(ws, N, g) + slab_floats(g));
  return (CoopXchg*)((e + 255) / 256 * 256);
}

// the exchange counter starts at 0 (kCoopWG arrivals per hand-off from there), the status word clear
int coop_reset(CoopXchg* xc, hipStream_t s) {
  static_assert(offsetof(CoopXchg, status) == offsetof(CoopXchg, ticket) + sizeof(unsigned), "ticket, status");
  if (xc) DRSA_HIP(hipMemsetAsync(&xc->ticket, 0, 2 * sizeof(unsigned), s));
  return DRSA_OK;
}

// spin budget of the cooperative finish (drsa_amd_debug_coop_spin_budget; default 100 ms + 20k polls)
long long g_coop_spin_ticks = kCoopSpinTicks;
int g_coop_min_polls = kCoopMinPolls;

// a capture is open on s (never asked of the null stream)
bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return s && hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// reads the run's sticky status word back (synchronises stream s); DRSA_ETIMEOUT if it is set
int coop_check(const CoopXchg* xc, hipStream_t s, const char* what) {
  if (!xc) return DRSA_OK;
  unsigned st = 0;
  DRSA_HIP(hipMemcpyAsync(&st, &xc->status, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  DRSA_HIP(hipStreamSynchronize(s));
  if (st) {
    drsa::set_error("%s: a cooperative finish hand-off timed out (the %d workgroups were not co-resident "
                    "within the spin budget); U and f are NaN from that step on", what, kCoopWG);
    return DRSA_ETIMEOUT;
  }
  return DRSA_OK;
}

// a full finish step at DP = 128 on kCoopWG cooperating workgroups (bit-identical to dispatch_finish)
int launch_finish_coop(const float* gs, double n_total, const Geom& g, const float* U, float* U_out, float* f_out,
                       int* counter, int by_counter, CoopXchg* xc, hipStream_t s) {
  const size_t lds = coop_lds_bytes();
  DRSA_SMEM(drsa_finish_coop_kernel, lds);
  hipLaunchKernelGGL(drsa_finish_coop_kernel, dim3(kCoopWG), dim3(1024), lds, s, gs, n_total, g.d, g.K, g.DKp, U, U_out,
                     f_out, counter, by_counter, kPolarTol, kPolarMaxIter, xc, g_coop_spin_ticks, g_coop_min_polls);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

// finish of one step of drsa_run / run_multi: cooperative at DP = 128, else the one-workgroup kernel
int step_finish(const float* gs, double n_total, const Geom& g, const float* U, float* U_out, float* f_out,
                int* counter, CoopXchg* xc, hipStream_t s) {
  if (U_out && xc && g.DP == 128) return launch_finish_coop(gs, n_total, g, U, U_out, f_out, counter, 1, xc, s);
  return dispatch_finish(gs, n_total, g, U, U_out, f_out, counter, 1, U_out ? 0 : 1, kPolarTol, kPolarMaxIter, nullptr,
                         s);
}

// the captured pair of steps and its executable, released on every path out of run_steps
struct StepGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  ~StepGraph() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
  }
};

// The step loop of drsa_run, run_multi and run_batched on stream s.  pair() records two steps
// U_io -> U_tmp -> U_io, tail() one step and the copy of U_tmp home, final() the objective at U_S.
// With use_graph, steps >= 2 and no capture already open on s, pair() is captured once into a
// hipGraph and replayed steps / 2 times; otherwise (also inside a caller's capture) the pairs are
// recorded one after the other.  Then the odd tail and the final objective.
template <class Pair, class Tail, class Final>
int run_steps(hipStream_t s, int steps, bool use_graph, Pair&& pair, Tail&& tail, Final&& final) {
  int done = 0;
  if (use_graph && steps >= 2 && !stream_capturing(s)) {
    StepGraph g;
    DRSA_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = pair();
    const hipError_t ce = hipStreamEndCapture(s, &g.graph);   // also after a failed body: the capture must end
    if (rc) return rc;
    DRSA_HIP(ce);
    DRSA_HIP(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
    for (; done + 2 <= steps; done += 2) DRSA_HIP(hipGraphLaunch(g.exec, s));
  }
  for (; done + 2 <= steps; done += 2)
    if (int rc = pair()) return rc;
  if (done < steps)
    if (int rc = tail()) return rc;
  return final();
}

// ---------------------------------------------------------------------------
// the natural geometry (drsa_amd_drsa_any_*): geom_nat, the ragged partial, then the same reduce
// and finish kernels at block stride DKp = dk
// ---------------------------------------------------------------------------
template <int DP>
int launch_partial_nat(const float* A, const float* C, int64_t N, const Geom& g, const float* U, float* partials,
                       const PartialPlan& pl, hipStream_t s) {
  using Cfg = NCfg<DP>;
  auto kern = (g.d & 3) == 0 ? drsa_partial_nat_kernel<DP, true> : drsa_partial_nat_kernel<DP, false>;
  DRSA_SMEM(kern, Cfg::lds_bytes);
  hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(Cfg::NT), Cfg::lds_bytes, s, A, C, N, g.d, g.K, g.dk, U, partials,
                     pl.rb_total, (int)slab_stride(g));
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

// gs_out = the gradient slab of the N rows at U (N = 0: zeros); arguments already checked
int any_partial(const float* A, const float* C, int64_t N, const Geom& g, const float* U, float* gs_out, void* ws,
                hipStream_t s) {
  if (N == 0) {
    DRSA_HIP(hipMemsetAsync(gs_out, 0, slab_floats(g) * sizeof(float), s));
    return DRSA_OK;
  }
  const PartialPlan pl = plan_partial(N);
  float* partials = (float*)ws;
  const int rc = with_dp(g.DP, [&](auto dp) -> int {
    return launch_partial_nat<decltype(dp)::value>(A, C, N, g, U, partials, pl, s);
  });
  if (rc) return rc;
  return launch_reduce(partials, pl, g, gs_out, s);
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

#ifdef DRSA_COOP_STAMP
int drsa_amd_debug_coop_stamps(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_coop_stamps), sizeof(g_coop_stamps));
}
#endif

int drsa_amd_drsa_coop_status(const void* ws, int64_t N, int d, int K, int* status_out, void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_coop_status", g, d, K, N, 0)) return rc;
  DRSA_REQUIRE(ws && status_out, "drsa_coop_status: null pointer");
  hipStream_t s = (hipStream_t)stream;
  DRSA_REQUIRE(!stream_capturing(s), "drsa_coop_status: the stream is being captured");
  *status_out = 0;
  const CoopXchg* xc = ws_xchg(const_cast<void*>(ws), N, g);
  if (!xc) return DRSA_OK;
  unsigned st = 0;
  DRSA_HIP(hipMemcpyAsync(&st, &xc->status, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  DRSA_HIP(hipStreamSynchronize(s));
  *status_out = st ? 1 : 0;
  return DRSA_OK;
}

int drsa_amd_debug_coop_spin_budget(long long ticks) {
  DRSA_REQUIRE(ticks >= -1, "debug_coop_spin_budget: ticks must be >= -1");
  if (ticks < 0) {
    g_coop_spin_ticks = kCoopSpinTicks;
    g_coop_min_polls = kCoopMinPolls;
  } else {
    g_coop_spin_ticks = ticks;
    g_coop_min_polls = 0;
  }
  return DRSA_OK;
}

size_t drsa_amd_drsa_workspace_bytes(int64_t N, int d, int K) {
  const Geom g = geom(d, K);
  if (!g.ok || N <= 0) return 0;
  return ws_bytes(N, g);
}

size_t drsa_amd_drsa_slab_floats(int d, int K) {
  const Geom g = geom(d, K);
  return g.ok ? slab_floats(g) : 0;
}

int drsa_amd_drsa_partial(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                          float* gs_out, void* ws, size_t ws_size, void* stream) {
  return partial_impl(A, C, N, d, K, U, gs_out, ws, ws_size, stream, 0);
}

int drsa_amd_drsa_partial_bf16(const uint16_t* A, const uint16_t* C, int64_t N, int d, int K, const float* U,
                               float* gs_out, void* ws, size_t ws_size, void* stream) {
  return partial_impl(A, C, N, d, K, U, gs_out, ws, ws_size, stream, 1);
}

int drsa_amd_drsa_partial_f16(const uint16_t* A, const uint16_t* C, int64_t N, int d, int K, const float* U,
                              float* gs_out, void* ws, size_t ws_size, void* stream) {
  return partial_impl(A, C, N, d, K, U, gs_out, ws, ws_size, stream, 2);
}

int drsa_amd_drsa_finish(const float* gs, int64_t N_total, int d, int K, const float* U, float* U_out,
                         float* f_out, int objective_only, int* iters_out, void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_finish", g, d, K, N_total, objective_only ? 0 : kNoAlias, {U, U_out})) return rc;
  DRSA_REQUIRE(gs && U && f_out && (objective_only || U_out), "drsa_finish: null pointer");
  return dispatch_finish(gs, (double)N_total, g, U, U_out, f_out, nullptr, 0, objective_only ? 1 : 0, kPolarTol,
                         kPolarMaxIter, iters_out, (hipStream_t)stream);
}

int drsa_amd_drsa_fused_supported(int d, int K) { return fused_ok(geom(d, K)) ? 1 : 0; }

int drsa_amd_drsa_fused_step(const float* A, const float* C, int64_t N, int d, int K, const float* gs,
                             int64_t N_total, const float* U, float* U_out, float* f_out, float* gs_out, void* ws,
                             size_t ws_size, void* stream) {
  Geom g;
  if (int rc = check_fused("drsa_fused_step", g, A, C, N, d, K, N_total, U, U_out, ws, ws_size)) return rc;
  DRSA_REQUIRE(A && C && gs && U && U_out && f_out && gs_out, "drsa_fused_step: null pointer");
  return fused_step(A, C, N, (double)N_total, g, gs, gs_out, U, U_out, f_out, nullptr, ws, (hipStream_t)stream);
}

int drsa_amd_drsa_fused_step_counted(const float* A, const float* C, int64_t N, int d, int K, const float* gs,
                                     int64_t N_total, const float* U, float* U_out, float* f_traj, int* counter,
                                     float* gs_out, void* ws, size_t ws_size, void* stream) {
  Geom g;
  if (int rc = check_fused("drsa_fused_step_counted", g, A, C, N, d, K, N_total, U, U_out, ws, ws_size)) return rc;
  DRSA_REQUIRE(A && C && gs && U && U_out && f_traj && counter && gs_out, "drsa_fused_step_counted: null pointer");
  return fused_step(A, C, N, (double)N_total, g, gs, gs_out, U, U_out, f_traj, counter, ws, (hipStream_t)stream);
}

int drsa_amd_drsa_finish_counted(const float* gs, int64_t N_total, int d, int K, const float* U, float* U_out,
                                 float* f_traj, int* counter, void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_finish_counted", g, d, K, N_total, kNoAlias, {U, U_out})) return rc;
  DRSA_REQUIRE(gs && U && U_out && f_traj && counter, "drsa_finish_counted: null pointer");
  return dispatch_finish(gs, (double)N_total, g, U, U_out, f_traj, counter, 1, 0, kPolarTol, kPolarMaxIter, nullptr,
                         (hipStream_t)stream);
}

int drsa_amd_drsa_step(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                       float* U_out, float* f_out, void* ws, size_t ws_size, void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_step", g, d, K, N, kNoAlias | kWs, {U, U_out, ws, ws_size})) return rc;
  float* gs = ws_gs(ws, N, g);
  int rc = drsa_amd_drsa_partial(A, C, N, d, K, U, gs, ws, ws_size, stream);
  if (rc) return rc;
  return drsa_amd_drsa_finish(gs, N, d, K, U, U_out, f_out, 0, nullptr, stream);
}

int drsa_amd_drsa_objective(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                            float* f_out, void* ws, size_t ws_size, void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_objective", g, d, K, N, kWs, {U, nullptr, ws, ws_size})) return rc;
  float* gs = ws_gs(ws, N, g);
  int rc = drsa_amd_drsa_partial(A, C, N, d, K, U, gs, ws, ws_size, stream);
  if (rc) return rc;
  return drsa_amd_drsa_finish(gs, N, d, K, U, nullptr, f_out, 1, nullptr, stream);
}

// S steps in one call: f_traj[0..steps] receives f(U_t) before each update and f(U_S) after
// the loop (SubspaceOptimizer.run's trajectory, drsa.py:82-117).  U_io holds U_0 on entry and
// U_S on exit; U_tmp is a d*d scratch.  With use_graph != 0 the two-step body is captured
// once into a hipGraph and replayed (launch-bound loop).
int drsa_amd_drsa_run(const float* A, const float* C, int64_t N, int d, int K, float* U_io, float* U_tmp,
                      int steps, float* f_traj, int* counter, void* ws, size_t ws_size, int use_graph,
                      void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_run", g, d, K, N, kWs, {U_io, U_tmp, ws, ws_size})) return rc;
  DRSA_REQUIRE(steps >= 0, "drsa_run: steps < 0");
  DRSA_REQUIRE(A && C && U_io && U_tmp && f_traj && counter, "drsa_run: null pointer");
  hipStream_t s = (hipStream_t)stream;
  float* gs = ws_gs(ws, N, g);
  DRSA_HIP(hipMemsetAsync(counter, 0, sizeof(int), s));
  CoopXchg* xc = ws_xchg(ws, N, g);
  if (int rc = coop_reset(xc, s)) return rc;
  // fused: the gradient at U_0 first, then per step one fused launch (finish of the previous step
  // + partial at the new U) and the slab reduce; the final objective reads the last gs
  const bool fused = fused_ok(g);
  if (fused) {
    int rc = drsa_amd_drsa_partial(A, C, N, d, K, U_io, gs, ws, ws_size, stream);
    if (rc) return rc;
  }
  auto one = [&](const float* Uin, float* Uout) -> int {
    if (fused) return fused_step(A, C, N, (double)N, g, gs, gs, Uin, Uout, f_traj, counter, ws, s);
    int rc = drsa_amd_drsa_partial(A, C, N, d, K, Uin, gs, ws, ws_size, stream);
    if (rc) return rc;
    return step_finish(gs, (double)N, g, Uin, Uout, f_traj, counter, xc, s);
  };
  auto pair = [&]() -> int {
    int rc = one(U_io, U_tmp);
    return rc ? rc : one(U_tmp, U_io);
  };
  auto tail = [&]() -> int {
    if (int rc = one(U_io, U_tmp)) return rc;
    DRSA_HIP(hipMemcpyAsync(U_io, U_tmp, (size_t)d * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    return DRSA_OK;
  };
  auto final = [&]() -> int {   // f(U_S) -> f_traj[steps]
    if (!fused) {
      int rc = drsa_amd_drsa_partial(A, C, N, d, K, U_io, gs, ws, ws_size, stream);
      if (rc) return rc;
    }
    return dispatch_finish(gs, (double)N, g, U_io, nullptr, f_traj, counter, 1, 1, kPolarTol, kPolarMaxIter, nullptr,
                           s);
  };
  // inside a caller's stream capture (e.g. a torch CUDA graph) this records the plain sequence and
  // leaves the cooperative finish's status check to the caller (drsa_amd_drsa_coop_status).
  // use_graph on the null stream is attempted (the capture fails with HIP's error).
  const bool capturing = stream_capturing(s);
  int rc = run_steps(s, steps, use_graph != 0, pair, tail, final);
  if (rc || capturing || steps == 0) return rc;
  return coop_check(xc, s, "drsa_run");
}

// P independent problems (e.g. the C5 joint optimisation of two layers, optsubspaces.py:18-23
// run one after the other in the reference) advanced together: per step every problem's
// partial/reduce/finish chain runs on its own forked stream inside ONE captured hipGraph, so
// the latency-bound single-workgroup finish kernels of different problems overlap and the
// whole S-step joint loop is one graph launch per two steps.
int drsa_amd_drsa_run_multi(int P, const drsa_amd_problem_t* probs, int steps, int use_graph, void* stream) {
  DRSA_REQUIRE(P >= 1 && P <= 64 && probs, "drsa_run_multi: P must be in [1, 64]");
  DRSA_REQUIRE(steps >= 0, "drsa_run_multi: steps < 0");
  bool all_f32 = true;
  for (int p = 0; p < P; ++p) {
    Geom g;
    if (int rc = check_run_problem("drsa_run_multi", p, probs[p], g, kDtype)) return rc;
    all_f32 = all_f32 && probs[p].dtype == 0;
  }
  if (all_f32 && (P == 1 || !use_graph || steps < 2)) {
    for (int p = 0; p < P; ++p) {
      const drsa_amd_problem_t& q = probs[p];
      int rc = drsa_amd_drsa_run(q.A, q.C, q.N, q.d, q.K, q.U_io, q.U_tmp, steps, q.f_traj, q.counter, q.ws,
                                 q.ws_size, use_graph, stream);
      if (rc) return rc;
    }
    return DRSA_OK;
  }
  hipStream_t s = (hipStream_t)stream;
  // side streams and fork/join events come from a per-thread, per-device pool that lives as long
  // as the thread: a captured graph's forks must not be destroyed before the capture ends
  struct SidePool {
    hipStream_t st[64] = {nullptr};
    hipEvent_t join[64] = {nullptr};
    hipEvent_t fork = nullptr;
  };
  thread_local SidePool pools[16];
  int dev = 0;
  DRSA_HIP(hipGetDevice(&dev));
  DRSA_REQUIRE(dev >= 0 && dev < 16, "drsa_run_multi: device index %d >= 16", dev);
  SidePool& pool = pools[dev];
  if (!pool.fork) DRSA_HIP(hipEventCreateWithFlags(&pool.fork, hipEventDisableTiming));
  for (int p = 0; p < P; ++p) {
    if (!pool.st[p]) DRSA_HIP(hipStreamCreateWithFlags(&pool.st[p], hipStreamNonBlocking));
    if (!pool.join[p]) DRSA_HIP(hipEventCreateWithFlags(&pool.join[p], hipEventDisableTiming));
    const drsa_amd_problem_t& q = probs[p];
    DRSA_HIP(hipMemsetAsync(q.counter, 0, sizeof(int), s));
    if (int rc = coop_reset(ws_xchg(q.ws, q.N, geom(q.d, q.K)), s)) return rc;
  }
  // one step of problem p on stream st: U_in -> U_out, f -> f_traj[counter++]
  auto one = [&](int p, hipStream_t st, const float* Uin, float* Uout) -> int {
    const drsa_amd_problem_t& q = probs[p];
    const Geom g = geom(q.d, q.K);
    float* gs = ws_gs(q.ws, q.N, g);
    int r = partial_impl(q.A, q.C, q.N, q.d, q.K, Uin, gs, q.ws, q.ws_size, st, q.dtype);
    if (r) return r;
    return step_finish(gs, (double)q.N, g, Uin, Uout, q.f_traj, q.counter, ws_xchg(q.ws, q.N, g), st);
  };
  // fork from s -> per problem, on its side stream: nsteps steps (an odd count ends in U_tmp and is
  // copied home), then the final objective if asked for -> join into s
  auto forked = [&](int nsteps, bool final_objective) -> int {
    DRSA_HIP(hipEventRecord(pool.fork, s));
    for (int p = 0; p < P; ++p) {
      const drsa_amd_problem_t& q = probs[p];
      hipStream_t st = pool.st[p];
      DRSA_HIP(hipStreamWaitEvent(st, pool.fork, 0));
      for (int k = 0; k < nsteps; ++k)
        if (int r = (k % 2 == 0) ? one(p, st, q.U_io, q.U_tmp) : one(p, st, q.U_tmp, q.U_io)) return r;
      if (nsteps & 1)
        DRSA_HIP(hipMemcpyAsync(q.U_io, q.U_tmp, (size_t)q.d * q.d * sizeof(float), hipMemcpyDeviceToDevice, st));
      if (final_objective)
        if (int r = one(p, st, q.U_io, nullptr)) return r;
      // Every side chain joins back into s before the call returns, whatever the geometry or step
      // count, and nothing else orders the side streams' work: a caller (or a caching allocator)
      // that frees or reuses A, C, U, f_traj or the workspaces in stream order on s after this call
      // is safe only because of this join.  Keep it on every path that put work on a side stream.
      DRSA_HIP(hipEventRecord(pool.join[p], st));
      DRSA_HIP(hipStreamWaitEvent(s, pool.join[p], 0));
    }
    return DRSA_OK;
  };
  // inside a caller's stream capture (a torch CUDA graph of the whole run) the forked plain sequence
  // is recorded into it: no graph of our own, no host synchronisation, no status read-back.
  // use_graph on the null stream is attempted (the capture fails with HIP's error).
  const bool capturing = stream_capturing(s);
  int rc = run_steps(s, steps, use_graph != 0, [&] { return forked(2, false); }, [&] { return forked(1, false); },
                     [&] { return forked(0, true); });
  if (rc || steps == 0 || capturing) return rc;
  for (int p = 0; p < P; ++p) {
    const drsa_amd_problem_t& q = probs[p];
    if (int rc2 = coop_check(ws_xchg(q.ws, q.N, geom(q.d, q.K)), s, "drsa_run_multi")) return rc2;
  }
  return DRSA_OK;
}

// P independent fp32 problems of one padded geometry advanced together, one launch per phase
// (partial / reduce / finish) for all of them -- the task-parallel DRSA grid of optsubspaces.py:17-23.
// blocks: workgroups per problem for the partial (0: about 4 waves of workgroups over the chip).
// Row partition, and so the fp32 summation order, depends on blocks: deterministic for a given
// value.  Graph-captured two steps at a time like drsa_amd_drsa_run.
int drsa_amd_drsa_run_batched(int P, const drsa_amd_problem_t* probs, int steps, int blocks, int use_graph,
                              void* stream) {
  DRSA_REQUIRE(P >= 1 && probs, "drsa_run_batched: P must be >= 1");
  DRSA_REQUIRE(steps >= 0, "drsa_run_batched: steps < 0");
  Geom g{};   // problem 0's: every problem shares its padded geometry
  bool vec = true;
  for (int p = 0; p < P; ++p) {
    const drsa_amd_problem_t& q = probs[p];
    Geom gq;
    if (int rc = check_run_problem("drsa_run_batched", p, q, gq, kAlign)) return rc;
    if (p == 0) g = gq;
    DRSA_REQUIRE(gq.DP == g.DP && gq.DKp == g.DKp,
                 "drsa_run_batched: problem %d (d=%d K=%d) does not share the padded geometry of problem 0", p,
                 q.d, q.K);
    DRSA_REQUIRE(q.dtype == 0, "drsa_run_batched: fp32 problems only (problem %d)", p);
    vec = vec && (q.d & 3) == 0;
  }
  hipStream_t s = (hipStream_t)stream;
  DRSA_REQUIRE(!stream_capturing(s),
               "drsa_run_batched: not capturable (allocates its descriptor table); use drsa_run_multi");
  // workgroups per problem: `blocks`, or about 16 waves of one-workgroup-per-CU launches over the
  // chip (the 90-problem grid: one leaf group per workgroup, 36.4k problem-steps/s against 36.0k
  // at two groups); each owns m = ceil(groups / G) whole leaf groups (the result does not depend on it)
  const int cu = drsa::cu_count();
  int Greq = blocks > 0 ? blocks : (16 * cu + P - 1) / P;
  if (Greq < 1) Greq = 1;
  const size_t E = slab_floats(g), ES = slab_stride(g);
  int G = 1;
  const bool leafwise = g.DKp >= 64;          // see drsa_partial_leaf_batched_kernel
  std::vector<BatchDesc> hd((size_t)P);
  for (int p = 0; p < P; ++p) {
    const drsa_amd_problem_t& q = probs[p];
    const Geom gq = geom(q.d, q.K);
    const PartialPlan pl = plan_partial(q.N);   // the leaves of drsa_run's partition
    const int ngrp = (pl.grid + kLeafGroup - 1) / kLeafGroup;
    const int m = leafwise ? 0 : (ngrp + Greq - 1) / Greq;
    const int Gp = leafwise ? pl.grid : (ngrp + m - 1) / m;
    if (Gp > G) G = Gp;
    hd[p] = BatchDesc{q.A, q.C, q.N, pl.rb_total, q.d, q.K, q.d / q.K, gq.DKp, Gp, pl.grid, m, q.U_io, q.U_tmp,
                      q.f_traj, q.counter, (float*)q.ws, ws_gs(q.ws, q.N, gq)};
  }
  // descriptor table on the device; freed once the stream has drained (the kernels read it)
  struct DeviceTable {
    hipStream_t s;
    BatchDesc* ptr = nullptr;
    ~DeviceTable() {
      if (!ptr) return;
      (void)hipStreamSynchronize(s);
      (void)hipFree(ptr);
    }
  } table{s};
  DRSA_HIP(hipMalloc((void**)&table.ptr, sizeof(BatchDesc) * (size_t)P));
  const BatchDesc* dd = table.ptr;
  DRSA_HIP(hipMemcpyAsync(table.ptr, hd.data(), sizeof(BatchDesc) * (size_t)P, hipMemcpyHostToDevice, s));
  for (int p = 0; p < P; ++p) DRSA_HIP(hipMemsetAsync(probs[p].counter, 0, sizeof(int), s));
  // one step (or, with final_obj, the objective alone) of every problem: partial, reduce, finish
  auto launch_phase = [&](int parity, int final_obj) -> int {
    int r = with_dp(g.DP, [&](auto dp) -> int {
      constexpr int DP = decltype(dp)::value;
      return with_dkp<DP>(g.DKp, [&](auto dkp) -> int {
        constexpr int DKP = decltype(dkp)::value;
        using Cfg = PCfg<DP, DKP>;
        if constexpr (DKP >= 64) {     // = leafwise
          auto kern = vec ? drsa_partial_leaf_batched_kernel<DP, DKP, true> : drsa_partial_leaf_batched_kernel<DP, DKP, false>;
          DRSA_SMEM(kern, Cfg::lds_bytes);
          hipLaunchKernelGGL(kern, dim3(G, P), dim3(Cfg::NT), Cfg::lds_bytes, s, dd, parity);
        } else {
          auto kern = vec ? drsa_partial_grouped_kernel<DP, DKP, true> : drsa_partial_grouped_kernel<DP, DKP, false>;
          DRSA_SMEM(kern, Cfg::glds_bytes);
          hipLaunchKernelGGL(kern, dim3(G, P), dim3(Cfg::NT), Cfg::glds_bytes, s, dd, parity);
        }
        DRSA_LAUNCH_CHECK();
        return DRSA_OK;
      });
    });
    if (r) return r;
    hipLaunchKernelGGL(drsa_reduce_batched_kernel, dim3((unsigned)((E + 63) / 64), P), dim3(256), 0, s, dd,
                       (int)E, (int)ES);
    DRSA_LAUNCH_CHECK();
    return with_dp(g.DP, [&](auto dp) -> int {
      constexpr int DP = decltype(dp)::value;
      const size_t lds = finish_lds<DP>();
      DRSA_SMEM(drsa_finish_batched_kernel<DP>, lds);
      hipLaunchKernelGGL(drsa_finish_batched_kernel<DP>, dim3(P), dim3(fin_threads<polar_dim<DP>()>()), lds, s, dd,
                         parity, final_obj ? 1 : 0, kPolarTol, kPolarMaxIter);
      DRSA_LAUNCH_CHECK();
      return DRSA_OK;
    });
  };
  auto pair = [&]() -> int {
    int r = launch_phase(0, 0);
    return r ? r : launch_phase(1, 0);
  };
  auto tail = [&]() -> int {   // U_S sits in U_tmp: bring it home
    if (int r = launch_phase(0, 0)) return r;
    for (int p = 0; p < P; ++p)
      DRSA_HIP(hipMemcpyAsync(probs[p].U_io, probs[p].U_tmp, (size_t)probs[p].d * probs[p].d * sizeof(float),
                              hipMemcpyDeviceToDevice, s));
    return DRSA_OK;
  };
  // use_graph on the null stream runs the eager pairs here (unlike drsa_run / run_multi).
  // final objective at U_S -> f_traj[steps]; table's destructor synchronises s on every path
  return run_steps(s, steps, use_graph && s, pair, tail, [&] { return launch_phase(0, 1); });
}

// ---------------------------------------------------------------------------
// Every K | d at d <= 128 (the natural geometry, geom_nat): fp32 only, no fused step.  Each entry
// point takes its padded namesake's arguments and also accepts the shapes the padded path takes
// (its slab layout and summation order differ from the padded ones).
// ---------------------------------------------------------------------------
int drsa_amd_drsa_any_supported(int d, int K) { return geom_nat(d, K).ok ? 1 : 0; }

size_t drsa_amd_drsa_any_slab_floats(int d, int K) {
  const Geom g = geom_nat(d, K);
  return g.ok ? slab_floats(g) : 0;
}

size_t drsa_amd_drsa_any_workspace_bytes(int64_t N, int d, int K) {
  const Geom g = geom_nat(d, K);
  if (!g.ok || N <= 0) return 0;
  return ws_bytes(N, g);
}

int drsa_amd_drsa_any_partial(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                              float* gs_out, void* ws, size_t ws_size, void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_any_partial", g, d, K, N, kEmptyOk | kWs | kAlign, {U, nullptr, ws, ws_size, A, C},
                             true))
    return rc;
  DRSA_REQUIRE(A && C && U && gs_out, "drsa_any_partial: null pointer (d=%d K=%d)", d, K);
  return any_partial(A, C, N, g, U, gs_out, ws, (hipStream_t)stream);
}

int drsa_amd_drsa_any_finish(const float* gs, int64_t N_total, int d, int K, const float* U, float* U_out,
                             float* f_out, int objective_only, int* iters_out, void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_any_finish", g, d, K, N_total, objective_only ? 0 : kNoAlias, {U, U_out}, true))
    return rc;
  DRSA_REQUIRE(gs && U && f_out && (objective_only || U_out), "drsa_any_finish: null pointer (d=%d K=%d)", d, K);
  return dispatch_finish(gs, (double)N_total, g, U, U_out, f_out, nullptr, 0, objective_only ? 1 : 0, kPolarTol,
                         kPolarMaxIter, iters_out, (hipStream_t)stream);
}

int drsa_amd_drsa_any_finish_counted(const float* gs, int64_t N_total, int d, int K, const float* U, float* U_out,
                                     float* f_traj, int* counter, void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_any_finish_counted", g, d, K, N_total, kNoAlias, {U, U_out}, true)) return rc;
  DRSA_REQUIRE(gs && U && U_out && f_traj && counter, "drsa_any_finish_counted: null pointer (d=%d K=%d)", d, K);
  return dispatch_finish(gs, (double)N_total, g, U, U_out, f_traj, counter, 1, 0, kPolarTol, kPolarMaxIter, nullptr,
                         (hipStream_t)stream);
}

int drsa_amd_drsa_any_step(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                           float* U_out, float* f_out, void* ws, size_t ws_size, void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_any_step", g, d, K, N, kNoAlias | kWs | kAlign, {U, U_out, ws, ws_size, A, C}, true))
    return rc;
  DRSA_REQUIRE(A && C && U && U_out && f_out, "drsa_any_step: null pointer (d=%d K=%d)", d, K);
  hipStream_t s = (hipStream_t)stream;
  float* gs = ws_gs(ws, N, g);
  if (int rc = any_partial(A, C, N, g, U, gs, ws, s)) return rc;
  return dispatch_finish(gs, (double)N, g, U, U_out, f_out, nullptr, 0, 0, kPolarTol, kPolarMaxIter, nullptr, s);
}

int drsa_amd_drsa_any_objective(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                                float* f_out, void* ws, size_t ws_size, void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_any_objective", g, d, K, N, kWs | kAlign, {U, nullptr, ws, ws_size, A, C}, true))
    return rc;
  DRSA_REQUIRE(A && C && U && f_out, "drsa_any_objective: null pointer (d=%d K=%d)", d, K);
  hipStream_t s = (hipStream_t)stream;
  float* gs = ws_gs(ws, N, g);
  if (int rc = any_partial(A, C, N, g, U, gs, ws, s)) return rc;
  return dispatch_finish(gs, (double)N, g, U, nullptr, f_out, nullptr, 0, 1, kPolarTol, kPolarMaxIter, nullptr, s);
}

// drsa_amd_drsa_run for the natural geometry: per step the ragged partial, the slab reduce and the
// finish (cooperative at DP = 128: drsa_finish_coop_kernel takes the block stride at run time and
// nowhere needs a power of two), two steps captured into a hipGraph and replayed.
int drsa_amd_drsa_any_run(const float* A, const float* C, int64_t N, int d, int K, float* U_io, float* U_tmp,
                          int steps, float* f_traj, int* counter, void* ws, size_t ws_size, int use_graph,
                          void* stream) {
  Geom g;
  if (int rc = check_problem("drsa_any_run", g, d, K, N, kNoAlias | kWs | kAlign, {U_io, U_tmp, ws, ws_size, A, C}, true))
    return rc;
  DRSA_REQUIRE(steps >= 0, "drsa_any_run: steps < 0 (d=%d K=%d)", d, K);
  DRSA_REQUIRE(A && C && U_io && U_tmp && f_traj && counter, "drsa_any_run: null pointer (d=%d K=%d)", d, K);
  hipStream_t s = (hipStream_t)stream;
  float* gs = ws_gs(ws, N, g);
  DRSA_HIP(hipMemsetAsync(counter, 0, sizeof(int), s));
  CoopXchg* xc = ws_xchg(ws, N, g);
  if (int rc = coop_reset(xc, s)) return rc;
  auto one = [&](const float* Uin, float* Uout) -> int {
    if (int rc = any_partial(A, C, N, g, Uin, gs, ws, s)) return rc;
    return step_finish(gs, (double)N, g, Uin, Uout, f_traj, counter, xc, s);
  };
  auto pair = [&]() -> int {
    int rc = one(U_io, U_tmp);
    return rc ? rc : one(U_tmp, U_io);
  };
  auto tail = [&]() -> int {
    if (int rc = one(U_io, U_tmp)) return rc;
    DRSA_HIP(hipMemcpyAsync(U_io, U_tmp, (size_t)d * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    return DRSA_OK;
  };
  auto final = [&]() -> int { return one(U_io, nullptr); };   // f(U_S) -> f_traj[steps]
  const bool capturing = stream_capturing(s);
  int rc = run_steps(s, steps, use_graph != 0, pair, tail, final);
  if (rc || capturing || steps == 0) return rc;
  return coop_check(xc, s, "drsa_any_run");
}

int drsa_amd_polar(const float* V, int d, float* U_out, int* iters_out, void* stream) {
  DRSA_REQUIRE(d >= 1 && d <= 128, "polar: unsupported d=%d (1..128)", d);
  DRSA_REQUIRE(V && U_out, "polar: null pointer");
  hipStream_t s = (hipStream_t)stream;
  return with_dp(pow2ceil(d < 32 ? 32 : d), [&](auto dp) -> int {
    constexpr int DP = decltype(dp)::value;
    if constexpr (DP >= 32) {   // the polar alone pads to 32 at least
      const size_t lds = finish_lds<DP>();
      DRSA_SMEM(polar_kernel<DP>, lds);
      hipLaunchKernelGGL(polar_kernel<DP>, dim3(1), dim3(fin_threads<DP>()), lds, s, V, d, U_out, kPolarTol,
                         kPolarMaxIter, iters_out);
      DRSA_LAUNCH_CHECK();
      return DRSA_OK;
    }
    return DRSA_EUNSUPPORTED;
  });
}

}  // extern "C"
