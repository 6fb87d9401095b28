// Whole-track explanations (DESIGN.md "Whole-track explanations"): the maps of n overlapping chunks,
// chunk c starting at track column c*h, are stitched into one track-length map per concept by a
// tapered overlap-add, and the concepts are un-sorted on the way (a chunk's slot j holds concept
// order[c][j]; the track's map k is always concept k - 1).
//
//   out[k][r][u] = (fmaf chain over the chunks c that cover u, ascending, of taper[t] x_c[r][t])
//                  / (plain sum of taper[t] in the same order),          t = u - c*h
//   act[k][u]    = sum over r of out[k][r][u]
//
// Memory-bound: every input element is read once and every output element written once.  One
// workgroup owns 32 rows x 32 lanes of columns of one map; a lane owns V = 4 adjacent columns when
// W, h (and so Wt) are multiples of 4 and the pointers are 16-byte aligned -- then the four columns
// share their cover set and every chunk read and output write is one 16-byte access -- and V = 1
// otherwise.  The 8 row lanes of a workgroup keep 4 rows each in flight.
#include "common.h"
#include "drsa_amd.h"

namespace {

constexpr int TS_CL = 32;                // column lanes of a workgroup
constexpr int TS_RL = 8;                 // row lanes
constexpr int TS_RPT = 4;                // rows per thread (all in flight)
constexpr int TS_RB = TS_RL * TS_RPT;    // rows per workgroup (include/drsa_amd.h states the act order)
constexpr int TS_THREADS = TS_CL * TS_RL;

struct StitchArgs {
  const float* std_maps;     // [n][1][H][W] or NULL
  const float* sub;          // [n][K][H][W]
  const int64_t* order;      // [n][K] or NULL
  const float* taper;        // [W]
  float* out;                // [C][H][Wt]
  float* act;                // [C][Wt]            (one row block)
  float* part;               // [C][nrb][Wt]       (several)
  int n, K, H, W, h, Wt, nrb, has_std, nslot;
};

template <int V> struct Vec;
template <> struct Vec<1> { using T = float; };
template <> struct Vec<4> { using T = float4; };

template <int V> __device__ __forceinline__ void load_v(const float* p, float (&x)[V]) {
  const typename Vec<V>::T v = *reinterpret_cast<const typename Vec<V>::T*>(p);
  if constexpr (V == 4) {
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
    x[0] = v;
  }
}

template <int V> __device__ __forceinline__ void store_v(float* p, const float (&x)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
    *p = x[0];
  }
}

// first and last chunk that cover column u (the first as ceil((u - W + 1) / h), clamped at 0)
__device__ __forceinline__ int cover_lo(int u, int W, int h) { return u < W ? 0 : (u - W) / h + 1; }
__device__ __forceinline__ int cover_hi(int u, int h, int n) { return min(n - 1, u / h); }

template <int V> __global__ __launch_bounds__(TS_THREADS) void track_stitch_kernel(StitchArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int COLS = TS_CL * V;
  float* tp = sm;                                          // [W] the taper
  int* slot = reinterpret_cast<int*>(sm + ((a.W + 3) & ~3));   // [nslot] slot of this map's concept, per chunk
  float* red = reinterpret_cast<float*>(slot + ((a.nslot + 3) & ~3));   // [TS_RL][COLS] act partials
  const int tid = threadIdx.x, cx = tid % TS_CL, ry = tid / TS_CL;
  const int k = blockIdx.z, rb = blockIdx.y;
  const int u0 = blockIdx.x * COLS;
  const int ulast = min(u0 + COLS, a.Wt) - 1;
  // the chunks that cover any column of this block
  const int c0 = cover_lo(u0, a.W, a.h), c1 = cover_hi(ulast, a.h, a.n);
  const int concept = k - a.has_std;                       // -1: the standard map
  const bool is_std = concept < 0;

  for (int i = tid; i < a.W; i += TS_THREADS) tp[i] = a.taper[i];
  // the permutation of every covering chunk, inverted once: slot[c - c0] = j with order[c][j] = concept
  for (int i = tid; i <= c1 - c0; i += TS_THREADS) slot[i] = (a.order || is_std) ? 0 : concept;
  __syncthreads();
  if (a.order && !is_std)
    for (int i = tid; i < (c1 - c0 + 1) * a.K; i += TS_THREADS)
      if (a.order[(int64_t)c0 * a.K + i] == concept) slot[i / a.K] = i % a.K;
  __syncthreads();

  const int u = u0 + cx * V;
  const bool live = u < a.Wt;                              // V = 4: Wt is a multiple of 4, all four or none
  const int uu = live ? u : u0;                            // an idle lane follows the block's first column
  const int lo = cover_lo(uu, a.W, a.h), hi = cover_hi(uu, a.h, a.n);
  const int r0 = rb * TS_RB + ry;
  const int64_t HW = (int64_t)a.H * a.W;
  const float* src = is_std ? a.std_maps : a.sub;
  const int64_t cstride = is_std ? HW : a.K * HW;

  float num[TS_RPT][V], den[V];
#pragma unroll
  for (int j = 0; j < V; ++j) den[j] = 0.f;
#pragma unroll
  for (int i = 0; i < TS_RPT; ++i)
#pragma unroll
    for (int j = 0; j < V; ++j) num[i][j] = 0.f;

  for (int c = lo; c <= hi; ++c) {
    const int t = uu - c * a.h;                            // 0 <= t <= W - V
    float w[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      w[j] = tp[t + j];
      den[j] += w[j];
    }
    const float* xc = src + c * cstride + slot[c - c0] * HW + t;
    float x[TS_RPT][V];
#pragma unroll
    for (int i = 0; i < TS_RPT; ++i)                       // a row past H reads row H - 1 and is dropped below
      load_v<V>(xc + (int64_t)min(r0 + i * TS_RL, a.H - 1) * a.W, x[i]);
#pragma unroll
    for (int i = 0; i < TS_RPT; ++i)
#pragma unroll
      for (int j = 0; j < V; ++j) num[i][j] = fmaf(w[j], x[i][j], num[i][j]);
  }

  float av[V];
#pragma unroll
  for (int j = 0; j < V; ++j) av[j] = 0.f;
  float* o = a.out + (int64_t)k * a.H * a.Wt + uu;
#pragma unroll
  for (int i = 0; i < TS_RPT; ++i) {
    const int r = r0 + i * TS_RL;
    if (live && r < a.H) {
      float q[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        q[j] = num[i][j] / den[j];
        av[j] += q[j];
      }
      store_v<V>(o + (int64_t)r * a.Wt, q);
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) red[ry * COLS + cx * V + j] = av[j];
  __syncthreads();
  if (ry == 0 && live) {
    float s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      s[j] = 0.f;
      for (int y = 0; y < TS_RL; ++y) s[j] += red[y * COLS + cx * V + j];
    }
    float* dst = a.nrb == 1 ? a.act + (int64_t)k * a.Wt : a.part + ((int64_t)k * a.nrb + rb) * a.Wt;
    store_v<V>(dst + u, s);
  }
}

// act[k][u] = the row blocks' partial sums, block ascending from +0
__global__ __launch_bounds__(256) void track_act_kernel(const float* part, float* act, int nrb, int Wt) {
  const int u = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (u >= Wt) return;
  const float* p = part + (int64_t)k * nrb * Wt + u;
  float s = 0.f;
  for (int b = 0; b < nrb; ++b) s += p[(int64_t)b * Wt];
  act[(int64_t)k * Wt + u] = s;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// 0: device memory (not read here); 1: host memory the device can read; 2: pageable host memory
int order_residence(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();                               // not known to the runtime: plain host memory
    return 2;
  }
  if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeArray) return 0;
  if (at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged) return 1;
  return 2;
}

}  // namespace

extern "C" size_t drsa_amd_track_stitch_workspace_bytes(int C, int H, int64_t Wt) {
  if (C < 1 || H < 1 || Wt < 1) return 0;
  const int64_t nrb = ((int64_t)H + TS_RB - 1) / TS_RB;
  return nrb > 1 ? (size_t)C * nrb * Wt * sizeof(float) : 0;
}

extern "C" int drsa_amd_track_stitch(const float* std_maps, const float* sub, const int64_t* order, const float* taper,
                                     int n, int K, int H, int W, int h, float* out, float* act, void* ws,
                                     size_t ws_bytes, void* stream) {
  DRSA_REQUIRE(sub && taper && out && act, "track_stitch: null pointer (sub, taper, out, act)");
  DRSA_REQUIRE(n >= 1, "track_stitch: n >= 1 chunks, got %d", n);
  DRSA_REQUIRE(K >= 1, "track_stitch: K >= 1 concepts, got %d", K);
  DRSA_REQUIRE(H >= 1, "track_stitch: H >= 1 rows, got %d", H);
  DRSA_REQUIRE(W >= 1 && h >= 1 && h <= W, "track_stitch: the chunk step must satisfy 1 <= h <= W (a larger step leaves "
               "gaps), got h = %d, W = %d", h, W);
  const int64_t Wt = (int64_t)(n - 1) * h + W;
  const int C = K + (std_maps ? 1 : 0);
  const int64_t nrb = ((int64_t)H + TS_RB - 1) / TS_RB;
  DRSA_REQUIRE(Wt < (1LL << 31) && C <= 65535 && nrb <= 65535, "track_stitch: Wt = %lld, C = %d or H = %d too large for "
               "the grid", (long long)Wt, C, H);
  if (order) {
    const int res = order_residence(order);
    if (res != 0) {
      for (int c = 0; c < n; ++c)
        for (int v = 0; v < K; ++v) {
          int seen = 0;
          for (int j = 0; j < K; ++j) seen += order[(int64_t)c * K + j] == v;
          DRSA_REQUIRE(seen == 1, "track_stitch: order[%d] is not a permutation of 0..%d (%d occurs %d times)", c, K - 1,
                       v, seen);
        }
      DRSA_REQUIRE(res == 1, "track_stitch: order is in pageable host memory, which the device cannot read");
    }
  }
  const size_t need = drsa_amd_track_stitch_workspace_bytes(C, H, Wt);
  if (need > ws_bytes || (need && !ws)) {
    drsa::set_error("track_stitch: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    return DRSA_EWORKSPACE;
  }
  const bool vec = W % 4 == 0 && h % 4 == 0 && aligned16(sub) && aligned16(std_maps) && aligned16(out) &&
                   aligned16(act) && aligned16(ws);
  const int cols = TS_CL * (vec ? 4 : 1);
  // the chunks that cover one block of columns: at most (cols + W - 2) / h + 2
  const int64_t nslot = ((int64_t)cols + W) / h + 2;
  const size_t smem = ((size_t)((W + 3) & ~3) + (size_t)((nslot + 3) & ~3LL) + (size_t)TS_RL * cols) * 4;
  if (smem > DRSA_LDS_MAX) {
    drsa::set_error("track_stitch: LDS footprint %zu B exceeds 160 KB (W %d, h %d)", smem, W, h);
    return DRSA_EUNSUPPORTED;
  }
  StitchArgs a{std_maps, sub, order, taper, out, act, static_cast<float*>(ws), n, K, H, W, h, (int)Wt, (int)nrb,
               std_maps ? 1 : 0, (int)nslot};
  const dim3 grid((unsigned)((Wt + cols - 1) / cols), (unsigned)nrb, (unsigned)C);
  if (vec) {
    DRSA_SMEM(track_stitch_kernel<4>, smem);
    hipLaunchKernelGGL(track_stitch_kernel<4>, grid, dim3(TS_THREADS), smem, (hipStream_t)stream, a);
  } else {
    DRSA_SMEM(track_stitch_kernel<1>, smem);
    hipLaunchKernelGGL(track_stitch_kernel<1>, grid, dim3(TS_THREADS), smem, (hipStream_t)stream, a);
  }
  DRSA_LAUNCH_CHECK();
  if (nrb > 1) {
    hipLaunchKernelGGL(track_act_kernel, dim3((unsigned)((Wt + 255) / 256), (unsigned)C), dim3(256), 0,
                       (hipStream_t)stream, a.part, act, (int)nrb, (int)Wt);
    DRSA_LAUNCH_CHECK();
  }
  return DRSA_OK;
}
