// Concept audio at STFT resolution (DESIGN.md "Concept audio at STFT resolution"): the relevance at
// the log-mel input is carried one layer further down, through the mel filterbank onto the STFT
// bins, masked there, and rendered as mask x spectrum.  Three launches beside audiogen.hip's
// analysis and normalisation:
//
//   drsa_amd_mel_relevance_to_stft   R [n][C][n_mels][width], mel, X -> R_stft [n][C][n_freq][width]:
//                                    the LRP z-rule through the filterbank (eps absorbs)
//   drsa_amd_heatmap_mask_large      drsa_amd_heatmap_mask for maps that do not fit the LDS: the map
//                                    stays in global memory (L2), the blur runs on 64 x 64 tiles
//   drsa_amd_stft_mask_to_audio      Y = mask x X -> inverse real FFT -> window -> owned overlap-add
//                                    -> / window envelope -> trimmed audio (drsa_amd_mel_to_audio
//                                    without the mel tile and the pseudo-inverse)
//
// The argument checks and everything of the synthesis after Y are audio_synth.h's, shared with
// audiogen.hip; stft_mask_to_audio_kernel keeps the transposed mask tile and Y = mask x X.
#include "audio_synth.h"
#include "common.h"
#include "drsa_amd.h"
#include "stockham.h"

#include <math.h>

namespace {

// ===========================================================================
// Lift: one workgroup per (source, block of 32 frames), the source's C maps in turn.
//   den[m][t] = mel[m][t] + eps                                    (LDS, loaded once)
//   ax[f][t]  = |X[t][f]|                                          (LDS, transposed on the way in:
//                                                                   X is frame-major, the maps are
//                                                                   frequency-major)
//   q[m][t]   = R_c[m][t] / den[m][t]
//   out_c[f][t] = ax[f][t] * (fmaf chain over the bands m that cover bin f, ascending, from 0)
// The filterbank comes bin by bin: bin f is covered by bands bin_lo[f] .. bin_lo[f]+bin_n[f]-1 with
// the weights bin_w[bin_off[f] ..].
// ===========================================================================
constexpr int LF_THREADS = 512;
constexpr int LF_TT = 32;               // frames per workgroup: 128-byte runs of every map row
constexpr int LF_TS = LF_TT + 1;        // row stride of the transposed |X| tile (conflict-free both ways)

struct LiftArgs {
  const float* R;            // [n][C][n_mels][width]
  const float* mel;          // [n][n_mels][width]
  const float* X;            // [n][width][n_freq] complex
  const int* bin_lo;
  const int* bin_n;
  const int* bin_off;
  const float* bin_w;
  float* out;                // [n][C][n_freq][width]
  int C, n_mels, width, n_freq, nnz, nblk;
  float eps;
  int o_ax, o_den, o_q, o_lo, o_n, o_off, o_w;
};

__global__ __launch_bounds__(LF_THREADS) void mel_relevance_to_stft_kernel(LiftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / a.nblk;
  const int t0 = (blockIdx.x % a.nblk) * LF_TT;
  const int nt = min(LF_TT, a.width - t0);
  float* ax = sm + a.o_ax;                             // [n_freq][LF_TS]
  float* den = sm + a.o_den;                           // [n_mels][LF_TT]
  float* q = sm + a.o_q;                               // [n_mels][LF_TT]
  int* blo = reinterpret_cast<int*>(sm + a.o_lo);
  int* bn = reinterpret_cast<int*>(sm + a.o_n);
  int* boff = reinterpret_cast<int*>(sm + a.o_off);
  float* bw = sm + a.o_w;

  // the tables are device data: a run is cut to the bands and weights that exist
  for (int f = tid; f < a.n_freq; f += LF_THREADS) {
    const int lo = min(max(a.bin_lo[f], 0), a.n_mels);
    const int off = min(max(a.bin_off[f], 0), a.nnz);
    blo[f] = lo;
    boff[f] = off;
    bn[f] = max(min(min(a.bin_n[f], a.n_mels - lo), a.nnz - off), 0);
  }
  for (int i = tid; i < a.nnz; i += LF_THREADS) bw[i] = a.bin_w[i];
  const float2* Xp = reinterpret_cast<const float2*>(a.X) + (b * a.width + t0) * a.n_freq;
  for (int i = tid; i < nt * a.n_freq; i += LF_THREADS) {
    const int t = i / a.n_freq, f = i % a.n_freq;
    const float2 x = Xp[i];
    ax[f * LF_TS + t] = sqrtf(x.x * x.x + x.y * x.y);
  }
  const int ntile = a.n_mels * LF_TT;
  for (int i = tid; i < ntile; i += LF_THREADS) {
    const int m = i / LF_TT, t = i % LF_TT;
    den[i] = t < nt ? a.mel[(b * a.n_mels + m) * a.width + t0 + t] + a.eps : 1.f;
  }
  for (int c = 0; c < a.C; ++c) {
    const float* R = a.R + (b * a.C + c) * (int64_t)a.n_mels * a.width;
    float* out = a.out + (b * a.C + c) * (int64_t)a.n_freq * a.width;
    __syncthreads();                                   // tables and tiles ready / previous map's q consumed
    for (int i = tid; i < ntile; i += LF_THREADS) {
      const int m = i / LF_TT, t = i % LF_TT;
      q[i] = t < nt ? R[(int64_t)m * a.width + t0 + t] / den[i] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < a.n_freq * LF_TT; i += LF_THREADS) {
      const int f = i / LF_TT, t = i % LF_TT;
      if (t >= nt) continue;
      const float* wf = bw + boff[f];
      const float* qf = q + blo[f] * LF_TT + t;
      float acc = 0.f;
      for (int j = 0; j < bn[f]; ++j) acc = fmaf(wf[j], qf[j * LF_TT], acc);
      out[(int64_t)f * a.width + t0 + t] = ax[f * LF_TS + t] * acc;
    }
  }
}

// ===========================================================================
// Large mask: heatmap_mask_kernel (audiogen.hip) with the map in global memory.
//   select   the same 4 x 8-bit radix select on the bits of relu(h), read from global memory (the
//            map is L2-resident); integer LDS counters, so the threshold does not depend on order
//   blur     on 64 x 64 output tiles: the thresholded values of the tile and its reflect-resolved
//            halo go to LDS, then the horizontal sums s = fmaf(taps[dx], v, s) (dx ascending) of
//            every halo row, then acc = fmaf(taps[dy], s, acc) (dy ascending): the LDS kernel's
//            arithmetic in its order, each horizontal sum computed once instead of k times
// A map's tiles are shared by `split` workgroups; each finds the threshold for itself (the same
// integer), so no workgroup waits for another one.
// ===========================================================================
constexpr int ML_THREADS = 1024;
constexpr int ML_LOADS = 8;              // independent global loads a thread issues before it uses them
constexpr int ML_TILE = 64;
constexpr int64_t ML_MAX_N = 1LL << 22;  // largest H*W (include/drsa_amd.h states it)
// Counter copies per histogram bucket, taken by lane & 15 and laid out [bucket][copy]: the lanes of a
// wave that hit one bucket (a map's values share a few exponents) spread over 16 banks, not one address.
constexpr int ML_REP = 16;

struct MaskLargeArgs {
  const float* h;
  float* out;
  const float* taps;
  int H, W, k, group, lo_first, lo_rest, split, tiles_x, ntiles;
};

__global__ __launch_bounds__(ML_THREADS) void heatmap_mask_large_kernel(MaskLargeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x;
  const int r = a.k >> 1, TS = ML_TILE + 2 * r;        // side of a tile with its halo
  const int n = a.H * a.W;
  float* tile = sm;                                    // [TS][TS]
  float* hs = tile + ((TS * TS + 3) & ~3);             // [TS][ML_TILE] horizontal sums
  float* taps = hs + TS * ML_TILE;                     // [k]
  unsigned* hist = reinterpret_cast<unsigned*>(taps + ((a.k + 3) & ~3));   // [256][ML_REP]
  unsigned* hsum = hist + 256 * ML_REP;                // [256] a bucket's copies summed
  const int64_t map = blockIdx.x / a.split;
  const int part = blockIdx.x % a.split;
  const float* h = a.h + map * n;
  float* o = a.out + map * n;
  const int lo = (map % a.group == 0) ? a.lo_first : a.lo_rest;

  for (int i = tid; i < a.k; i += ML_THREADS) taps[i] = a.taps[i];
  unsigned prefix = 0;
  if (lo >= 0) {
    int kk = lo;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      __syncthreads();                                 // previous scan done
      for (int i = tid; i < 256 * ML_REP; i += ML_THREADS) hist[i] = 0;
      __syncthreads();
      // a pass is bound by L2 latency: ML_LOADS loads in flight per thread (index clamped, so that no
      // load sits behind a branch), then the counters
      for (int i0 = tid; i0 < n; i0 += ML_THREADS * ML_LOADS) {
        float x[ML_LOADS];
#pragma unroll
        for (int q = 0; q < ML_LOADS; ++q) x[q] = h[min(i0 + q * ML_THREADS, n - 1)];
#pragma unroll
        for (int q = 0; q < ML_LOADS; ++q) {
          const unsigned u = __float_as_uint(x[q] > 0.f ? x[q] : 0.f);
          if (i0 + q * ML_THREADS < n && (pass == 0 || (u >> (shift + 8)) == (prefix >> (shift + 8))))
            atomicAdd(&hist[((u >> shift) & 255u) * ML_REP + (tid & (ML_REP - 1))], 1u);
        }
      }
      __syncthreads();
      if (tid < 256) {
        unsigned c = 0;
        for (int q = 0; q < ML_REP; ++q) c += hist[tid * ML_REP + ((q + tid) & (ML_REP - 1))];
        hsum[tid] = c;
      }
      __syncthreads();
      // the bucket that holds rank kk (the counted elements are more than kk, so there is one):
      // four buckets per LDS read, then the place inside the four
      int cum = 0, d = 0;
      for (; d < 252; d += 4) {
        const uint4 c = *reinterpret_cast<const uint4*>(hsum + d);
        const int s4 = (int)(c.x + c.y + c.z + c.w);
        if (kk < cum + s4) break;
        cum += s4;
      }
      for (int e = d + 3; d < e; ++d) {
        const int c = (int)hsum[d];
        if (kk < cum + c) break;
        cum += c;
      }
      prefix |= (unsigned)d << shift;
      kk -= cum;
    }
  }
  for (int tl = part; tl < a.ntiles; tl += a.split) {
    const int y0 = (tl / a.tiles_x) * ML_TILE, x0 = (tl % a.tiles_x) * ML_TILE;
    const int th = min(ML_TILE, a.H - y0), tw = min(ML_TILE, a.W - x0);
    const int hw = tw + 2 * r;
    __syncthreads();                                   // taps loaded / previous tile's sums consumed
    const int nh = (th + 2 * r) * hw;
    for (int i0 = tid; i0 < nh; i0 += ML_THREADS * ML_LOADS) {
      float x[ML_LOADS];
#pragma unroll
      for (int q = 0; q < ML_LOADS; ++q) {
        const int i = min(i0 + q * ML_THREADS, nh - 1);
        x[q] = h[reflect_index(y0 - r + i / hw, a.H) * a.W + reflect_index(x0 - r + i % hw, a.W)];
      }
#pragma unroll
      for (int q = 0; q < ML_LOADS; ++q) {
        const int i = i0 + q * ML_THREADS;
        float v = x[q] > 0.f ? x[q] : 0.f;
        if (lo >= 0 && !(__float_as_uint(v) > prefix)) v = 0.f;
        if (i < nh) tile[(i / hw) * TS + i % hw] = v;
      }
    }
    __syncthreads();
    for (int i = tid; i < (th + 2 * r) * tw; i += ML_THREADS) {
      const int ty = i / tw, x = i % tw;
      const float* row = tile + ty * TS + x;
      float s = 0.f;
      for (int dx = 0; dx < a.k; ++dx) s = fmaf(taps[dx], row[dx], s);
      hs[ty * ML_TILE + x] = s;
    }
    __syncthreads();
    for (int i = tid; i < th * tw; i += ML_THREADS) {
      const int y = i / tw, x = i % tw;
      const float* col = hs + y * ML_TILE + x;
      float acc = 0.f;
      for (int dy = 0; dy < a.k; ++dy) acc = fmaf(taps[dy], col[dy * ML_TILE], acc);
      o[(y0 + y) * a.W + x0 + x] = acc;
    }
  }
}

// ===========================================================================
// Synthesis: audio_synth.h's spans (one workgroup per (source, span), one wave per frame of the
// SY_TF-frame tile) with the frames' bins taken from the spectrum directly:
//   Y[t][f] = mask_c[f][t] * X[t][f]   (the mask tile is transposed through LDS)
//   ->  synth_frame  ->  overlap_add_span
// ===========================================================================
constexpr int SY_MS = SY_TF + 1;        // row stride of the mask tile

struct StftSynArgs {
  SynGeom g;
  const float* mask;         // [n][C][n_freq][width]
  int o_mask;
};

__global__ __launch_bounds__(SY_THREADS) void stft_mask_to_audio_kernel(StftSynArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const SynSpan s = synth_span(a.g, sm);
  const int64_t b = s.b;
  const int t0 = s.t0, width = a.g.width;
  const int M = a.g.nfft >> 1, nfreq = M + 1;
  float* mk = sm + a.o_mask;                           // [n_freq][SY_MS]

  synth_fill_tables(a.g, s, tid);

  for (int c = 0; c < a.g.C; ++c) {
    const float* mask = a.mask + (b * a.g.C + c) * (int64_t)nfreq * width;
    __syncthreads();                                   // tables ready / previous audio done
    for (int i = tid; i < nfreq * SY_TF; i += SY_THREADS) {
      const int f = i / SY_TF, tl = i % SY_TF, t = t0 + tl;
      mk[f * SY_MS + tl] = (t >= 0 && t < width) ? mask[(int64_t)f * width + t] : 0.f;
    }
    __syncthreads();
    // ---- wave w: masked spectrum of frame t0 + w -> windowed time frame ----
    if (const int tl = w, t = t0 + w; t >= 0 && t < width) {
      const float2* Xp = reinterpret_cast<const float2*>(a.g.X) + (b * width + t) * nfreq;
      synth_frame(a.g, s, tl, [&](int k) -> cf {
        const float2 X = Xp[k];
        const float m = mk[k * SY_MS + tl];
        return {m * X.x, m * X.y};
      }, lane);
    }
    __syncthreads();
    overlap_add_span(a.g, s, c, tid);
  }
}

}  // namespace

extern "C" int drsa_amd_mel_relevance_to_stft(const float* relevance, const float* mel, const float* X, int64_t n_src,
                                              int C, int n_mels, int width, int n_freq, const int* bin_lo,
                                              const int* bin_n, const int* bin_off, const float* bin_w, int bin_nnz,
                                              float eps, float* out, void* stream) {
  DRSA_REQUIRE(relevance && mel && X && bin_lo && bin_n && bin_off && bin_w && out,
               "mel_relevance_to_stft: null pointer");
  DRSA_REQUIRE(n_src >= 0 && C >= 1 && n_mels >= 1 && width >= 1 && n_freq >= 1 && bin_nnz >= 0,
               "mel_relevance_to_stft: bad n_src/C/n_mels/width/n_freq/bin_nnz");
  DRSA_REQUIRE(eps > 0.f && eps < INFINITY, "mel_relevance_to_stft: eps must be positive and finite (it keeps "
               "R / (mel + eps) finite where mel = 0), got %g", (double)eps);
  DRSA_REQUIRE(aligned8(X), "mel_relevance_to_stft: X is read as (re, im) pairs and must be 8-byte aligned");
  LiftArgs a{};
  const int nblk = (width + LF_TT - 1) / LF_TT;
  DRSA_REQUIRE(n_src * nblk < (1LL << 31), "mel_relevance_to_stft: too many sources");
  LdsCarve lds;
  a.o_ax = lds.take((int64_t)n_freq * LF_TS);
  a.o_den = lds.take((int64_t)n_mels * LF_TT);
  a.o_q = lds.take((int64_t)n_mels * LF_TT);
  a.o_lo = lds.take(n_freq);
  a.o_n = lds.take(n_freq);
  a.o_off = lds.take(n_freq);
  a.o_w = lds.take(bin_nnz);
  const size_t smem = lds.bytes();
  if (smem > DRSA_LDS_MAX) {
    drsa::set_error("mel_relevance_to_stft: LDS footprint %zu B exceeds 160 KB (n_freq %d, n_mels %d)", smem, n_freq,
                    n_mels);
    return DRSA_EUNSUPPORTED;
  }
  if (n_src == 0) return DRSA_OK;
  a.R = relevance;
  a.mel = mel;
  a.X = X;
  a.bin_lo = bin_lo;
  a.bin_n = bin_n;
  a.bin_off = bin_off;
  a.bin_w = bin_w;
  a.out = out;
  a.C = C;
  a.n_mels = n_mels;
  a.width = width;
  a.n_freq = n_freq;
  a.nnz = bin_nnz;
  a.nblk = nblk;
  a.eps = eps;
  DRSA_SMEM(mel_relevance_to_stft_kernel, smem);
  hipLaunchKernelGGL(mel_relevance_to_stft_kernel, dim3((unsigned)(n_src * nblk)), dim3(LF_THREADS), smem,
                     (hipStream_t)stream, a);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

extern "C" int drsa_amd_heatmap_mask_large(const float* heatmaps, int64_t n_maps, int H, int W, int group,
                                           int rank_first, int rank_rest, const float* taps, int k, float* mask,
                                           void* stream) {
  if (int rc = check_mask_args("heatmap_mask_large", heatmaps, n_maps, H, W, group, rank_first, rank_rest, taps, k,
                               mask))
    return rc;
  if ((int64_t)H * W > ML_MAX_N) {
    drsa::set_error("heatmap_mask_large: a %dx%d map has more than %lld elements", H, W, (long long)ML_MAX_N);
    return DRSA_EUNSUPPORTED;
  }
  if (n_maps == 0) return DRSA_OK;
  MaskLargeArgs a{heatmaps, mask, taps, H, W, k, group, rank_first, rank_rest};
  a.tiles_x = (W + ML_TILE - 1) / ML_TILE;
  a.ntiles = a.tiles_x * ((H + ML_TILE - 1) / ML_TILE);
  // with fewer maps than CUs a map's tiles are spread over `split` workgroups (each repeats the select)
  const int64_t want = drsa::cu_count() / n_maps;
  a.split = (int)(want < 1 ? 1 : (want > a.ntiles ? a.ntiles : want));
  DRSA_REQUIRE(n_maps * a.split < (1LL << 31), "heatmap_mask_large: too many maps");
  const int TS = ML_TILE + 2 * (k / 2);
  const size_t smem = ((size_t)((TS * TS + 3) & ~3) + (size_t)TS * ML_TILE + ((k + 3) & ~3) + 256 * (ML_REP + 1)) * 4;
  DRSA_SMEM(heatmap_mask_large_kernel, smem);
  hipLaunchKernelGGL(heatmap_mask_large_kernel, dim3((unsigned)(n_maps * a.split)), dim3(ML_THREADS), smem,
                     (hipStream_t)stream, a);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

extern "C" int drsa_amd_stft_mask_to_audio(const float* X, const float* mask, int64_t n_src, int C, int n_fft, int hop,
                                           int width, const float* window, const float* envelope, float* audio,
                                           void* stream) {
  DRSA_REQUIRE(X && mask && window && envelope && audio, "stft_mask_to_audio: null pointer");
  StftSynArgs a{};
  LdsCarve lds;
  // no mel bands and no power here: the shape rules see values that pass
  if (int rc = synth_plan("stft_mask_to_audio", a.g, lds, X, n_src, C, n_fft, hop, /*n_mels=*/1, width, /*power=*/1,
                          window, envelope, audio))
    return rc;
  a.mask = mask;
  a.o_mask = lds.take((int64_t)(n_fft / 2 + 1) * SY_MS);
  synth_take_fft(a.g, lds);
  const size_t smem = lds.bytes();
  if (smem > DRSA_LDS_MAX) {
    drsa::set_error("stft_mask_to_audio: LDS footprint %zu B exceeds 160 KB (n_fft %d)", smem, n_fft);
    return DRSA_EUNSUPPORTED;
  }
  if (n_src == 0) return DRSA_OK;
  DRSA_SMEM(stft_mask_to_audio_kernel, smem);
  hipLaunchKernelGGL(stft_mask_to_audio_kernel, dim3((unsigned)(n_src * a.g.nspan)), dim3(SY_THREADS), smem,
                     (hipStream_t)stream, a);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}
