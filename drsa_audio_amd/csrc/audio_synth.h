// What the concept-audio entries of audiogen.hip and stft_audio.hip share beside the transform
// (stockham.h): the argument checks of the FFT and mask entries, and the back half of the two
// synthesis kernels (mel_to_audio_kernel, stft_mask_to_audio_kernel).
//
// Synthesis: one workgroup per (source, span of G hops of padded output positions), one wave per
// frame.  The workgroup computes the SY_TF = G + extra frames that touch its span, for each of the
// source's C masks in turn; each kernel forms the frame's bins Y(k) its own way, the rest is here:
//   Y -> n_fft-point inverse real FFT -> * window / n_fft   (inverse_real_frame; the windowed frame
//                                                            goes to the wave's free ping-pong buffer)
//   out[p] = (sum over the frames t that cover p, ascending t) / envelope[p]   (overlap_add_span)
// Each output sample is written by exactly one workgroup with a fixed summation order.
#pragma once

#include "common.h"
#include "stockham.h"

namespace {

constexpr int SY_TF = 16;               // frames per workgroup, one wave each
constexpr int SY_THREADS = SY_TF * 64;

inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// common shape rules of the transforms
inline int check_fft_shape(const char* who, int n_fft, int hop, int n_mels, int width, int power, int* radix,
                           int* n_stages) {
  DRSA_REQUIRE(n_fft >= 8 && n_fft % 2 == 0, "%s: n_fft must be even and >= 8 (got %d)", who, n_fft);
  DRSA_REQUIRE(hop >= 1 && n_mels >= 1 && width >= 1, "%s: bad hop/n_mels/width", who);
  DRSA_REQUIRE(hop <= n_fft, "%s: hop %d > n_fft %d leaves gaps between frames", who, hop, n_fft);
  DRSA_REQUIRE(power == 1 || power == 2, "%s: power must be 1 or 2 (got %d)", who, power);
  *n_stages = factor_radices(n_fft / 2, radix);
  DRSA_REQUIRE(*n_stages > 0, "%s: n_fft/2 = %d must factor into 2, 3, 5", who, n_fft / 2);
  return DRSA_OK;
}

// common rules of the two mask entries
inline int check_mask_args(const char* who, const float* heatmaps, int64_t n_maps, int H, int W, int group,
                           int rank_first, int rank_rest, const float* taps, int k, const float* mask) {
  DRSA_REQUIRE(heatmaps && taps && mask, "%s: null pointer", who);
  DRSA_REQUIRE(n_maps >= 0 && n_maps < (1LL << 31) && H >= 1 && W >= 1 && group >= 1, "%s: bad n_maps/H/W/group", who);
  DRSA_REQUIRE(k >= 1 && k % 2 == 1 && k <= 63, "%s: blur kernel size must be odd and in [1, 63] (got %d)", who, k);
  DRSA_REQUIRE(k / 2 < H && k / 2 < W, "%s: reflect padding %d needs a larger map than %dx%d", who, k / 2, H, W);
  const int64_t n = (int64_t)H * W;
  DRSA_REQUIRE(rank_first >= -1 && rank_first < n && rank_rest >= -1 && rank_rest < n,
               "%s: rank must be -1 (no threshold) or in [0, H*W)", who);
  return DRSA_OK;
}

// The part of a synthesis kernel's arguments that both kernels have.
struct SynGeom {
  const float* X;            // [n][width][n_freq] complex
  const float* window;       // [nfft]
  const float* wss;          // [outlen] window envelope over the kept span
  float* out;                // [n][C][outlen]
  int C, nfft, hop, width;
  int n_stages;
  int radix[LM_MAX_STAGES];
  int G, extra, nspan, outlen;
  int o_tw, o_ptw, o_win, o_fft;   // LDS offsets (floats); the kernel's own tiles lie between o_win and o_fft
};

// Checks what the two synthesis entries have in common, fills g but o_fft, and takes the tables from
// the carve.  The entry takes its own tiles next, then synth_take_fft.
inline int synth_plan(const char* who, SynGeom& g, LdsCarve& lds, const float* X, int64_t n_src, int C, int n_fft,
                      int hop, int n_mels, int width, int power, const float* window, const float* envelope,
                      float* audio) {
  if (int rc = check_fft_shape(who, n_fft, hop, n_mels, width, power, g.radix, &g.n_stages)) return rc;
  DRSA_REQUIRE(n_src >= 0 && C >= 1 && width >= 2, "%s: need n_src >= 0, C >= 1, width >= 2", who);
  DRSA_REQUIRE(aligned8(X), "%s: X is read as (re, im) pairs and must be 8-byte aligned", who);
  const int extra = (n_fft + hop - 1) / hop - 1;       // earlier frames that reach into a span
  if (extra > SY_TF / 2) {
    drsa::set_error("%s: n_fft/hop = %d/%d overlaps more than %d frames", who, n_fft, hop, SY_TF / 2 + 1);
    return DRSA_EUNSUPPORTED;
  }
  const int M = n_fft / 2;
  g.X = X;
  g.window = window;
  g.wss = envelope;
  g.out = audio;
  g.C = C;
  g.nfft = n_fft;
  g.hop = hop;
  g.width = width;
  g.extra = extra;
  g.G = SY_TF - extra;
  const int64_t outlen = (int64_t)hop * (width - 1);
  DRSA_REQUIRE(outlen + n_fft < (1LL << 30), "%s: audio too long", who);
  g.outlen = (int)outlen;
  g.nspan = (int)((M + outlen + (int64_t)g.G * hop - 1) / ((int64_t)g.G * hop));
  DRSA_REQUIRE(n_src * g.nspan < (1LL << 31), "%s: too many sources", who);
  g.o_tw = lds.take(2 * M);
  g.o_ptw = lds.take(2 * (M + 1));
  g.o_win = lds.take(n_fft);
  return DRSA_OK;
}

// the waves' ping-pong buffers: the last buffer of both layouts
inline void synth_take_fft(SynGeom& g, LdsCarve& lds) { g.o_fft = lds.take((int64_t)SY_TF * 2 * g.nfft); }

// A workgroup's place: source b, span g, and its LDS buffers.
struct SynSpan {
  int64_t b;
  int g;
  int t0;                    // first frame of the tile (may be < 0)
  int p_lo, p_hi;            // the padded output positions this workgroup owns
  cf* tw;
  cf* ptw;
  float* win;
  cf* fa;                    // this wave's ping-pong buffers
  cf* fb;
  float* fr;                 // windowed frame tl of the tile is at fr + tl * 2 n_fft
  float invN;
};

__device__ __forceinline__ SynSpan synth_span(const SynGeom& a, float* sm) {
  const int M = a.nfft >> 1, half = a.nfft >> 1;
  SynSpan s;
  s.b = blockIdx.x / a.nspan;
  s.g = blockIdx.x % a.nspan;
  s.t0 = s.g * a.G - a.extra;
  s.tw = reinterpret_cast<cf*>(sm + a.o_tw);
  s.ptw = reinterpret_cast<cf*>(sm + a.o_ptw);
  s.win = sm + a.o_win;
  s.fa = reinterpret_cast<cf*>(sm + a.o_fft) + (size_t)wave_id() * 2 * M;
  s.fb = s.fa + M;
  // the transform of an even number of passes ends in fa, so the windowed frame (n_fft floats = one
  // buffer) goes to fb, and the other way round
  s.fr = sm + a.o_fft + ((a.n_stages & 1) ? 0 : 2 * M);
  s.invN = 1.f / (float)a.nfft;
  s.p_lo = max(s.g * a.G * a.hop, half);
  s.p_hi = min((s.g + 1) * a.G * a.hop, half + a.outlen);
  return s;
}

__device__ __forceinline__ void synth_fill_tables(const SynGeom& a, const SynSpan& s, int tid) {
  fill_twiddles(s.tw, s.ptw, a.nfft >> 1, tid, SY_THREADS);
  for (int i = tid; i < a.nfft; i += SY_THREADS) s.win[i] = a.window[i];
}

// frame tl of the tile from its bins Y(k): the wave's transform, windowed into the tile's frame row
template <class Bins>
__device__ __forceinline__ void synth_frame(const SynGeom& a, const SynSpan& s, int tl, Bins Y, int lane) {
  inverse_real_frame(Y, s.fa, s.fb, s.fr + tl * 2 * a.nfft, s.tw, s.ptw, s.win, s.invN, a.nfft >> 1, a.n_stages,
                     a.radix, lane);
}

// the owned overlap-add of audio c of the source over this workgroup's span (all frames written)
__device__ __forceinline__ void overlap_add_span(const SynGeom& a, const SynSpan& s, int c, int tid) {
  const int half = a.nfft >> 1;
  float* out = a.out + (s.b * a.C + c) * (int64_t)a.outlen;
  for (int p = s.p_lo + tid; p < s.p_hi; p += SY_THREADS) {
    float acc = 0.f;
    const int t_hi = p / a.hop;                        // the last frame that starts at or before p
    for (int t = t_hi - a.extra; t <= t_hi; ++t) {     // ascending t: the fixed summation order
      const int off = p - t * a.hop;
      if (t >= 0 && t < a.width && off < a.nfft) acc += s.fr[(t - s.t0) * 2 * a.nfft + off];
    }
    out[p - half] = acc / a.wss[p - half];
  }
}

}  // namespace
