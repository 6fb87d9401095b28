// Concept audio back end: heatmaps -> waveforms (reference cxai/xai/explain/audiogen.py,
// Mel2Audio.make_audios; DESIGN.md "Concept audio").  Four launches:
//
//   drsa_amd_stft_mel_phase   chunk -> linear mel |X|^power [n][n_mels][width] and the complex
//                             spectrum X [n][width][n_freq] of frames frame0..frame0+width-1
//                             (frame-major: a frame's bins are contiguous for the synthesis)
//   drsa_amd_heatmap_mask     relu -> rank threshold (on-chip radix select) -> Gaussian blur
//   drsa_amd_mel_to_audio     masked mel -> relu(P m)^(1/power) -> x phase -> inverse real FFT ->
//                             window -> owned overlap-add -> / window envelope -> trimmed audio
//   drsa_amd_audio_normalize  peak normalisation + volume matching (needs a whole audio's
//                             maximum, hence its own small pass)
//
// drsa_amd_istft_envelope is host code: the window's overlap-added sum of squares over the kept
// span (a plan constant) and the check that it is invertible.
//
// The transforms, forward and inverse, are the wave-local ones of stockham.h.  The argument checks
// and the synthesis's spans, frames and overlap-add are audio_synth.h's, shared with stft_audio.hip:
// mel_to_audio_kernel keeps what is its own, the mel tile, the P m contraction and Y = mag x phase.
#include "audio_synth.h"
#include "common.h"
#include "drsa_amd.h"
#include "stockham.h"

#include <math.h>
#include <stdlib.h>

namespace {

constexpr int AG_WAVES = 8;
constexpr int AG_THREADS = AG_WAVES * 64;
constexpr int AG_TF = 16;               // frames per workgroup (= the MFMA tile's 16 columns)
constexpr int AG_PB = 16;               // blocks of 4 rows of P^T a lane loads ahead of its MFMAs
static_assert(SY_TF == AG_TF, "the synthesis runs one wave per column of the MFMA tile");

// ===========================================================================
// Analysis: one workgroup per (chunk, block of 16 frames), one frame per wave at a time.
// ===========================================================================
struct StftArgs {
  const float* wav;
  int64_t stride;
  int L, nfft, hop, n_mels, width, frame0, power, nblk;
  int n_stages;
  int radix[LM_MAX_STAGES];
  const float* window;
  const int* band_lo;
  const int* band_n;
  const int* band_off;
  const float* band_w;
  int nnz, peak_norm;
  float* mel;                // [n][n_mels][width]
  float* X;                  // [n][width][n_freq] complex (re, im)
  int o_tw, o_ptw, o_win, o_blo, o_bn, o_boff, o_bw, o_fft, o_mel, o_red;
};

__global__ __launch_bounds__(AG_THREADS) void stft_mel_phase_kernel(StftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int chunk = blockIdx.x / a.nblk, tb = (blockIdx.x % a.nblk) * AG_TF;
  const int M = a.nfft >> 1, half = a.nfft >> 1, nfreq = M + 1;
  const float* x = a.wav + (int64_t)chunk * a.stride;
  cf* tw = reinterpret_cast<cf*>(sm + a.o_tw);
  cf* ptw = reinterpret_cast<cf*>(sm + a.o_ptw);
  float* win = sm + a.o_win;
  int* blo = reinterpret_cast<int*>(sm + a.o_blo);
  int* bn = reinterpret_cast<int*>(sm + a.o_bn);
  int* boff = reinterpret_cast<int*>(sm + a.o_boff);
  float* bw = sm + a.o_bw;
  cf* fa = reinterpret_cast<cf*>(sm + a.o_fft) + (size_t)w * 2 * M;
  cf* fb = fa + M;
  float* melt = sm + a.o_mel;                        // [n_mels][AG_TF]
  float* red = sm + a.o_red;

  fill_twiddles(tw, ptw, M, tid, AG_THREADS);
  for (int i = tid; i < a.nfft; i += AG_THREADS) win[i] = a.window[i];
  for (int m = tid; m < a.n_mels; m += AG_THREADS) {
    blo[m] = a.band_lo[m];
    bn[m] = a.band_n[m];
    boff[m] = a.band_off[m];
  }
  for (int i = tid; i < a.nnz; i += AG_THREADS) bw[i] = a.band_w[i];
  // peak_normalizer: the chunk's samples are divided by its peak on the load, as the reference
  // divides the waveform before the transform (every workgroup of the chunk finds the same maximum)
  float pk = 1.f;
  if (a.peak_norm) {
    float p = 0.f;
    for (int i = tid; i < a.L; i += AG_THREADS) p = fmaxf(p, fabsf(x[i]));
    for (int o = 32; o > 0; o >>= 1) p = fmaxf(p, shfl_xor(p, o));
    if (lane == 0) red[w] = p;
    __syncthreads();
    pk = red[0];
    for (int i = 1; i < AG_WAVES; ++i) pk = fmaxf(pk, red[i]);
  }
  __syncthreads();

  for (int tl = w; tl < AG_TF; tl += AG_WAVES) {
    const int t = tb + tl;
    if (t >= a.width) break;
    const int base = (a.frame0 + t) * a.hop - half;
    for (int n = lane; n < M; n += 64) {
      const int j = base + 2 * n;
      fa[n] = {(x[reflect_index(j, a.L)] / pk) * win[2 * n], (x[reflect_index(j + 1, a.L)] / pk) * win[2 * n + 1]};
    }
    wave_lds_sync();
    cf* src = stockham_fft(fa, fb, tw, M, a.n_stages, a.radix, lane);
    float* mag = reinterpret_cast<float*>(src == fa ? fb : fa);
    float2* Xo = reinterpret_cast<float2*>(a.X) + ((int64_t)chunk * a.width + t) * nfreq;
    for (int k = lane; k <= M; k += 64) {
      const cf X = real_split(src, ptw, k, M);
      Xo[k] = make_float2(X.x, X.y);
      const float p2 = X.x * X.x + X.y * X.y;
      mag[k] = a.power == 2 ? p2 : sqrtf(p2);
    }
    wave_lds_sync();
    for (int m = lane; m < a.n_mels; m += 64) {
      const float* wm = bw + boff[m];
      const float* mg = mag + blo[m];
      float acc = 0.f;
      for (int q = 0; q < bn[m]; ++q) acc = fmaf(wm[q], mg[q], acc);
      melt[m * AG_TF + tl] = acc;
    }
    wave_lds_sync();                                   // mag is consumed before the next frame is packed
  }
  __syncthreads();
  for (int i = tid; i < a.n_mels * AG_TF; i += AG_THREADS) {
    const int m = i / AG_TF, t = tb + i % AG_TF;
    if (t < a.width) a.mel[((int64_t)chunk * a.n_mels + m) * a.width + t] = melt[i];
  }
}

// ===========================================================================
// Mask: one workgroup per map, the map in LDS.
//   hp = relu(h); keep hp > a[lo] (a = sorted hp, lo = floor(p/100 (n-1))): np.percentile's linear
//   interpolation lies in [a[lo], a[lo+1]) for a fractional rank and equals a[lo] for a whole one,
//   so "hp > percentile" is "hp > a[lo]" in both cases.  a[lo] by a 4 x 8-bit radix select on the
//   float bits (hp >= 0: bit order = value order; integer LDS counters, so order-free).
//   Blur: torchvision GaussianBlur, separable taps, reflect padding; the horizontal sums are
//   recomputed per output row so the map needs no second LDS copy.
// ===========================================================================
struct MaskArgs {
  const float* h;
  float* out;
  const float* taps;
  int H, W, k, group, lo_first, lo_rest;
};

__global__ __launch_bounds__(AG_THREADS) void heatmap_mask_kernel(MaskArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x;
  const int n = a.H * a.W;
  float* v = sm;                                       // [n]
  float* taps = sm + ((n + 3) & ~3);                   // [k]
  unsigned* hist = reinterpret_cast<unsigned*>(taps + ((a.k + 3) & ~3));   // [256]
  const int64_t map = blockIdx.x;
  const float* h = a.h + map * n;
  const int lo = (map % a.group == 0) ? a.lo_first : a.lo_rest;

  for (int i = tid; i < a.k; i += AG_THREADS) taps[i] = a.taps[i];
  for (int i = tid; i < n; i += AG_THREADS) {
    const float x = h[i];
    v[i] = x > 0.f ? x : 0.f;
  }
  if (lo >= 0) {
    unsigned prefix = 0;
    int kk = lo;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      __syncthreads();                                 // map loaded / previous scan done
      for (int i = tid; i < 256; i += AG_THREADS) hist[i] = 0;
      __syncthreads();
      for (int i = tid; i < n; i += AG_THREADS) {
        const unsigned u = __float_as_uint(v[i]);
        if (pass == 0 || (u >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(u >> shift) & 255u], 1u);
      }
      __syncthreads();
      int cum = 0, d = 0;
      for (; d < 255; ++d) {
        const int c = (int)hist[d];
        if (kk < cum + c) break;
        cum += c;
      }
      prefix |= (unsigned)d << shift;
      kk -= cum;
    }
    __syncthreads();
    for (int i = tid; i < n; i += AG_THREADS)
      if (!(__float_as_uint(v[i]) > prefix)) v[i] = 0.f;
  }
  __syncthreads();
  const int r = a.k >> 1;
  float* o = a.out + map * n;
  for (int i = tid; i < n; i += AG_THREADS) {
    const int y = i / a.W, xx = i % a.W;
    float acc = 0.f;
    for (int dy = 0; dy < a.k; ++dy) {
      const float* row = v + reflect_index(y + dy - r, a.H) * a.W;
      float s = 0.f;
      for (int dx = 0; dx < a.k; ++dx) s = fmaf(taps[dx], row[reflect_index(xx + dx - r, a.W)], s);
      acc = fmaf(taps[dy], s, acc);
    }
    o[i] = acc;
  }
}

// ===========================================================================
// Synthesis: audio_synth.h's spans (one workgroup per (source, span), one wave per frame of the
// AG_TF-frame tile) with the frames' bins from the masked mel, for each of the source's C masks:
//   m[j][t]   = mel[j][t] * mask_c[j][t]                         (LDS, the mel tile is loaded once)
//   mag[t][f] = relu(sum_j P[f][j] m[j][t])^(1/power)            (fp32 MFMA 16x16x4: 16 bins x 16 frames,
//                                                                 two k-ordered fma chains over j)
//   Y = mag * X / |X|  ->  synth_frame  ->  overlap_add_span
// ===========================================================================
struct SynArgs {
  SynGeom g;
  const float* mel;          // [n][n_mels][width]
  const float* mask;         // [n][C][n_mels][width]
  const float* pinv_t;       // [n_mels][n_freq]: P transposed
  int n_mels, power;
  int njb;                   // blocks of 4 mel rows, even (zero rows pad the m tile)
  int FS;                    // mag row stride: n_freq rounded up to 16
  int o_melt, o_m, o_mag;
};

__global__ __launch_bounds__(SY_THREADS) void mel_to_audio_kernel(SynArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const SynSpan s = synth_span(a.g, sm);
  const int64_t b = s.b;
  const int t0 = s.t0, width = a.g.width;
  const int M = a.g.nfft >> 1, nfreq = M + 1;
  float* melt = sm + a.o_melt;                         // [4 njb][AG_TF]
  float* mt = sm + a.o_m;                              // [4 njb][AG_TF]
  float* mag = sm + a.o_mag;                           // [AG_TF][FS]

  synth_fill_tables(a.g, s, tid);
  const int ntile = a.njb * 4 * AG_TF;
  for (int i = tid; i < ntile; i += SY_THREADS) {
    const int j = i / AG_TF, t = t0 + i % AG_TF;
    const bool ok = j < a.n_mels && t >= 0 && t < width;
    melt[i] = ok ? a.mel[(b * a.n_mels + j) * width + t] : 0.f;
  }

  for (int c = 0; c < a.g.C; ++c) {
    const float* mask = a.mask + (b * a.g.C + c) * (int64_t)a.n_mels * width;
    __syncthreads();                                   // tables + mel tile ready / previous audio done
    for (int i = tid; i < ntile; i += SY_THREADS) {
      const int j = i / AG_TF, t = t0 + i % AG_TF;
      const bool ok = j < a.n_mels && t >= 0 && t < width;
      mt[i] = ok ? melt[i] * mask[(int64_t)j * width + t] : 0.f;
    }
    __syncthreads();
    // ---- mag = relu(P m)^(1/power): wave w takes the 16-bin tiles w, w + 8, ... ----
    for (int f0 = w * 16; f0 < nfreq; f0 += SY_TF * 16) {
      const int fi = min(f0 + (lane & 15), nfreq - 1);
      const int kq = lane >> 4;
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      // P streams from L2: AG_PB row blocks' loads in flight per lane; even blocks chain into
      // acc0, odd ones into acc1, each in ascending j
      for (int jb = 0; jb < a.njb; jb += AG_PB) {
        float av[AG_PB];
#pragma unroll
        for (int u = 0; u < AG_PB; ++u)
          av[u] = a.pinv_t[(int64_t)min((jb + u) * 4 + kq, a.n_mels - 1) * nfreq + fi];
#pragma unroll
        for (int u = 0; u < AG_PB; u += 2) {
          if (jb + u < a.njb) {                        // njb is even: blocks come in pairs
            acc0 = mfma16(av[u], mt[(jb + u) * 64 + lane], acc0);
            acc1 = mfma16(av[u + 1], mt[(jb + u) * 64 + 64 + lane], acc1);
          }
        }
      }
      f32x4 r = acc0 + acc1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float x = r[q] > 0.f ? r[q] : 0.f;
        r[q] = a.power == 2 ? sqrtf(x) : x;
      }
      // lane holds bins f0 + 4 (lane >> 4) + q of frame lane & 15 (rows past n_freq land in the row's padding)
      *reinterpret_cast<f32x4*>(mag + (lane & 15) * a.FS + f0 + 4 * kq) = r;
    }
    __syncthreads();
    // ---- wave w: spectrum of frame t0 + w -> windowed time frame ----
    if (const int tl = w, t = t0 + w; t >= 0 && t < width) {
      const float2* Xp = reinterpret_cast<const float2*>(a.g.X) + (b * width + t) * nfreq;
      const float* mg = mag + tl * a.FS;
      synth_frame(a.g, s, tl, [&](int k) -> cf {
        const float2 X = Xp[k];
        const float n2 = X.x * X.x + X.y * X.y;
        cf ph = {1.f, 0.f};                            // librosa magphase: 1 + 0i where |X| = 0
        if (n2 > 0.f) {
          const float inv = 1.f / sqrtf(n2);
          ph = {X.x * inv, X.y * inv};
        }
        return cscale(ph, mg[k]);
      }, lane);
    }
    __syncthreads();
    overlap_add_span(a.g, s, c, tid);
  }
}

// ===========================================================================
// Normalise: one workgroup per audio.  peak_normalizer, then (wav given) adjust_vol against the
// source waveform: clamp(a * |rms(wav) / rms(a)|, -1, 1).  Sums of squares in fp64, fixed order.
// ===========================================================================
constexpr int AN_THREADS = 256;

__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = AN_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(AN_THREADS) void audio_normalize_kernel(float* audio, int len, const float* wav,
                                                                      int64_t wav_stride, int wav_len, int C) {
  __shared__ double red[AN_THREADS];
  __shared__ float redf[AN_THREADS];
  const int tid = threadIdx.x;
  float* x = audio + (int64_t)blockIdx.x * len;
  float p = 0.f;
  for (int i = tid; i < len; i += AN_THREADS) p = fmaxf(p, fabsf(x[i]));
  redf[tid] = p;
  __syncthreads();
  for (int s = AN_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) redf[tid] = fmaxf(redf[tid], redf[tid + s]);
    __syncthreads();
  }
  const float pk = redf[0];
  float gain = 1.f;
  if (wav) {
    double s2 = 0.0, s1 = 0.0;
    for (int i = tid; i < len; i += AN_THREADS) {
      const float q = x[i] / pk;
      s2 += (double)q * (double)q;
    }
    const float* r = wav + (int64_t)(blockIdx.x / C) * wav_stride;
    for (int i = tid; i < wav_len; i += AN_THREADS) s1 += (double)r[i] * (double)r[i];
    s2 = block_sum(s2, red, tid);
    s1 = block_sum(s1, red, tid);
    gain = fabsf(sqrtf((float)(s1 / wav_len)) / sqrtf((float)(s2 / len)));
  }
  for (int i = tid; i < len; i += AN_THREADS) {
    const float q = x[i] / pk;                         // a silent audio: 0 / 0 = NaN, as the reference
    if (wav) {
      const float y = q * gain;
      x[i] = y < -1.f ? -1.f : (y > 1.f ? 1.f : y);    // torchaudio Vol's clamp (keeps NaN)
    } else {
      x[i] = q;
    }
  }
}

}  // namespace

extern "C" int drsa_amd_stft_mel_phase(const float* wav, int64_t n_chunks, int64_t chunk_stride, int chunk_len,
                                       int n_fft, int hop, int n_mels, int width, int frame0, int power,
                                       const float* window, const int* band_lo, const int* band_n,
                                       const int* band_off, const float* band_w, int band_nnz, int peak_norm,
                                       float* mel, float* X, void* stream) {
  DRSA_REQUIRE(wav && window && band_lo && band_n && band_off && band_w && mel && X,
               "stft_mel_phase: null pointer");
  StftArgs a{};
  if (int rc = check_fft_shape("stft_mel_phase", n_fft, hop, n_mels, width, power, a.radix, &a.n_stages)) return rc;
  DRSA_REQUIRE(aligned8(X), "stft_mel_phase: X is written as (re, im) pairs and must be 8-byte aligned");
  DRSA_REQUIRE(n_chunks >= 0 && frame0 >= 0 && band_nnz >= 0, "stft_mel_phase: bad n_chunks/frame0/band_nnz");
  DRSA_REQUIRE(chunk_len > n_fft / 2, "stft_mel_phase: reflect padding needs chunk_len > n_fft/2");
  DRSA_REQUIRE(frame0 + width <= 1 + chunk_len / hop, "stft_mel_phase: frames %d..%d exceed the %d STFT frames",
               frame0, frame0 + width - 1, 1 + chunk_len / hop);
  if (n_chunks == 0) return DRSA_OK;
  const int nblk = (width + AG_TF - 1) / AG_TF;
  DRSA_REQUIRE(n_chunks * nblk < (1LL << 31), "stft_mel_phase: too many chunks");
  a.wav = wav;
  a.stride = chunk_stride;
  a.L = chunk_len;
  a.nfft = n_fft;
  a.hop = hop;
  a.n_mels = n_mels;
  a.width = width;
  a.frame0 = frame0;
  a.power = power;
  a.nblk = nblk;
  a.window = window;
  a.band_lo = band_lo;
  a.band_n = band_n;
  a.band_off = band_off;
  a.band_w = band_w;
  a.nnz = band_nnz;
  a.peak_norm = peak_norm;
  a.mel = mel;
  a.X = X;
  const int M = n_fft / 2;
  LdsCarve lds;
  a.o_tw = lds.take(2 * M);
  a.o_ptw = lds.take(2 * (M + 1));
  a.o_win = lds.take(n_fft);
  a.o_blo = lds.take(n_mels);
  a.o_bn = lds.take(n_mels);
  a.o_boff = lds.take(n_mels);
  a.o_bw = lds.take(band_nnz);
  a.o_fft = lds.take(AG_WAVES * 4 * M);
  a.o_mel = lds.take(n_mels * AG_TF);
  a.o_red = lds.take(AG_WAVES);
  const size_t smem = lds.bytes();
  if (smem > DRSA_LDS_MAX) {
    drsa::set_error("stft_mel_phase: LDS footprint %zu B exceeds 160 KB (n_fft %d, n_mels %d)", smem, n_fft, n_mels);
    return DRSA_EUNSUPPORTED;
  }
  DRSA_SMEM(stft_mel_phase_kernel, smem);
  hipLaunchKernelGGL(stft_mel_phase_kernel, dim3((unsigned)(n_chunks * nblk)), dim3(AG_THREADS), smem,
                     (hipStream_t)stream, a);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

extern "C" int drsa_amd_heatmap_mask(const float* heatmaps, int64_t n_maps, int H, int W, int group, int rank_first,
                                     int rank_rest, const float* taps, int k, float* mask, void* stream) {
  if (int rc = check_mask_args("heatmap_mask", heatmaps, n_maps, H, W, group, rank_first, rank_rest, taps, k, mask))
    return rc;
  const int64_t n = (int64_t)H * W;
  const size_t smem = ((size_t)((n + 3) & ~3) + ((k + 3) & ~3) + 256) * 4;
  if (smem > DRSA_LDS_MAX) {
    drsa::set_error("heatmap_mask: a %dx%d map (%zu B with its tables) does not fit the 160 KB LDS", H, W, smem);
    return DRSA_EUNSUPPORTED;
  }
  if (n_maps == 0) return DRSA_OK;
  MaskArgs a{heatmaps, mask, taps, H, W, k, group, rank_first, rank_rest};
  DRSA_SMEM(heatmap_mask_kernel, smem);
  hipLaunchKernelGGL(heatmap_mask_kernel, dim3((unsigned)n_maps), dim3(AG_THREADS), smem, (hipStream_t)stream, a);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

extern "C" int drsa_amd_istft_envelope(const float* window_host, int n_fft, int hop, int width, float* envelope_host) {
  DRSA_REQUIRE(window_host && envelope_host, "istft_envelope: null pointer");
  DRSA_REQUIRE(n_fft >= 2 && n_fft % 2 == 0 && hop >= 1 && hop <= n_fft && width >= 2,
               "istft_envelope: need even n_fft, 1 <= hop <= n_fft, width >= 2");
  const int half = n_fft / 2;
  const int64_t outlen = (int64_t)hop * (width - 1);
  double lowest = INFINITY;
  for (int64_t s = 0; s < outlen; ++s) {
    const int64_t p = s + half;
    int64_t t_lo = (p - n_fft) / hop + 1;
    if (p - n_fft < 0) t_lo = 0;
    const int64_t t_hi = p / hop < width - 1 ? p / hop : width - 1;
    double e = 0.0;
    for (int64_t t = t_lo; t <= t_hi; ++t) {
      const double wv = (double)window_host[p - t * hop];
      e += wv * wv;
    }
    envelope_host[s] = (float)e;
    lowest = e < lowest ? e : lowest;
  }
  DRSA_REQUIRE(lowest > 1e-11, "istft_envelope: the window's sum of squares falls to %.3g inside the kept span "
               "(not invertible: NOLA)", lowest);
  return DRSA_OK;
}

extern "C" int drsa_amd_mel_to_audio(const float* mel, const float* X, const float* mask, int64_t n_src, int C,
                                     int n_fft, int hop, int n_mels, int width, int power, const float* window,
                                     const float* pinv_t, const float* envelope, float* audio, void* stream) {
  DRSA_REQUIRE(mel && X && mask && window && pinv_t && envelope && audio, "mel_to_audio: null pointer");
  SynArgs a{};
  LdsCarve lds;
  if (int rc = synth_plan("mel_to_audio", a.g, lds, X, n_src, C, n_fft, hop, n_mels, width, power, window, envelope,
                          audio))
    return rc;
  a.mel = mel;
  a.mask = mask;
  a.pinv_t = pinv_t;
  a.n_mels = n_mels;
  a.power = power;
  a.njb = 2 * ((n_mels + 7) / 8);
  a.FS = 16 * ((n_fft / 2 + 1 + 15) / 16);
  a.o_melt = lds.take(a.njb * 4 * AG_TF);
  a.o_m = lds.take(a.njb * 4 * AG_TF);
  a.o_mag = lds.take(AG_TF * a.FS);
  synth_take_fft(a.g, lds);
  const size_t smem = lds.bytes();
  if (smem > DRSA_LDS_MAX) {
    drsa::set_error("mel_to_audio: LDS footprint %zu B exceeds 160 KB (n_fft %d, n_mels %d)", smem, n_fft, n_mels);
    return DRSA_EUNSUPPORTED;
  }
  if (n_src == 0) return DRSA_OK;
  DRSA_SMEM(mel_to_audio_kernel, smem);
  hipLaunchKernelGGL(mel_to_audio_kernel, dim3((unsigned)(n_src * a.g.nspan)), dim3(SY_THREADS), smem,
                     (hipStream_t)stream, a);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

extern "C" int drsa_amd_audio_normalize(float* audio, int64_t n_audio, int len, const float* wav, int64_t wav_stride,
                                        int wav_len, int C, void* stream) {
  DRSA_REQUIRE(audio, "audio_normalize: null pointer");
  DRSA_REQUIRE(n_audio >= 0 && n_audio < (1LL << 31) && len >= 1, "audio_normalize: bad n_audio/len");
  DRSA_REQUIRE(!wav || (wav_len >= 1 && C >= 1), "audio_normalize: volume matching needs wav_len >= 1 and C >= 1");
  if (n_audio == 0) return DRSA_OK;
  hipLaunchKernelGGL(audio_normalize_kernel, dim3((unsigned)n_audio), dim3(AN_THREADS), 0, (hipStream_t)stream, audio,
                     len, wav, wav_stride, wav_len, C);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}
