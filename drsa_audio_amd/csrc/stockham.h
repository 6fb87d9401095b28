// Wave-local real FFT pieces shared by the log-mel front end (logmel.hip) and the audio back end
// (audiogen.hip, stft_audio.hip; audio_synth.h): complex helpers, the twiddle tables, forward
// radix-2/3/4/5 butterflies, one Stockham pass over LDS ping-pong buffers and the whole M-point
// transform, the real-input split of the forward n_fft = 2M-point real transform, the inverse real
// transform of one frame (half-length packing, conj(DFT(conj z)), window and 1/n_fft), reflect
// padding, and the host-side radix factoring.  logmel800_kernel has its own tables and transform.
#pragma once

#include "common.h"

namespace {

constexpr int LM_MAX_STAGES = 8;

struct cf {
  float x, y;
};
__device__ __forceinline__ cf cadd(cf a, cf b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cf csub(cf a, cf b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cf cmul(cf a, cf b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cf cscale(cf a, float s) { return {a.x * s, a.y * s}; }
__device__ __forceinline__ cf mul_negi(cf a) { return {a.y, -a.x}; }   // -i * a

// Wave-local LDS hand-off: all lanes' LDS writes are visible to the wave's later reads.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// twiddle tables from exact fp64 angles rounded once to fp32: tw[j] = W_M^j (j < M), ptw[k] = W_N^k
// (k <= M, N = 2M)
__device__ __forceinline__ void fill_twiddles(cf* tw, cf* ptw, int M, int tid, int nthreads) {
  for (int j = tid; j < M; j += nthreads) {
    double s, c;
    sincospi(2.0 * (double)j / (double)M, &s, &c);
    tw[j] = {(float)c, (float)-s};
  }
  for (int k = tid; k <= M; k += nthreads) {
    double s, c;
    sincospi((double)k / (double)M, &s, &c);
    ptw[k] = {(float)c, (float)-s};
  }
}

// index i of a length-n axis under reflect padding (torch pad_mode="reflect"; -n < i < 2n - 1)
__device__ __forceinline__ int reflect_index(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * (n - 1) - i : i;
}

// forward DFT butterflies (sign -i), in place on v[0..R)
__device__ __forceinline__ void bfly2(cf* v) {
  cf a = v[0], b = v[1];
  v[0] = cadd(a, b);
  v[1] = csub(a, b);
}
__device__ __forceinline__ void bfly4(cf* v) {
  cf t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]);
  cf t2 = cadd(v[1], v[3]), t3 = mul_negi(csub(v[1], v[3]));
  v[0] = cadd(t0, t2);
  v[2] = csub(t0, t2);
  v[1] = cadd(t1, t3);
  v[3] = csub(t1, t3);
}
__device__ __forceinline__ void bfly3(cf* v) {
  const float s = 0.86602540378443864676f;
  cf sm = cadd(v[1], v[2]);
  cf y0 = cadd(v[0], sm);
  cf t = csub(v[0], cscale(sm, 0.5f));
  cf u = mul_negi(cscale(csub(v[1], v[2]), s));
  v[0] = y0;
  v[1] = cadd(t, u);
  v[2] = csub(t, u);
}
__device__ __forceinline__ void bfly5(cf* v) {
  const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;
  const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
  cf b1 = cadd(v[1], v[4]), b2 = cadd(v[2], v[3]);
  cf d1 = csub(v[1], v[4]), d2 = csub(v[2], v[3]);
  cf a0 = v[0];
  cf r1 = cadd(a0, cadd(cscale(b1, c1), cscale(b2, c2)));
  cf r2 = cadd(a0, cadd(cscale(b1, c2), cscale(b2, c1)));
  cf q1 = mul_negi(cadd(cscale(d1, s1), cscale(d2, s2)));   // -i (s1 d1 + s2 d2)
  cf q2 = mul_negi(csub(cscale(d1, s2), cscale(d2, s1)));   // -i (s2 d1 - s1 d2)
  v[0] = cadd(a0, cadd(b1, b2));
  v[1] = cadd(r1, q1);
  v[4] = csub(r1, q1);
  v[2] = cadd(r2, q2);
  v[3] = csub(r2, q2);
}

// One Stockham pass of radix R over M points (Govindaraju et al. 2008 indexing):
//   v[r] = in[j + r*M/R] * W_M^{r*k*M/(Ns*R)}, k = j % Ns;  out[(j/Ns)*Ns*R + k + r*Ns] = DFT_R(v)[r]
template <int R>
__device__ __forceinline__ void stockham_pass(const cf* __restrict__ in, cf* __restrict__ out, const cf* tw, int M,
                                              int Ns, int lane) {
  const int MR = M / R;
  const int tstep = M / (Ns * R);
  for (int j = lane; j < MR; j += 64) {
    const int k = j % Ns;
    cf v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = in[j + r * MR];
    if (Ns > 1) {
#pragma unroll
      for (int r = 1; r < R; ++r) v[r] = cmul(v[r], tw[r * k * tstep]);
    }
    if constexpr (R == 2) bfly2(v);
    if constexpr (R == 3) bfly3(v);
    if constexpr (R == 4) bfly4(v);
    if constexpr (R == 5) bfly5(v);
    const int base = (j / Ns) * Ns * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r) out[base + r * Ns] = v[r];
  }
}

// The whole M-point forward transform of one wave: the passes of `radix` from buffer a to b and
// back.  tw[j] = W_M^j.  Returns the buffer that holds the result (the other one is free).
__device__ __forceinline__ cf* stockham_fft(cf* a, cf* b, const cf* tw, int M, int n_stages, const int* radix,
                                            int lane) {
  cf* src = a;
  cf* dst = b;
  int Ns = 1;
  for (int s = 0; s < n_stages; ++s) {
    const int R = radix[s];
    if (R == 4) stockham_pass<4>(src, dst, tw, M, Ns, lane);
    else if (R == 5) stockham_pass<5>(src, dst, tw, M, Ns, lane);
    else if (R == 3) stockham_pass<3>(src, dst, tw, M, Ns, lane);
    else stockham_pass<2>(src, dst, tw, M, Ns, lane);
    wave_lds_sync();
    Ns *= R;
    cf* t = src;
    src = dst;
    dst = t;
  }
  return src;
}

// Real-input split: bin k <= M of the 2M-point transform of the real frame x, from the M-point
// transform Z of z[n] = x[2n] + i x[2n+1]:
//   X[k] = E[k] + W_N^k O[k],  E = (Z_k + conj Z_{M-k})/2,  O = (Z_k - conj Z_{M-k})/(2i)
__device__ __forceinline__ cf real_split(const cf* Z, const cf* ptw, int k, int M) {
  const cf zk = Z[k == M ? 0 : k];
  const cf zr = Z[k == 0 ? 0 : M - k];
  const cf zc = {zr.x, -zr.y};
  const cf e = cscale(cadd(zk, zc), 0.5f);
  const cf d = csub(zk, zc);
  const cf o = {0.5f * d.y, -0.5f * d.x};
  return cadd(e, cmul(ptw[k], o));
}

// The inverse 2M-point real transform of one wave's frame from its bins Y(k), k <= M, windowed and
// scaled by invN = 1/n_fft into fo[0..2M), the wave's buffer (a or b) that the passes leave free.
// The imaginary parts of Y(0) and Y(M), a real signal's DC and Nyquist bins, are dropped (as irfft
// does).  Half-length packing: z[n] = x[2n] + i x[2n+1] = IDFT_M(Z)/2,
//   Z[k] = (Y[k] + conj Y[M-k]) + i (Y[k] - conj Y[M-k]) conj(W_N^k);   IDFT = conj DFT conj
template <class Bins>
__device__ __forceinline__ void inverse_real_frame(Bins Y, cf* a, cf* b, float* fo, const cf* tw, const cf* ptw,
                                                   const float* win, float invN, int M, int n_stages,
                                                   const int* radix, int lane) {
  for (int k = lane; k < M; k += 64) {
    cf yk = Y(k), ym = Y(M - k);
    if (k == 0) yk.y = ym.y = 0.f;                     // the only k < M that reads bins 0 and M
    const cf yc = {ym.x, -ym.y};
    const cf e = cadd(yk, yc);
    const cf o = cmul(csub(yk, yc), cf{ptw[k].x, -ptw[k].y});
    a[k] = {e.x - o.y, -(e.y + o.x)};
  }
  wave_lds_sync();
  const cf* F = stockham_fft(a, b, tw, M, n_stages, radix, lane);
  for (int n = lane; n < M; n += 64) {
    fo[2 * n] = (F[n].x * invN) * win[2 * n];
    fo[2 * n + 1] = (-F[n].y * invN) * win[2 * n + 1];
  }
}

// M = 2^a 3^b 5^c -> its radices (4s first), or -1
inline int factor_radices(int M, int* r) {
  int n = 0;
  while (M % 4 == 0 && n < LM_MAX_STAGES) { r[n++] = 4; M /= 4; }
  while (M % 2 == 0 && n < LM_MAX_STAGES) { r[n++] = 2; M /= 2; }
  while (M % 3 == 0 && n < LM_MAX_STAGES) { r[n++] = 3; M /= 3; }
  while (M % 5 == 0 && n < LM_MAX_STAGES) { r[n++] = 5; M /= 5; }
  return M == 1 ? n : -1;
}

}  // namespace
