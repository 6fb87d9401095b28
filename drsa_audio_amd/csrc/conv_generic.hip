// K x K 'same' convolution (odd kh, kw <= 7, stride 1, zero padding) on fp32 MFMA
// (v_mfma_f32_32x32x2_f32) for the LRP engine: the forward with the rule's denominator and the rule
// backward of a conv that is not 3x3 (reference create_model.py:17,58: the conv_kernel argument).
//
// The arithmetic is the 3x3 kernels' (lrp_conv_kernel.h) with the tap loops generalised: every output
// is one k-ordered fp32 fma chain from +0, k = (ci * kh + ky) * kw + kx, a pixel off the image an
// operand 0; everything after the accumulator is what drsa_amd_conv_fwd(pool = 0) and
// drsa_amd_conv_bwd(g_amax = NULL) compute, operation for operation.  At kh = kw = 3 the results
// are the bits of those entry points.
//
// GEMM view (the 3x3 kernels' mapping): D[channel][pixel] = W^T[channel][k] X[k][pixel].  A workgroup
// of 4 waves owns an 8 x 16 pixel tile of one sample and one 32-channel slice of the output; wave w
// owns the two tile rows 2w, 2w + 1 (32 pixels: one MFMA column block).  The input channels run in
// chunks of `cic` (even, chosen by the host so that a workgroup's LDS stays near 40 KiB: four
// workgroups per CU at 7x7 with three weight groups): per chunk the (8 + kh - 1) x (16 + kw - 1) halo
// of every channel and the chunk's weight rows [ng][cic * kh * kw][32] are staged in LDS, then each
// k-step pair is one MFMA per weight group.  kh and kw are run-time values: two LDS tables, made
// once per workgroup, turn a chunk-local k into its halo offset and a halo element into its
// (channel, row, column), so no loop divides.
#include "common.h"
#include "convk.h"
#include "drsa_amd.h"
#include "lrp_conv.h"

#include <stdlib.h>

namespace {
using drsa_convk::KArgs;
using drsa_convk::kTH;
using drsa_convk::kTW;
constexpr int kT = 256;

// The backward's epilogue for one output: R = xmode(t0, t1; x), then the post step of the layer below
// (drsa_amd_conv_bwd's expressions: no fma, IEEE division, the modes as uniform selects).
template <int NG>
__device__ __forceinline__ float rule_post(float t0, float t1, float xx, float dd, bool mul_x, bool split_x,
                                           bool post_div, bool post_any, float eps) {
  const float m = split_x ? fmaxf(xx, 0.f) : xx;
  float R = (mul_x ? m : 1.f) * t0;
  if constexpr (NG >= 2) {
    if (split_x) R += fminf(xx, 0.f) * t1;
  }
  const float q = div_nb(R, stab(dd, eps));
  const float yv = post_div ? q : R;
  return (post_any && !(xx > 0.f)) ? 0.f : yv;
}

template <int NG, bool BWD>
__global__ __launch_bounds__(kT) void convk_kernel(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int kh = a.kh, kw = a.kw, ph = kh >> 1, pw = kw >> 1;
  const int HX = kTW + kw - 1, PLANE = (kTH + kh - 1) * HX;
  const int taps = kh * kw, KCM = a.cic * taps;     // k-steps of a full chunk
  float* halo = smem;                               // [cic][PLANE]
  float* wl = halo + a.cic * PLANE;                 // [NG][KCM][32]
  int* ktab = reinterpret_cast<int*>(wl + NG * KCM * 32);   // [KCM]: halo offset of chunk-local k
  int* htab = ktab + KCM;                           // [cic * PLANE]: channel << 16 | row << 8 | column

  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int h = lane >> 5, p = lane & 31;
  const int H = a.H, W = a.W, HW = H * W;
  const int tiles_x = (W + kTW - 1) / kTW;
  const int ty0 = (blockIdx.x / tiles_x) * kTH, tx0 = (blockIdx.x % tiles_x) * kTW;
  const int bq = blockIdx.y, n0 = blockIdx.z * 32;

  for (int kk = tid; kk < KCM; kk += kT) {
    const int cl = kk / taps, t = kk % taps;
    ktab[kk] = cl * PLANE + (t / kw) * HX + t % kw;
  }
  for (int i = tid; i < a.cic * PLANE; i += kT) {
    const int cl = i / PLANE, r = i % PLANE;
    htab[i] = cl << 16 | (r / HX) << 8 | r % HX;
  }
  // lane = pixel p of the wave's two rows; registers = channels (r&3) + 8(r>>2) + 4h of the slice
  const int py = 2 * w + (p >> 4), px = p & 15;
  const int pix_off = py * HX + px;

  f32x16 acc[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;

  const float* inb = a.in + (size_t)bq * a.cin * HW;
  const size_t gstride = (size_t)a.cin_p * taps * a.cout_p;   // one weight group
  for (int c0 = 0; c0 < a.cin_p; c0 += a.cic) {
    const int nch = a.cin_p - c0 < a.cic ? a.cin_p - c0 : a.cic;
    const int KC = nch * taps;   // even: nch is
    __syncthreads();             // the tables are written; the previous chunk is read
    for (int i = tid; i < nch * PLANE; i += kT) {
      const int e = htab[i];
      const int ci = c0 + (e >> 16), y = ty0 + ((e >> 8) & 255) - ph, x = tx0 + (e & 255) - pw;
      float v = 0.f;
      if (ci < a.cin && y >= 0 && y < H && x >= 0 && x < W) v = inb[(size_t)ci * HW + (unsigned)(y * W + x)];
      halo[i] = v;
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const float* src = a.wts + g * gstride + (size_t)c0 * taps * a.cout_p + n0;
      for (int i = tid; i < KC * 32; i += kT) wl[g * KCM * 32 + i] = src[(size_t)(i >> 5) * a.cout_p + (i & 31)];
    }
    __syncthreads();
    for (int j = 0; j < KC; j += 2) {
      const int kk = j + h;
      const float x = halo[ktab[kk] + pix_off];
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        float xg = x;
        // forward, three groups: W on x, W+ on x+, W- on x- (the 3x3 kernels' expression)
        if constexpr (!BWD && NG == 3) xg = (g == 0) ? x : (g == 1 ? fmaxf(x, 0.f) : fminf(x, 0.f));
        acc[g] = mfma32(wl[(g * KCM + kk) * 32 + p], xg, acc[g]);
      }
    }
  }

  const int Y = ty0 + py, X = tx0 + px;
  const bool pix_ok = Y < H && X < W;
  const unsigned pix = pix_ok ? (unsigned)(Y * W + X) : 0u;
  float* const ob = a.out + (size_t)bq * a.cout * HW;
  if constexpr (!BWD) {
    float* const db = a.out_den ? a.out_den + (size_t)bq * a.cout * HW : nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = n0 + (r & 3) + 8 * (r >> 2) + 4 * h;   // < cout_p: bias is [3][cout_p]
      const bool ok = pix_ok && co < a.cout;
      const float b0 = a.bias[co], b1 = a.bias[a.cout_p + co], b2 = a.bias[2 * a.cout_p + co];
      const float z = acc[0][r] + b0;
      float yv = z > 0.f ? z : 0.f;
      if (z != z) yv = z;   // relu(NaN) = NaN (torch semantics)
      const size_t o = (size_t)(ok ? co : 0) * HW + pix;
      if (ok) ob[o] = yv;
      if (db && ok) {
        float d;
        if (a.den_map) d = a.den_map[o];
        else if constexpr (NG == 1) d = acc[0][r] + b1;
        else if constexpr (NG == 2) d = (acc[1][r] + b1) + b2;
        else d = (acc[1][r] + b1) + (acc[2][r] + b2);
        db[o] = d;
      }
    }
  } else {
    const int bs = bq / a.clones;
    const bool need_x = a.xmode != XM_NONE || a.post != POST_NONE;
    const bool mul_x = a.xmode != XM_NONE, split_x = a.xmode == XM_SPLIT;
    const bool post_div = a.post == POST_DIV, post_any = a.post != POST_NONE;
    const float* const xb = need_x ? a.x + (size_t)bs * a.cout * HW : ob;
    const float* const dnb = post_div ? a.den + (size_t)bs * a.cout * HW : xb;
    // x and den from clamped, always valid addresses, all issued before the arithmetic; the modes are
    // uniform selects (lrp_conv_kernel.h EPI_BWD)
    float xv[16], dv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = n0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      const size_t o = (size_t)(pix_ok && co < a.cout ? co : 0) * HW + pix;
      xv[r] = need_x ? xb[o] : 0.f;
      dv[r] = post_div ? dnb[o] : 1.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = n0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      const bool ok = pix_ok && co < a.cout;
      const float res = rule_post<NG>(acc[0][r], acc[NG - 1][r], xv[r], dv[r], mul_x, split_x, post_div, post_any, a.eps);
      if (ok) ob[(size_t)co * HW + pix] = res;
    }
  }
}

// The backward into ONE output channel (the first layer's: cout = 1), where an MFMA tile would spend 31 of
// its 32 channel rows on padding: a VALU chain per pixel, the same fmaf chain in the same order.  A workgroup
// owns a 16 x 16 pixel tile, one thread per pixel; per chunk of `cic` g channels the halo and the chunk's
// weights (column 0 of the rows) are staged in LDS, the weights read back as broadcasts.
constexpr int kSH = 16, kSW = 16;
template <int NG>
__global__ __launch_bounds__(kT) void convk_bwd1_kernel(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int kh = a.kh, kw = a.kw, ph = kh >> 1, pw = kw >> 1;
  const int HY = kSH + kh - 1, HX = kSW + kw - 1, PLANE = HY * HX, taps = kh * kw;
  float* halo = smem;                      // [cic][PLANE]
  float* wl = smem + a.cic * PLANE;        // [NG][cic * taps]
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int H = a.H, W = a.W, HW = H * W;
  const int tiles_x = (W + kSW - 1) / kSW;
  const int ty0 = (blockIdx.x / tiles_x) * kSH, tx0 = (blockIdx.x % tiles_x) * kSW;
  const int bq = blockIdx.y;
  const float* inb = a.in + (size_t)bq * a.cin * HW;
  const size_t gstride = (size_t)a.cin_p * taps * a.cout_p;
  float acc0 = 0.f, acc1 = 0.f;
  for (int c0 = 0; c0 < a.cin; c0 += a.cic) {
    const int nch = a.cin - c0 < a.cic ? a.cin - c0 : a.cic;
    __syncthreads();
    {   // halo rows (channel, hy) in order, 8 per pass, one lane per column (HX <= 22 of the 32)
      const int col = tid & 31, x = tx0 + col - pw;
      const bool xok = x >= 0 && x < W;
      int cl = 0, hy = tid >> 5;
      while (cl < nch) {
        const int y = ty0 + hy - ph;
        if (col < HX) {
          float v = 0.f;
          if (xok && y >= 0 && y < H) v = inb[(size_t)(c0 + cl) * HW + (unsigned)(y * W + x)];
          halo[cl * PLANE + hy * HX + col] = v;
        }
        hy += 8;
        if (hy >= HY) { hy -= HY; ++cl; }   // HY >= 16: at most one channel step per pass
      }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g)
      for (int kk = tid; kk < nch * taps; kk += kT)
        wl[g * a.cic * taps + kk] = a.wts[g * gstride + (size_t)(c0 * taps + kk) * a.cout_p];
    __syncthreads();
    for (int cl = 0; cl < nch; ++cl)
      for (int ky = 0; ky < kh; ++ky) {
        const float* hrow = halo + cl * PLANE + (ty + ky) * HX + tx;
        const float* wrow = wl + (cl * kh + ky) * kw;
        for (int kx = 0; kx < kw; ++kx) {
          const float v = hrow[kx];
          acc0 = fmaf(v, wrow[kx], acc0);
          if constexpr (NG == 2) acc1 = fmaf(v, wrow[a.cic * taps + kx], acc1);
        }
      }
  }
  const int Y = ty0 + ty, X = tx0 + tx;
  if (Y >= H || X >= W) return;
  const size_t pix = (size_t)Y * W + X;
  const int bs = bq / a.clones;
  const bool need_x = a.xmode != XM_NONE || a.post != POST_NONE, post_div = a.post == POST_DIV;
  const float xx = need_x ? a.x[(size_t)bs * HW + pix] : 0.f;
  const float dd = post_div ? a.den[(size_t)bs * HW + pix] : 1.f;
  a.out[(size_t)bq * HW + pix] = rule_post<NG>(acc0, acc1, xx, dd, a.xmode != XM_NONE, a.xmode == XM_SPLIT, post_div,
                                               a.post != POST_NONE, a.eps);
}

int pad32(int c) { return (c + 31) / 32 * 32; }
int pad2(int c) { return (c + 1) / 2 * 2; }
bool odd_k(int k) { return k == 1 || k == 3 || k == 5 || k == 7; }

// floats of LDS per chunk channel; the chunk is the largest even count that keeps a workgroup within
// kLdsBudget (four workgroups per CU), at least 2
constexpr size_t kLdsBudget = 40 * 1024;
size_t lds_per_channel(int kh, int kw, int ng) {
  const size_t plane = (size_t)(kTH + kh - 1) * (kTW + kw - 1);
  return 2 * plane + (size_t)kh * kw * (32 * ng + 1);
}
int chunk_channels(int kh, int kw, int ng, int cin_p) {
  int cic = (int)(kLdsBudget / 4 / lds_per_channel(kh, kw, ng)) & ~1;
  if (cic > 32) cic = 32;
  if (cic > cin_p) cic = cin_p;
  return cic < 2 ? 2 : cic;
}

template <int NG, bool BWD>
int launch_ng(const KArgs& a, int batch, hipStream_t s) {
  const size_t lds = (size_t)a.cic * lds_per_channel(a.kh, a.kw, NG) * 4;
  const int tiles = ((a.H + kTH - 1) / kTH) * ((a.W + kTW - 1) / kTW);
  hipLaunchKernelGGL((convk_kernel<NG, BWD>), dim3(tiles, batch, a.cout_p / 32), dim3(kT), lds, s, a);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

template <int NG>
int launch_bwd1(KArgs a, int batch, hipStream_t s) {
  a.cic = a.cin < 8 ? a.cin : 8;
  const size_t lds = (size_t)a.cic * ((kSH + a.kh - 1) * (kSW + a.kw - 1) + NG * a.kh * a.kw) * 4;
  const int tiles = ((a.H + kSH - 1) / kSH) * ((a.W + kSW - 1) / kSW);
  hipLaunchKernelGGL((convk_bwd1_kernel<NG>), dim3(tiles, batch), dim3(kT), lds, s, a);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

// the checks the two directions share; n: entry point, for messages
int check_common(const char* n, int batch, int cin, int cout, int H, int W, int kh, int kw) {
  DRSA_REQUIRE(odd_k(kh) && odd_k(kw), "%s: kh and kw must be odd, 1..7 (got %dx%d)", n, kh, kw);
  DRSA_REQUIRE(batch > 0 && batch <= 65535 && cin > 0 && cout > 0 && H > 0 && W > 0, "%s: bad shape", n);
  DRSA_REQUIRE(drsa_amd_convk_supported(kh, kw, cin, cout), "%s: unsupported channel counts %d -> %d", n, cin, cout);
  DRSA_REQUIRE(H % 2 == 0 && W % 4 == 0, "%s: H must be even and W %% 4 == 0 (got %dx%d)", n, H, W);
  DRSA_REQUIRE((int64_t)(cin > cout ? cin : cout) * H * W < ((int64_t)1 << 31),
               "%s: one sample's channels x H x W must stay below 2^31", n);
  return DRSA_OK;
}

}  // namespace

extern "C" {

int drsa_amd_convk_supported(int kh, int kw, int cin, int cout) {
  // the grid's z axis carries the 32-channel output slices
  return odd_k(kh) && odd_k(kw) && cin >= 1 && cout >= 1 && cin <= (1 << 20) && pad32(cout) / 32 <= 65535;
}

size_t drsa_amd_convk_weight_floats(int kh, int kw, int cin, int cout, int ng) {
  if (!drsa_amd_convk_supported(kh, kw, cin, cout) || ng < 1) return 0;
  return (size_t)ng * pad2(cin) * kh * kw * pad32(cout);
}

int drsa_amd_convk_fwd(const float* in, const float* wts, const float* bias, const float* den_map, float* out,
                       float* out_den, int B, int cin, int cout, int H, int W, int kh, int kw, int ng, void* stream) {
  const char* n = "convk_fwd";
  DRSA_REQUIRE(in && wts && bias && out, "%s: null pointer", n);
  DRSA_REQUIRE(ng >= 1 && ng <= 3, "%s: ng must be 1..3", n);
  if (int rc = check_common(n, B, cin, cout, H, W, kh, kw)) return rc;
  KArgs a{};
  a.in = in; a.wts = wts; a.bias = bias; a.den_map = den_map; a.out = out; a.out_den = out_den;
  a.H = H; a.W = W; a.cin = cin; a.cout = cout; a.cin_p = pad2(cin); a.cout_p = pad32(cout); a.kh = kh; a.kw = kw;
  a.cic = chunk_channels(kh, kw, ng, a.cin_p); a.clones = 1;
  hipStream_t s = (hipStream_t)stream;
  return ng == 1 ? launch_ng<1, false>(a, B, s) : ng == 2 ? launch_ng<2, false>(a, B, s) : launch_ng<3, false>(a, B, s);
}

int drsa_amd_convk_bwd(const float* g, const float* wts, const float* x, const float* den, float* out, int Bq,
                       int clones, int cin, int cout, int H, int W, int kh, int kw, int ng, int xmode, int post,
                       float eps, void* stream) {
  const char* n = "convk_bwd";
  DRSA_REQUIRE(g && wts && out, "%s: null pointer", n);
  DRSA_REQUIRE(ng >= 1 && ng <= 2, "%s: ng must be 1..2", n);
  DRSA_REQUIRE(clones > 0 && Bq > 0 && Bq % clones == 0, "%s: bad batch/clones", n);
  if (int rc = check_common(n, Bq, cin, cout, H, W, kh, kw)) return rc;
  DRSA_REQUIRE(xmode == XM_NONE || xmode == XM_MUL || xmode == XM_SPLIT, "%s: bad xmode", n);
  DRSA_REQUIRE(post == POST_NONE || post == POST_DIV || post == POST_MASK, "%s: post must be 0, 1 or 2", n);
  DRSA_REQUIRE(xmode == XM_NONE || x, "%s: xmode needs x", n);
  DRSA_REQUIRE(post == POST_NONE || (x && (den || post == POST_MASK)), "%s: POST_DIV needs x and den", n);
  KArgs a{};
  a.in = g; a.wts = wts; a.x = x; a.den = den; a.out = out;
  a.H = H; a.W = W; a.cin = cin; a.cout = cout; a.cin_p = pad2(cin); a.cout_p = pad32(cout); a.kh = kh; a.kw = kw;
  a.cic = chunk_channels(kh, kw, ng, a.cin_p); a.clones = clones; a.xmode = xmode; a.post = post; a.eps = eps;
  hipStream_t s = (hipStream_t)stream;
  if (cout == 1) return ng == 1 ? launch_bwd1<1>(a, Bq, s) : launch_bwd1<2>(a, Bq, s);   // the VALU chain
  return ng == 1 ? launch_ng<1, true>(a, Bq, s) : launch_ng<2, true>(a, Bq, s);
}

}  // extern "C"
