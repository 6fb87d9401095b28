/* Pinned-order fp32 primitives of the K x K conv entry points (drsa_amd_convk_fwd / _bwd), for
 * tests/convk_ref.py: every output is one fp32 fma chain from +0 in ascending k, a pixel off the
 * image contributing operand 0 (include/drsa_amd.h).  Built by convk_ref.py with the flags of
 * oracle/Makefile (-ffp-contract=off: the only fused operations are the fmaf calls below). */
#include <math.h>
#include <stddef.h>

/* out[b][co][y][x] = chain over k = (ci * kh + ky) * kw + kx of
 * fmaf(x[b][ci][y + ky - ph][x + kx - pw], w[co][ci][ky][kx], acc); then + bias[co] (one rounding). */
void convk_exact(const float* x, const float* w, const float* b, float* out, int B, int Cin, int Cout, int H,
                 int W, int kh, int kw) {
  const int ph = (kh - 1) / 2, pw = (kw - 1) / 2;
#pragma omp parallel for collapse(2)
  for (int n = 0; n < B; ++n)
    for (int co = 0; co < Cout; ++co)
      for (int y = 0; y < H; ++y)
        for (int xx = 0; xx < W; ++xx) {
          float acc = 0.f;
          for (int ci = 0; ci < Cin; ++ci)
            for (int ky = 0; ky < kh; ++ky)
              for (int kx = 0; kx < kw; ++kx) {
                const int yy = y + ky - ph, xc = xx + kx - pw;
                const float v = (yy >= 0 && yy < H && xc >= 0 && xc < W)
                                    ? x[(((size_t)n * Cin + ci) * H + yy) * W + xc] : 0.f;
                acc = fmaf(v, w[(((size_t)co * Cin + ci) * kh + ky) * kw + kx], acc);
              }
          out[(((size_t)n * Cout + co) * H + y) * W + xx] = b ? acc + b[co] : acc;
        }
}

/* The transposed conv as a 'same' conv over g with flipped taps: out[b][ci][y][x] = chain over
 * k = (co * kh + ky) * kw + kx of fmaf(g[b][co][y + ky - ph][x + kx - pw], w[co][ci][kh-1-ky][kw-1-kx], acc). */
void convk_transpose_exact(const float* g, const float* w, float* out, int B, int Cout, int Cin, int H, int W,
                           int kh, int kw) {
  const int ph = (kh - 1) / 2, pw = (kw - 1) / 2;
#pragma omp parallel for collapse(2)
  for (int n = 0; n < B; ++n)
    for (int ci = 0; ci < Cin; ++ci)
      for (int y = 0; y < H; ++y)
        for (int xx = 0; xx < W; ++xx) {
          float acc = 0.f;
          for (int co = 0; co < Cout; ++co)
            for (int ky = 0; ky < kh; ++ky)
              for (int kx = 0; kx < kw; ++kx) {
                const int yy = y + ky - ph, xc = xx + kx - pw;
                const float v = (yy >= 0 && yy < H && xc >= 0 && xc < W)
                                    ? g[(((size_t)n * Cout + co) * H + yy) * W + xc] : 0.f;
                acc = fmaf(v, w[(((size_t)co * Cin + ci) * kh + (kh - 1 - ky)) * kw + (kw - 1 - kx)], acc);
              }
          out[(((size_t)n * Cin + ci) * H + y) * W + xx] = acc;
        }
}
