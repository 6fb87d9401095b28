// Kernel arguments of the K x K conv kernels (conv_generic.hip; not part of the public ABI).
#pragma once
#include <stdint.h>

namespace drsa_convk {

constexpr int kTH = 8, kTW = 16;   // pixel tile of a workgroup

struct KArgs {
  const float* in;        // forward: x [B][cin][H][W]; backward: g [Bq][cin][H][W]
  const float* wts;       // [ng][cin_p * kh * kw][cout_p], row k = (ci * kh + ky) * kw + kx
  const float* bias;      // forward: [3][cout_p]
  const float* den_map;   // forward, WSquare / Flat: [cout][H][W]
  const float* x;         // backward: the layer's input [Bq / clones][cout][H][W]
  const float* den;       // backward POST_DIV: the denominator of the layer below, like x
  float* out;
  float* out_den;
  int H, W;
  int cin, cout;          // channels of `in` and of `out`
  int cin_p, cout_p;      // cin padded to 2 (the MFMA's k step), cout to 32
  int kh, kw;
  int cic;                // input channels per chunk (even)
  int clones, xmode, post;
  float eps;
};

}  // namespace drsa_convk
