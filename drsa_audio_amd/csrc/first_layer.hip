// LRP first layer (WSquare / Flat rules, reference constants.py:29,42; zennit 0.5.1), one input
// channel:
//   * backward  R[y][x] = sum_co sum_{dy,dx} G[co][y+dy][x+dx] * W2[co][1-dy][1-dx]
//               the one-chain kernels of first_layer_bwd.h, G dense or pool-sparse (gp, argmax)
//   * the rules' denominator map (input independent)
#include "first_layer_bwd.h"

namespace {

// den[co][y][x] = sum_ci sum_{in-bounds taps} w2[co][ci][ky][kx] * 1 + b2[co]
__global__ void first_layer_den_kernel(const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ den,
                                       int C, int CI, int H, int W) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)C * H * W) return;
  const int co = (int)(i / ((size_t)H * W));
  const int y = (int)((i / W) % H), x = (int)(i % W);
  float acc = 0.f;
  for (int ci = 0; ci < CI; ++ci)
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) acc = fmaf(1.f, w2[((co * CI + ci) * 3 + ky) * 3 + kx], acc);
      }
  den[i] = acc + (b2 ? b2[co] : 0.f);
}

}  // namespace

extern "C" {

int drsa_amd_first_layer_bwd(const float* g, const uint8_t* amax, const float* w2f, float* out, int Bq, int clones,
                             int C, int H, int W, void* stream) {
  return first_layer_bwd_launch<1, StoreChain>("first_layer_bwd", g, amax, w2f, out, Bq, clones, C, H, W, stream);
}

int drsa_amd_first_layer_den(const float* w2, const float* b2, float* den, int C, int CI, int H, int W, void* stream) {
  const size_t n = (size_t)C * H * W;
  hipLaunchKernelGGL(first_layer_den_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w2,
                     b2, den, C, CI, H, W);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

}  // extern "C"
