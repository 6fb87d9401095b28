// Host dispatch of the 3x3 conv kernels (kernel: lrp_conv_kernel.h; instantiations: conv_*.hip
// through lrp_conv_inst.h).  Only the tables and the configuration are seen here, not the kernel.
#include "common.h"
#include "lrp_conv.h"
#include "lrp_conv_table.h"

#include <stdlib.h>

// ---------------------------------------------------------------------------
// dispatch table
// ---------------------------------------------------------------------------
// The tables find() searches, in its search order: one per conv_*.hip file (CONV_TABLE).  A table
// missing here is never searched.  conv_small.hip's kTableSmall is read by small_tile() only.
#define DRSA_CONV_TABLES(X) \
  X(FwdA) X(FwdB) X(FwdC) X(FwdD) X(FwdE) X(BwdA) X(BwdB) X(BwdC) X(FwdBfA) X(FwdBfB) X(FwdBfC) X(FwdP4) X(BwdBfA) X(BwdBfB)

namespace drsa_conv {
#define DRSA_CONV_DECLARE(T) extern const Table kTable##T;
DRSA_CONV_TABLES(DRSA_CONV_DECLARE)
extern const Table kTableSmall;
}

namespace {
using drsa_conv::Entry;
using namespace drsa_conv;

#define DRSA_CONV_ADDRESS(T) &drsa_conv::kTable##T,
const drsa_conv::Table* kTables[] = {DRSA_CONV_TABLES(DRSA_CONV_ADDRESS)};

int pad32(int c) { return (c + 31) / 32 * 32; }

// The tables hold, per kernel set, the one tile of each width class (the tile rule:
// lrp_conv_config.h wide_tile_w()), so the lookup only picks the class of W.
const Entry* find(int cin_p, int cout_p, int W, int ng, int amode, int epi, int et = 0, int pw = 2) {
  const int wide = W >= kWideW;
  for (const drsa_conv::Table* t : kTables)
    for (int i = 0; i < t->n; ++i) {
      const Entry& e = t->entries[i];
      if (e.cin_p == cin_p && e.cout_p == cout_p && e.ng == ng && e.amode == amode && e.epi == epi && e.et == et &&
          e.pw == pw && e.wide == wide)
        return &e;
    }
  return nullptr;
}

// 4 x 8 tiles (conv_small.hip) replace an 8 x 8 entry whose grid would have fewer workgroups than
// this (two per CU): twice the workgroups for the small maps at small batches.  VGGish (B = 32):
// conv_fwd:features.24 / .28 0.108 / 0.103 -> 0.064 / 0.061 ms, conv_bwd:features.31 0.060 ->
// 0.044, fp32 standard LRP 8.2k -> 8.6k samples/s; at GTZAN's 512 workgroups (features.12, B = 512)
// 8 x 8 stays faster (4 x 8: 0.093 -> 0.119 ms forward, 0.051 -> 0.080 backward)
#ifndef DRSA_CONV_SMALL_WG
#define DRSA_CONV_SMALL_WG 512
#endif
const Entry* small_tile(const Entry* e, int H, int W, int batch) {
  if (e->th != 8 || e->tw != 8) return e;
  if ((int64_t)((H + 7) / 8) * ((W + 7) / 8) * batch >= DRSA_CONV_SMALL_WG) return e;
  for (int i = 0; i < drsa_conv::kTableSmall.n; ++i) {
    const Entry& c = drsa_conv::kTableSmall.entries[i];
    if (c.cin_p == e->cin_p && c.cout_p == e->cout_p && c.ng == e->ng && c.amode == e->amode && c.epi == e->epi &&
        c.et == e->et && c.pw == e->pw)
      return &c;
  }
  return e;
}

int launch(const Entry* e0, const ConvArgs& args, int batch, hipStream_t s) {   // batch = grid.y
  // the kernels address one sample's planes with 32-bit offsets from a per-sample base
  DRSA_REQUIRE((int64_t)(args.cin > args.cout ? args.cin : args.cout) * args.H * args.W < ((int64_t)1 << 31),
               "conv: one sample's channels x H x W must stay below 2^31");
  const Entry* e = small_tile(e0, args.H, args.W, batch);
  DRSA_SMEM(e->fn, e->lds);   // per device, thread-safe
  const int tiles = ((args.H + e->th - 1) / e->th) * ((args.W + e->tw - 1) / e->tw);
  hipLaunchKernelGGL(e->fn, dim3(tiles, batch), dim3(kThreads), e->lds, s, args);
  DRSA_LAUNCH_CHECK();
  return DRSA_OK;
}

int cin_pad(int cin) { return cin == 1 ? 1 : pad32(cin); }

// ---------------------------------------------------------------------------
// lookup: what identifies a kernel, per direction.  The *_has_kernel* queries and the launches all go
// through these two, so a query answers with the lookup the launch will do.
// ---------------------------------------------------------------------------
const Entry* find_fwd(int cin, int cout, int W, int ng, int pool, int bf16) {
  return find(bf16 ? pad32(cin) : cin_pad(cin), pad32(cout), W, ng, A_DENSE, pool ? EPI_FWD_POOL : EPI_FWD_RELU,
              bf16 ? 1 : 0, pool == 2 ? 4 : 2);
}

const Entry* find_bwd(int cin, int cout, int W, int ng, int sparse, int bf16, int pool_w) {
  return find(pad32(cin), pad32(cout), W, ng, sparse ? A_POOLSPARSE : A_DENSE, EPI_BWD, bf16 ? 1 : 0, pool_w);
}

// pool: the forward's pool mode ("pool") or the backward's pool window width ("pool_w")
int no_kernel(const char* entry, int cin, int cout, int W, int ng, int sparse, int bf16, const char* pool_key, int pool) {
  drsa::set_error("%s: no kernel for cin=%d cout=%d W=%d ng=%d sparse=%d bf16=%d %s=%d", entry, cin, cout, W, ng, sparse,
                  bf16 ? 1 : 0, pool_key, pool);
  return DRSA_EUNSUPPORTED;
}

// ---------------------------------------------------------------------------
// forward: one checked path for conv_fwd, conv_fwd_bf16 and conv_fwd_den_ring
// ---------------------------------------------------------------------------
struct FwdCall {
  const char* name;   // entry point, for messages
  const float* in;
  const void* wts;
  int bf16;           // wts are bf16 (16-byte aligned, cin > 1)
  const float *bias, *den_map;
  float* out;
  uint8_t* out_amax;
  float* out_den;
  int den_ring_only;
  int B, cin, cout, H, W, ng, pool;
};

int conv_fwd_run(const FwdCall& c, void* stream) {
  const char* n = c.name;
  DRSA_REQUIRE(c.B > 0 && c.H > 0 && c.W > 0, "%s: bad shape", n);
  DRSA_REQUIRE(!c.bf16 || c.cin > 1, "%s: cin = 1 runs on drsa_amd_conv_fwd (fp32 VALU kernel)", n);
  DRSA_REQUIRE(c.ng >= 1 && c.ng <= 3, "%s: ng must be 1..3", n);
  DRSA_REQUIRE(c.H % 2 == 0 && c.W % 2 == 0, "%s: H and W must be even (got %dx%d)", n, c.H, c.W);
  DRSA_REQUIRE(c.pool >= 0 && c.pool <= 2, "%s: pool must be 0 (none), 1 (2x2) or 2 (2x4)", n);
  DRSA_REQUIRE(!c.pool || c.out_amax, "%s: pool needs out_amax", n);
  DRSA_REQUIRE(c.pool || c.W % 4 == 0, "%s: an unpooled output needs W %% 4 == 0 (float4 epilogue; got W=%d)", n, c.W);
  DRSA_REQUIRE(c.pool != 2 || c.W % 4 == 0, "%s: a 2x4 pool needs W %% 4 == 0 (got W=%d)", n, c.W);
  DRSA_REQUIRE(!c.bf16 || ((uintptr_t)c.wts & 15) == 0, "%s: weights must be 16-byte aligned", n);
  ConvArgs a{};
  a.in = c.in; a.wts = reinterpret_cast<const float*>(c.wts); a.bias = c.bias; a.den_map = c.den_map; a.out = c.out;
  a.out_amax = c.out_amax; a.out_den = c.out_den; a.H = c.H; a.W = c.W; a.cin = c.cin; a.cout = c.cout; a.clones = 1;
  a.den_ring_only = c.den_ring_only;
  if (c.cin == 1 && c.pool == 1 && c.W % 8 == 0)   // the Cin = 1 VALU kernel (conv_first.hip)
    return drsa_first_conv_pool(a, pad32(c.cout), c.ng, c.B, (hipStream_t)stream);
  const Entry* e = find_fwd(c.cin, c.cout, c.W, c.ng, c.pool, c.bf16);
  if (!e) return no_kernel(n, c.cin, c.cout, c.W, c.ng, 0, c.bf16, "pool", c.pool);
  return launch(e, a, c.B, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// backward: one checked path for the five conv_bwd* entry points
// ---------------------------------------------------------------------------
struct BwdCall {
  const char* name;   // entry point, for messages
  const float* g;
  const uint8_t* g_amax;
  int pool_w;         // pool window width of a pool-sparse g (the kernel's PW; 2 with a dense g)
  const void* wts;
  int bf16;           // wts are bf16 (ng 1, cin >= 16, 16-byte aligned)
  const float *x, *den, *den_const4;
  int den_shared;
  float* out;
  int Bq, clones, cin, cout, H, W, ng, xmode, post;
  float eps;
};

int conv_bwd_run(const BwdCall& c, void* stream) {
  const char* n = c.name;
  DRSA_REQUIRE(c.Bq > 0 && c.clones > 0 && c.Bq % c.clones == 0, "%s: bad batch/clones", n);
  if (c.bf16) {
    DRSA_REQUIRE(c.ng == 1, "%s: bf16 weights need ng == 1 (the Gamma x-/W- term is for the fp32 first layer)", n);
    DRSA_REQUIRE(c.cin >= 16, "%s: bf16 weights need cin >= 16 (16-channel bf16 chunks)", n);
    DRSA_REQUIRE(((uintptr_t)c.wts & 15) == 0, "%s: bf16 weights must be 16-byte aligned", n);
  } else {
    DRSA_REQUIRE(c.ng >= 1 && c.ng <= 2, "%s: ng must be 1..2", n);
  }
  // the compact ring (den_const4) has its own size rule: drsa_amd_conv_bwd_den_ring, H a pooled height
  DRSA_REQUIRE(c.den_const4 || (c.H % 2 == 0 && c.W % 4 == 0),
               "%s: H must be even and W %% 4 == 0 (got %dx%d)", n, c.H, c.W);
  DRSA_REQUIRE(c.xmode == XM_NONE || c.x, "%s: xmode needs x", n);
  DRSA_REQUIRE(c.post == POST_NONE || (c.x && (c.den || c.post == POST_MASK)), "%s: POST_DIV needs x and den", n);
  const int sparse = c.g_amax != nullptr;
  const Entry* e = find_bwd(c.cin, c.cout, c.W, c.ng, sparse, c.bf16, c.pool_w);
  if (!e) return no_kernel(n, c.cin, c.cout, c.W, c.ng, sparse, c.bf16, "pool_w", c.pool_w);
  ConvArgs a{};
  a.in = c.g; a.in_amax = c.g_amax; a.wts = reinterpret_cast<const float*>(c.wts); a.x = c.x; a.den = c.den;
  a.den_const4 = c.den_const4; a.den_shared = c.den_shared; a.out = c.out; a.H = c.H; a.W = c.W; a.cin = c.cin;
  a.cout = c.cout; a.clones = c.clones; a.xmode = c.xmode; a.post = c.post; a.eps = c.eps;
  return launch(e, a, c.Bq, (hipStream_t)stream);
}

}  // namespace

extern "C" {

size_t drsa_amd_conv_weight_floats(int cin, int cout, int ng) {
  return (size_t)ng * 9 * cin_pad(cin) * pad32(cout);
}

size_t drsa_amd_conv_weight_bf16_elems(int cin, int cout, int ng) {
  return (size_t)ng * 9 * pad32(cin) * pad32(cout);
}

// ------------------------------------------------------------------ queries
int drsa_amd_conv_fwd_has_kernel(int cin, int cout, int W, int ng, int pool, int bf16) {
  if (cin == 1 && !bf16 && pool == 1) return 1;   // conv_first (W % 8 == 0) or the generic Cin = 1 kernels
  if (pool < 0 || pool > 2 || ng < 1 || ng > 3 || (bf16 && cin == 1)) return 0;
  return find_fwd(cin, cout, W, ng, pool, bf16) != nullptr;
}

int drsa_amd_conv_bwd_has_kernel_bf16(int cin, int cout, int W, int ng, int sparse) {
  if (cin < 16 || ng != 1) return 0;
  return find_bwd(cin, cout, W, ng, sparse, 1, 2) != nullptr;
}

int drsa_amd_conv_bwd_has_kernel_pw(int cin, int cout, int W, int ng, int pool_w) {
  if (cin < 2 || (pool_w != 2 && pool_w != 4) || (pool_w == 4 && (W / 4) % 4 != 0)) return 0;
  return find_bwd(cin, cout, W, ng, 1, 0, pool_w) != nullptr;
}

int drsa_amd_conv_bwd_has_kernel_bf16_pw(int cin, int cout, int W, int pool_w) {
  if (cin < 16 || (pool_w != 2 && pool_w != 4)) return 0;
  return find_bwd(cin, cout, W, 1, 1, 1, pool_w) != nullptr;
}

// ------------------------------------------------------------------ forward
int drsa_amd_conv_fwd(const float* in, const float* wts, const float* bias, const float* den_map, float* out,
                      uint8_t* out_amax, float* out_den, int B, int cin, int cout, int H, int W, int ng,
                      int pool, void* stream) {
  return conv_fwd_run({"conv_fwd", in, wts, 0, bias, den_map, out, out_amax, out_den, 0, B, cin, cout, H, W, ng, pool},
                      stream);
}

int drsa_amd_conv_fwd_bf16(const float* in, const uint16_t* wts, const float* bias, const float* den_map, float* out,
                           uint8_t* out_amax, float* out_den, int B, int cin, int cout, int H, int W, int ng,
                           int pool, void* stream) {
  return conv_fwd_run({"conv_fwd_bf16", in, wts, 1, bias, den_map, out, out_amax, out_den, 0, B, cin, cout, H, W, ng, pool},
                      stream);
}

int drsa_amd_conv_fwd_den_ring(const float* in, const float* wts, const float* bias, const float* den_map, float* out,
                               uint8_t* out_amax, float* den_ring, int B, int cout, int H, int W, int ng,
                               void* stream) {
  DRSA_REQUIRE(in && wts && den_map && out && out_amax && den_ring, "conv_fwd_den_ring: null pointer");
  // W % 16 == 0 sends the call to the Cin = 1 kernel (W % 8 == 0), the only one that writes the ring
  DRSA_REQUIRE(B > 0 && H >= 4 && W > 0 && H % 2 == 0 && W % 16 == 0,
               "conv_fwd_den_ring: needs H >= 4 even and W %% 16 == 0 (got %dx%d)", H, W);
  return conv_fwd_run({"conv_fwd_den_ring", in, wts, 0, bias, den_map, out, out_amax, den_ring, 1, B, 1, cout, H, W, ng, 1},
                      stream);
}

// ------------------------------------------------------------------ backward
int drsa_amd_conv_bwd(const float* g, const uint8_t* g_amax, const float* wts, const float* x, const float* den,
                      float* out, int Bq, int clones, int cin, int cout, int H, int W, int ng, int xmode,
                      int post, float eps, void* stream) {
  return conv_bwd_run({"conv_bwd", g, g_amax, 2, wts, 0, x, den, nullptr, 0, out, Bq, clones, cin, cout, H, W, ng, xmode,
                       post, eps}, stream);
}

int drsa_amd_conv_bwd_bf16(const float* g, const uint8_t* g_amax, const uint16_t* wts, const float* x, const float* den,
                           float* out, int Bq, int clones, int cin, int cout, int H, int W, int ng, int xmode,
                           int post, float eps, void* stream) {
  return conv_bwd_run({"conv_bwd_bf16", g, g_amax, 2, wts, 1, x, den, nullptr, 0, out, Bq, clones, cin, cout, H, W, ng,
                       xmode, post, eps}, stream);
}

int drsa_amd_conv_bwd_bf16_pw(const float* g, const uint8_t* g_amax, int pool_w, const uint16_t* wts, const float* x,
                              const float* den, float* out, int Bq, int clones, int cin, int cout, int H, int W,
                              int xmode, int post, float eps, void* stream) {
  DRSA_REQUIRE(g_amax && (pool_w == 2 || pool_w == 4), "conv_bwd_bf16_pw: needs g_amax and pool_w 2 or 4");
  return conv_bwd_run({"conv_bwd_bf16_pw", g, g_amax, pool_w, wts, 1, x, den, nullptr, 0, out, Bq, clones, cin, cout, H,
                       W, 1, xmode, post, eps}, stream);
}

int drsa_amd_conv_bwd_den_map(const float* g, const uint8_t* g_amax, int pool_w, const void* wts, int wts_bf16,
                              const float* x, const float* den_map, float* out, int Bq, int clones, int cin, int cout,
                              int H, int W, int ng, int xmode, float eps, void* stream) {
  DRSA_REQUIRE(x && den_map, "conv_bwd_den_map: needs x and den_map");
  DRSA_REQUIRE(!g_amax || pool_w == 2 || pool_w == 4, "conv_bwd_den_map: pool_w must be 2 or 4");
  DRSA_REQUIRE(xmode == XM_NONE || xmode == XM_MUL || xmode == XM_SPLIT, "conv_bwd_den_map: bad xmode");
  const bool pool24 = g_amax && pool_w == 4;
  DRSA_REQUIRE(wts_bf16 || !pool24 || ng == 1, "conv_bwd_den_map: fp32 weights need ng 1 under a 2x4 pool (got ng=%d)", ng);
  DRSA_REQUIRE(!pool24 || (W / 4) % 4 == 0, "conv_bwd_den_map: a 2x4 pool-sparse g needs W / 4 %% 4 == 0 (got W=%d)", W);
  return conv_bwd_run({"conv_bwd_den_map", g, g_amax, g_amax ? pool_w : 2, wts, wts_bf16 != 0, x, den_map, nullptr, 1, out,
                       Bq, clones, cin, cout, H, W, ng, xmode, POST_DIV, eps}, stream);
}

int drsa_amd_conv_bwd_den_ring(const float* g, const uint8_t* g_amax, const void* wts, int wts_bf16, const float* x,
                               const float* den_ring, const float* den_const4, float* out, int Bq, int clones, int cin,
                               int cout, int H, int W, int ng, int xmode, float eps, void* stream) {
  DRSA_REQUIRE(x && den_ring && den_const4, "conv_bwd_den_ring: needs x, den_ring and den_const4");
  // the compact ring (2W + 8(H - 2) floats per channel at the pooled resolution) needs distinct
  // first / last float4 groups per row and at least two rows: the forward's W % 16, H >= 4 unpooled
  DRSA_REQUIRE(H >= 2 && W >= 8 && W % 8 == 0,
               "conv_bwd_den_ring: needs pooled H >= 2 and W >= 8, W %% 8 == 0 (got %dx%d)", H, W);
  DRSA_REQUIRE(xmode == XM_NONE || xmode == XM_MUL || xmode == XM_SPLIT, "conv_bwd_den_ring: bad xmode");
  DRSA_REQUIRE(((uintptr_t)den_const4 & 15) == 0, "conv_bwd_den_ring: den_const4 must be 16-byte aligned");
  return conv_bwd_run({"conv_bwd_den_ring", g, g_amax, 2, wts, wts_bf16 != 0, x, den_ring, den_const4, 0, out, Bq, clones,
                       cin, cout, H, W, ng, xmode, POST_DIV_RING, eps}, stream);
}

}  // extern "C"
