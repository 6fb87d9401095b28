/*
 * drsa_amd — C ABI of the MI355X (gfx950) DRSA audio-explanation engine.
 *
 * Plain pointers and sizes only; every pointer argument is a DEVICE pointer unless
 * stated otherwise; `stream` is a hipStream_t (NULL = legacy default stream).
 * Every entry point returns 0 on success, a negative DRSA_E* code on an argument
 * error, or a positive hipError_t; it never throws.  drsa_amd_last_error() gives the
 * message of the last failure on the calling thread.
 *
 * Layouts: activations/relevances NCHW fp32 (the reference's torch layout);
 * A, C row-major [N, d] fp32; U row-major [d, d] fp32.
 *
 * Each entry point names the reference interface it replaces (file:line in
 * sharckhai/drsa-audio @ 2024-12-20, paths relative to the repository root).
 */
#ifndef DRSA_AMD_H
#define DRSA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRSA_OK 0
#define DRSA_EINVAL (-1)
#define DRSA_EWORKSPACE (-2)
#define DRSA_EUNSUPPORTED (-3)
#define DRSA_ETIMEOUT (-4)   /* a cooperative kernel's cross-workgroup hand-off timed out (results NaN) */

const char* drsa_amd_last_error(void);
int drsa_amd_version(void);

/* ------------------------------------------------------------------------- *
 * DRSA optimiser (cxai/xai/drsa/drsa.py)
 * Supported: d <= 128, d % K == 0, with dk = d/K padded to DKp = next power of two (<= 64)
 * and DP = next power of two >= max(16, K*DKp) <= 128.  d in {16,32,64,128} runs unpadded;
 * e.g. d = 100, K = 4 (VGGish layer 19, getdrsadata.py:119) runs as DP = 128, DKp = 32.
 * The reference takes every K | d (drsa.py:61-62); the shapes this padded geometry refuses
 * (DKp > 64 or K*DKp > 128: d = 100 with K = 5, 10 or 20, K = 1 at d > 64, ...) run through the
 * drsa_amd_drsa_any_* entry points further down.
 * ------------------------------------------------------------------------- */

/* Bytes of device workspace needed by the drsa_* calls below for N rows (0: unsupported). */
size_t drsa_amd_drsa_workspace_bytes(int64_t N, int d, int K);

/* Floats of the gradient slab gs (DP*DP + DP/DKp, padded coordinates) exchanged between
 * drsa_amd_drsa_partial and drsa_amd_drsa_finish (the all-reduce payload of a sharded run).
 * Equals d*d + K when d is a power of two >= 16 and d/K is a power of two; 0 if unsupported. */
size_t drsa_amd_drsa_slab_floats(int d, int K);

/* Local (shard) pass: gs_out[0:DP*DP] = A^T (R (.) CU) + C^T (R (.) AU) (unscaled gradient,
 * R = relu block sums broadcast over each concept block), gs_out[DP*DP : DP*DP+Kp] = S_k =
 * sum_n relu(s_nk)^2 (padded coordinates; drsa_amd_drsa_slab_floats).  Sum gs_out over
 * shards (e.g. one RCCL all-reduce), then call drsa_amd_drsa_finish with the global row count.
 * Replaces the forward+autograd half of SubspaceOptimizer.run (drsa.py:91-100). */
int drsa_amd_drsa_partial(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                          float* gs_out, void* workspace, size_t workspace_bytes, void* stream);

/* f_out[0] = objective f(U) (objective_fn, drsa.py:224-238); unless objective_only,
 * U_out = polar(U + grad f(U)) (orthogonalize, drsa.py:201-221, on device).
 * iters_out (nullable, device int) receives the Newton-Schulz iteration count; 40 (the iteration
 * limit, see drsa_amd_polar) means U + grad f(U) was singular or nearly so and U_out is finite but not
 * orthogonal (e.g. a zero column of U: its gradient is zero, so it stays one).
 * A concept with no relevance at all (S_k = 0: every relu block sum of concept k is 0) gets the
 * column scale c_k = 0, so its columns of U enter the polar unchanged; f counts its M_k = 0.  The
 * reference's autograd yields NaN there (0 * inf); 0 is this library's contract, pinned by the
 * dead_concept cases of tests/test_polar_paths_gpu.py.  Every run loop (drsa_amd_drsa_run, _run_multi,
 * _run_batched, _any_run) computes the same bits as this entry point does on the slab of the partial
 * entry point of the same geometry and dtype. */
int drsa_amd_drsa_finish(const float* gs, int64_t N_total, int d, int K, const float* U, float* U_out,
                         float* f_out, int objective_only, int* iters_out, void* stream);

/* One fused sharded step (row-sharded DRSA; drsa.py:84-106 split over ranks): from
 * the ALL-REDUCED slab gs of the previous partials (N_total rows over all ranks) and the U they
 * were taken at, U_out = polar(U + G diag(c)) and f(U) -> f_out[0]; then the partial of this
 * rank's N rows at U_out -> gs_out (the next all-reduce's payload; may alias gs).  Equals
 * drsa_amd_drsa_finish followed by drsa_amd_drsa_partial bit for bit, in one launch fewer.
 * Available where drsa_amd_drsa_fused_supported(d, K) returns 1 (padded d = 64, block width
 * <= 16: C3, C4); otherwise use the two-call form. */
int drsa_amd_drsa_fused_supported(int d, int K);
int drsa_amd_drsa_fused_step(const float* A, const float* C, int64_t N, int d, int K, const float* gs,
                             int64_t N_total, const float* U, float* U_out, float* f_out, float* gs_out, void* ws,
                             size_t ws_size, void* stream);

/* Counter-indexed forms for a step loop captured once in a graph and replayed (the sharded loop
 * with its RCCL all-reduce, xai/drsa/distributed.py): f(U) goes to f_traj[*counter] and the device
 * int *counter is incremented by the kernel, so every replay fills the next trajectory slot.
 * Otherwise identical to drsa_amd_drsa_fused_step / drsa_amd_drsa_finish (objective_only = 0). */
int drsa_amd_drsa_fused_step_counted(const float* A, const float* C, int64_t N, int d, int K, const float* gs,
                                     int64_t N_total, const float* U, float* U_out, float* f_traj, int* counter,
                                     float* gs_out, void* ws, size_t ws_size, void* stream);
int drsa_amd_drsa_finish_counted(const float* gs, int64_t N_total, int d, int K, const float* U, float* U_out,
                                 float* f_traj, int* counter, void* stream);

/* One SubspaceOptimizer.run iteration (drsa.py:84-106): f_out[0] = f(U), U_out = new U. */
int drsa_amd_drsa_step(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                       float* U_out, float* f_out, void* workspace, size_t workspace_bytes, void* stream);

/* SubspaceOptimizer.obj_val + objective_fn (drsa.py:122-155): f_out[0] = f(U). */
int drsa_amd_drsa_objective(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                            float* f_out, void* workspace, size_t workspace_bytes, void* stream);

/* SubspaceOptimizer.run(steps) (drsa.py:76-117) without file output: f_traj[0..steps]
 * (steps+1 floats) receives the objective before every update and after the last;
 * U_io holds U_0 on entry and U_steps on exit; U_tmp is d*d scratch; counter is one
 * device int.  use_graph != 0 replays a captured two-step hipGraph (needs a non-NULL
 * stream).  At padded size 128 (d > 64) each step's polar runs on 8 cooperating workgroups
 * that hand X over through the workspace (bit-identical to drsa_amd_drsa_finish's single
 * workgroup).  They wait on each other, so they must become resident together: work running
 * concurrently on other streams only delays them, unless it holds more than 248 CUs while itself
 * waiting on this stream.  A wait that outlives 100 ms (and 20k polls) gives up: U and f are NaN
 * from that step on, the run's later finishes skip straight to NaN, and drsa_amd_drsa_run returns
 * DRSA_ETIMEOUT (it reads the workspace's status word back, synchronising the stream, at d > 64).
 * Inside a caller's stream capture that read is skipped: check drsa_amd_drsa_coop_status after
 * the replay. */
int drsa_amd_drsa_run(const float* A, const float* C, int64_t N, int d, int K, float* U_io, float* U_tmp,
                      int steps, float* f_traj, int* counter, void* workspace, size_t workspace_bytes,
                      int use_graph, void* stream);

/* Status of the cooperative finish of the last drsa_amd_drsa_run / _run_multi on this workspace
 * (same N, d, K): *status_out = 1 if a hand-off timed out (U, f NaN), else 0 (always 0 at d <= 64).
 * Synchronises `stream`; not callable while it is being captured. */
int drsa_amd_drsa_coop_status(const void* workspace, int64_t N, int d, int K, int* status_out, void* stream);

/* ------------------------------------------------------------------------- *
 * DRSA optimiser for every K | d at d <= 128 (the reference's own domain, drsa.py:61-62).
 * The natural geometry: concept blocks at their real columns, DP = next power of two >=
 * max(16, d); the slab is gs[i*DP + j] = Gt[i][j] (i, j < d), gs[DP*DP + k] = S_k (k < K), +0.0
 * elsewhere: DP*DP + K floats.  fp32 A, C only; no fused step and no run_multi / run_batched
 * form.  Each entry point takes the arguments of its namesake above and means the same; a slab
 * or workspace of one family is not valid for the other (drsa_amd_drsa_any_slab_floats /
 * _any_workspace_bytes size them).  Every valid (d, K) is accepted, those of the padded family
 * included (the two families' fp32 summation orders differ, so their results agree to rounding,
 * not bit for bit).  An unsupported (d, K) returns DRSA_EUNSUPPORTED.  drsa_amd_drsa_any_run uses
 * the cooperative finish at d > 64 and returns DRSA_ETIMEOUT like drsa_amd_drsa_run.
 * ------------------------------------------------------------------------- */
int drsa_amd_drsa_any_supported(int d, int K);               /* 1: 0 < d <= 128, K > 0, K | d */
size_t drsa_amd_drsa_any_slab_floats(int d, int K);          /* DP*DP + K; 0 if unsupported */
size_t drsa_amd_drsa_any_workspace_bytes(int64_t N, int d, int K);
int drsa_amd_drsa_any_partial(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                              float* gs_out, void* workspace, size_t workspace_bytes, void* stream);
int drsa_amd_drsa_any_finish(const float* gs, int64_t N_total, int d, int K, const float* U, float* U_out,
                             float* f_out, int objective_only, int* iters_out, void* stream);
int drsa_amd_drsa_any_finish_counted(const float* gs, int64_t N_total, int d, int K, const float* U, float* U_out,
                                     float* f_traj, int* counter, void* stream);
int drsa_amd_drsa_any_step(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                           float* U_out, float* f_out, void* workspace, size_t workspace_bytes, void* stream);
int drsa_amd_drsa_any_objective(const float* A, const float* C, int64_t N, int d, int K, const float* U,
                                float* f_out, void* workspace, size_t workspace_bytes, void* stream);
int drsa_amd_drsa_any_run(const float* A, const float* C, int64_t N, int d, int K, float* U_io, float* U_tmp,
                          int steps, float* f_traj, int* counter, void* workspace, size_t workspace_bytes,
                          int use_graph, void* stream);

/* Test hook: the cooperative finish's spin budget in 100 MHz ticks for launches enqueued from now on
 * (0: give up at the first poll that finds a workgroup missing, with no minimum poll count);
 * -1 restores the default (100 ms and 20k polls). */
int drsa_amd_debug_coop_spin_budget(long long ticks);

/* orthogonalize (drsa.py:201-221): U_out = V (V^T V)^{-1/2}, Newton-Schulz on device, d <= 128.
 * Stop rule (polar_ns.h): iterate X <- X (3I - X^T X)/2 from the scaled V until max|X^T X - I| is
 * below the internal tolerance (4e-7), or stop after the update that starts from d * max|X^T X - I|
 * < 1e-2 (that update provably leaves a spectral error below 0.75 e^2 (1 + e/3) < 7.6e-5, e <= d *
 * max|.|; the typical spread-out error of V = U + G is ~sqrt(d) smaller), or when fp32 rounding is
 * the floor.  So the tolerance is advisory for that last update: orthogonality of the result is the
 * bound above, gated in tests/test_drsa_gpu.py at |U^T U - I| < 2e-6 (step) and 5e-6 (d = 128
 * orthogonalize), by the DRSA trajectories against the reference's fp64 eigh at 1e-4, and in
 * tests/test_polar_paths_gpu.py on ill-scaled and ill-conditioned V (both scaling branches, every
 * exit, 0 to 40 iterations) at 5e-6, with U within 5e-5 of the float64 polar up to condition 1e3.
 * The loop also ends after 40 iterations whatever the error: iters_out (nullable, device int)
 * receives the count, and iters_out == 40 is how a caller sees that V did not converge (a singular
 * or nearly singular V: U_out is then finite but not orthogonal; a converged call reports 40 only if
 * its last update was the 40th, which takes a condition number of about 1e6). */
int drsa_amd_polar(const float* V, int d, float* U_out, int* iters_out, void* stream);

/* compute_subspace_relevances (explainer.py:206-242): out[b][k] = sum_n sum_{j in block k}
 * (act[b][n] U)_j (ctx[b][n] U)_j for act, ctx [B][N][d], d <= 128, K | d.  The workspace
 * (drsa_amd_subspace_relevances_workspace_bytes) holds per-chunk partial sums. */
size_t drsa_amd_subspace_relevances_workspace_bytes(int64_t B, int64_t N, int d, int K);
int drsa_amd_subspace_relevances(const float* act, const float* ctx, int64_t B, int64_t N, int d, int K,
                                 const float* U, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Principal Relevant Component Analysis (csrc/prca.hip): the closed-form baseline of DRSA from the
 * same paper.  The orthonormal U maximising tr(U^T M U), M = (A^T C + C^T A) / (2N), is the
 * eigenvectors of the symmetric indefinite M by descending eigenvalue.  The reference has no PRCA;
 * its habit for a d x d spectral step is a host float64 eigh (orthogonalize, drsa.py:201-221).
 * Any 1 <= d <= 128 (DRSA_EUNSUPPORTED above) and N >= 1.  No call synchronises or allocates.
 * ------------------------------------------------------------------------- */

/* Bytes of device workspace drsa_amd_prca_partial needs for N rows (0: unsupported): one slab per
 * leaf of the fixed row partition (min(256, ceil(N / 16)) leaves, as the DRSA gradient). */
size_t drsa_amd_prca_workspace_bytes(int64_t N, int d);

/* slab[d*d] = A^T C over this call's N rows, un-normalised (fp32 MFMA, each of A and C read once;
 * deterministic: fixed leaves, fixed fold order, no atomics, so the bits depend neither on the
 * device nor on the grid).  Slabs of row shards add up (the payload of an all-reduce). */
int drsa_amd_prca_partial(const float* A, const float* C, int64_t N, int d, float* slab, void* ws, size_t ws_bytes,
                          void* stream);

/* M_out[i][j] = (slab[i][j] + slab[j][i]) / (2 N_total): symmetric bit for bit. */
int drsa_amd_prca_finish(const float* slab, int64_t N_total, int d, float* M_out, void* stream);

/* Eigen-decomposition of the symmetric M [d][d] (its upper triangle is read): w_out[d] descending
 * (stable), V_out[d][d] with eigenvector k in column k, its entry of largest magnitude (lowest
 * index on a tie) positive.  One workgroup, M in LDS, V in registers: cyclic two-sided Jacobi in
 * round-robin order (ceil(d/2) disjoint Rutishauser rotations per step; a pair rests when |m_pq| <=
 * 2^-24 max_k |m_kk|) until a sweep makes no rotation or 30 sweeps have run, so the call ends for
 * any input; then V is re-orthogonalised by the Newton-Schulz polar of drsa_amd_polar and each w_k is
 * the Rayleigh quotient v_k^T M v_k (float64 sum) against the input.  sweeps_out (nullable, device
 * int) receives the sweep count.  The workspace (drsa_amd_syevj_workspace_bytes; 0: unsupported d)
 * is the call's status block of four ints: {sweeps, 1 if the last sweep made no rotation, 0, 0}. */
size_t drsa_amd_syevj_workspace_bytes(int d);
int drsa_amd_syevj(const float* M, int d, float* w_out, float* V_out, int* sweeps_out, void* ws, size_t ws_bytes,
                   void* stream);


/* ------------------------------------------------------------------------- *
 * LRP engine (zennit 0.5.1 rules over the VGG-type CNN; cxai/xai/explain).
 * Enumerations shared by the calls below:
 *   xmode: 0 = R = acc, 1 = R = x * acc, 2 = R = max(x,0)*acc0 + min(x,0)*acc1
 *   post : 0 = none, 1 = g = [x > 0] R / stab(den, eps), 2 = g = [x > 0] R
 * stab(t, eps) = t + eps * (sign(t) + [t == 0])   (zennit Stabilizer)
 * ------------------------------------------------------------------------- */

/* Floats of a prepared conv weight tensor [ng][9 * cin_p][cout_p]. */
size_t drsa_amd_conv_weight_floats(int cin, int cout, int ng);

/* Forward conv3x3 'same' + bias + ReLU [+ max-pool with argmax] and the layer's LRP
 * denominator (Gamma: ng = 2 for x >= 0, where set 1 is applied to x as is, or ng = 3 with
 * the x+ / x- split; den = (z1 + bias[1]) + (z2 + bias[2]), and zennit 0.5.1's Gamma passes
 * bias[2] = 0 because its x- terms' modifiers zero the bias; Epsilon: ng = 1; WSquare/Flat: den_map).
 * pool: 0 = none (out and out_den at full resolution), 1 = 2x2, 2 = 2x4 (VGGish's (2,4) pool,
 * create_model.py:61); pooled: out = window max, out_amax = row-major index of its first
 * maximum (NaN wins, torch max_pool2d), out_den = the denominator at that pixel.
 * Replaces the model forward (create_model.py:91-97) plus the modified forwards zennit's
 * BasicHook re-runs in backward (attribute.py:98-107 via zennit.core.BasicHook).
 * Like every conv entry point below, it needs one sample's channels x H x W < 2^31 (the kernels
 * address a sample's planes with 32-bit offsets); otherwise it returns an error. */
int drsa_amd_conv_fwd(const float* in, const float* wts, const float* bias, const float* den_map, float* out,
                      uint8_t* out_amax, float* out_den, int B, int cin, int cout, int H, int W, int ng,
                      int pool, void* stream);

/* bf16-operand variant of drsa_amd_conv_fwd (the bf16 CNN with fp32 accumulate; the
 * reference has no bf16 path).  The conv input is rounded to bf16 (nearest even) as it is staged,
 * the weights come pre-rounded in the layout [ng][cin_p/16][9 taps][2][cout_p][8] bf16
 * (cin_p = pad32(cin), cout_p = pad32(cout); input channel = 16 chunk + 8 half + j, tap = 3 ky + kx;
 * drsa_amd_conv_weight_bf16_elems elements, 16-byte aligned), products are summed in fp32 on
 * v_mfma_f32_32x32x16_bf16 and everything after the accumulator (bias, ReLU, pool, argmax,
 * denominators) and every output is fp32, exactly as drsa_amd_conv_fwd.  cin > 1 only (the
 * Cin = 1 first layer stays on the fp32 kernel). */
size_t drsa_amd_conv_weight_bf16_elems(int cin, int cout, int ng);
int drsa_amd_conv_fwd_bf16(const float* in, const uint16_t* wts, const float* bias, const float* den_map, float* out,
                           uint8_t* out_amax, float* out_den, int B, int cin, int cout, int H, int W, int ng,
                           int pool, void* stream);

/* 1 if drsa_amd_conv_fwd (bf16 = 0) / drsa_amd_conv_fwd_bf16 (bf16 = 1) has a kernel for this
 * shape and pool mode, else 0 (callers then pool with drsa_amd_maxpool_capture). */
int drsa_amd_conv_fwd_has_kernel(int cin, int cout, int W, int ng, int pool, int bf16);

/* Rule backward of one conv as a transposed conv (flipped/transposed weights), with the
 * max-pool/ReLU backward folded into the input (g_amax != NULL: g at pool resolution) and
 * the next layer's division folded into the output (post).  Bq rows = samples * clones.
 * Replaces zennit's Gamma / Epsilon / WSquare / Flat gradient_mapper + reducer
 * (constants.py:27-51 rule maps). */
int drsa_amd_conv_bwd(const float* g, const uint8_t* g_amax, const float* wts, const float* x, const float* den,
                      float* out, int Bq, int clones, int cin, int cout, int H, int W, int ng, int xmode,
                      int post, float eps, void* stream);

/* bf16-operand variant of drsa_amd_conv_bwd (SURVEY C5 "VGGish-depth CNN bf16": the relevance
 * backward of a bf16 plan; the reference has no bf16 path).  g (the quotient R / stab(den) entering
 * the transposed conv, after the pool backward) is rounded to bf16 (nearest even) as it is staged,
 * the weights come pre-rounded in the forward bf16 layout of the backward weight set:
 * [cin_p/16][9 taps][2][cout_p][8] bf16 with cin = g channels (the forward cout), cout = output
 * channels (the forward cin), both padded to 32 (drsa_amd_conv_weight_bf16_elems(cin, cout, 1)
 * elements, 16-byte aligned); products are summed in fp32 on v_mfma_f32_32x32x16_bf16 and the
 * epilogue (x-multiply, the next layer's division) is fp32 as in drsa_amd_conv_bwd.  ng = 1 and
 * cin >= 16 only (the first layer keeps the fp32 kernel).  Replaces the same zennit rule
 * backward as drsa_amd_conv_bwd (constants.py:27-51). */
int drsa_amd_conv_bwd_bf16(const float* g, const uint8_t* g_amax, const uint16_t* wts, const float* x, const float* den,
                           float* out, int Bq, int clones, int cin, int cout, int H, int W, int ng, int xmode,
                           int post, float eps, void* stream);
/* 1 if drsa_amd_conv_bwd_bf16 has a kernel for this shape (sparse: g at 2x2-pool resolution). */
int drsa_amd_conv_bwd_has_kernel_bf16(int cin, int cout, int W, int ng, int sparse);

/* drsa_amd_conv_bwd_bf16 with g at 2 x pool_w max-pool resolution (pool_w = 4: the VGGish (2,4)
 * pool of block 1, create_model.py:61; pool_w = 2 is drsa_amd_conv_bwd_bf16 with g_amax): the pool
 * backward is folded into the staging (each halo pixel takes its cell's g where the cell's argmax
 * byte, row * pool_w + col, names it), so no unpooled g is written or read.  ng = 1. */
int drsa_amd_conv_bwd_bf16_pw(const float* g, const uint8_t* g_amax, int pool_w, const uint16_t* wts, const float* x,
                              const float* den, float* out, int Bq, int clones, int cin, int cout, int H, int W,
                              int xmode, int post, float eps, void* stream);
/* 1 if drsa_amd_conv_bwd_bf16_pw has a kernel for this shape and pool width. */
int drsa_amd_conv_bwd_has_kernel_bf16_pw(int cin, int cout, int W, int pool_w);

/* The backward conv (fp32 weights: wts_bf16 = 0, ng 1..2, g dense or 2x2-pool-sparse; bf16 weights:
 * wts_bf16 = 1, ng = 1, g dense or 2 x pool_w pool-sparse) with post = POST_DIV whose denominator is
 * the next layer's input-independent WSquare / Flat map den_map [cout][H][W] itself, the same plane
 * for every sample: the layer below is a WSquare / Flat conv NOT followed by a pool (VGGish block 1,
 * block_depth 2: conv0 -> conv3), so its per-sample denominator is the map and no per-sample copy
 * is written or read.  Bit-identical to drsa_amd_conv_bwd{,_bf16,_bf16_pw}(post = POST_DIV) on the
 * copy (replaces the same rule backward, attribute.py:98-107). */
int drsa_amd_conv_bwd_den_map(const float* g, const uint8_t* g_amax, int pool_w, const void* wts, int wts_bf16,
                              const float* x, const float* den_map, float* out, int Bq, int clones, int cin, int cout,
                              int H, int W, int ng, int xmode, float eps, void* stream);
/* 1 when the fp32 backward (drsa_amd_conv_bwd_den_map with g_amax) has a kernel for g at 2 x pool_w
 * pool resolution: the (2,4) pool backward folded into the fp32 staging (VGGish block 1; 2 x 4 cells
 * expanded to their 8 pixels at the LDS store; needs W / 4 % 4 == 0), bit-identical to the unpool
 * followed by the dense-g backward (the same MFMA operands). */
int drsa_amd_conv_bwd_has_kernel_pw(int cin, int cout, int W, int ng, int pool_w);

/* K x K 'same' conv (odd kh, kw in {1, 3, 5, 7}, stride 1, zero padding ((kh-1)/2, (kw-1)/2)) for the
 * VGG-type model's conv_kernel argument (create_model.py:17,58).  Each output is one fp32 fma chain
 * from +0 over k = (ci * kh + ky) * kw + kx ascending (a pixel off the image contributes operand 0);
 * everything after the chain is drsa_amd_conv_fwd at pool = 0 / drsa_amd_conv_bwd with g_amax = NULL,
 * and at kh = kw = 3 the results are the bits of those entry points.
 * Weights: [ng][cin_p * kh * kw][cout_p] fp32, row k as above, cin_p = cin rounded up to 2 (the MFMA's
 * k step), cout_p = cout rounded up to 32, padding zero; bias [3][cout_p].  A backward call names
 * its channels like drsa_amd_conv_bwd (cin = channels of g) and takes the taps flipped:
 * row (co * kh + ky) * kw + kx holds w[co][ci][kh-1-ky][kw-1-kx].
 * drsa_amd_convk_supported (create_model.py:17,58): 1 if the kernels take this geometry; host only. */
int drsa_amd_convk_supported(int kh, int kw, int cin, int cout);
/* Floats of a prepared K x K weight tensor (create_model.py:17,58); 0 if unsupported. */
size_t drsa_amd_convk_weight_floats(int kh, int kw, int cin, int cout, int ng);
/* Forward K x K conv + bias + ReLU at full resolution and the layer's LRP denominator (out_den
 * nullable; den_map non-NULL: out_den is the map's copy), ng as drsa_amd_conv_fwd (create_model.py:17,58).
 * H even, W % 4 == 0. */
int drsa_amd_convk_fwd(const float* in, const float* wts, const float* bias, const float* den_map, float* out,
                       float* out_den, int B, int cin, int cout, int H, int W, int kh, int kw, int ng,
                       void* stream);
/* Rule backward of a K x K conv over a dense g, with xmode / post (0..2) / clones as drsa_amd_conv_bwd
 * (create_model.py:17,58). */
int drsa_amd_convk_bwd(const float* g, const float* wts, const float* x, const float* den, float* out, int Bq,
                       int clones, int cin, int cout, int H, int W, int kh, int kw, int ng, int xmode, int post,
                       float eps, void* stream);

/* WSquare / Flat first layer under a 2x2 max-pool, with its denominator map split for the next
 * backward (zennit WSquare/Flat: den = conv(1; W^2, b^2); constants.py:29 puts
 * WSquare on the first layer).  Such a map holds one value per channel on every pixel off its
 * 1-pixel border ring (each interior pixel sums all 9 taps in the same order), so the denominator
 * at the pool argmax is that value everywhere except near the image border.
 *   drsa_amd_conv_fwd_den_ring: drsa_amd_conv_fwd for cin = 1, pool = 1 and the map den, except
 *       that the per-sample copy of the denominator at the argmax goes only to den_ring, the border
 *       ring of float4 groups stored compactly: per (sample, channel) plane R = 2 W/2 + 8 (H/2 - 2)
 *       floats = [pooled row 0 | pooled row H/2-1 | rows 1..H/2-2 x (columns 0..3, W/2-4..W/2-1)]
 *       (H >= 4, W % 16 == 0).
 *   drsa_amd_conv_bwd_den_ring: drsa_amd_conv_bwd (wts_bf16 = 0) or _bf16 (wts_bf16 = 1) with
 *       post = POST_DIV whose denominator is den_ring (the compact ring above) on the ring and den_const4[c][0..3] (the
 *       map's interior value of channel c, 4 copies, 16-byte aligned) elsewhere.  Here H, W are the
 *       pooled resolution.
 * Together they give bit for bit what drsa_amd_conv_fwd (with out_den) + drsa_amd_conv_bwd(POST_DIV)
 * give, while only ~1/16 of the per-sample denominator copy is ever stored and read, in full
 * coalesced float4s (replace the same rule passes, attribute.py:98-107). */
int drsa_amd_conv_fwd_den_ring(const float* in, const float* wts, const float* bias, const float* den_map, float* out,
                               uint8_t* out_amax, float* den_ring, int B, int cout, int H, int W, int ng,
                               void* stream);
int drsa_amd_conv_bwd_den_ring(const float* g, const uint8_t* g_amax, const void* wts, int wts_bf16, const float* x,
                               const float* den_ring, const float* den_const4, float* out, int Bq, int clones, int cin,
                               int cout, int H, int W, int ng, int xmode, float eps, void* stream);

/* Dense layer forward: z = x W^T + b [, relu(z)]  (classifier Linear layers).  x [M][K], W [N][K] and
 * z_out [M][N] are required; a null bias is a layer without one (0 is added), a null relu_out is not
 * written.  relu(z) keeps a NaN.  Any alignment is accepted: for K % 4 == 0 and K >= 128 the rows are
 * read as float4 when x and W are 16-byte aligned and element by element otherwise, with the same
 * k-ascending chain per output and so the same bits. */
int drsa_amd_linear_fwd(const float* x, const float* W, const float* bias, float* z_out, float* relu_out, int M,
                        int N, int K, void* stream);

/* Dense layer rule backward: g = [z>0?] (R | seed) / stab(z, eps)  ->  out = epi(g W).
 * seed_cls (device int per row) replaces lrp_output_modifier (attribute.py:111-160):
 * R = one_hot ? onehot(cls) : z * onehot(cls).
 * z, W and out are required, and R or seed_cls.  xmode is XM_NONE or XM_MUL (x required); post is
 * POST_NONE, POST_DIV (x and den required) or POST_MASK (x required); any other value is refused. */
int drsa_amd_linear_bwd(const float* R, const int* seed_cls, int one_hot, const float* z, int relu_mask, int rule_eps,
                        float eps, const float* W, const float* x, int xmode, const float* den, int post,
                        float eps_post, float* out, int M, int Nout, int Kin, void* stream);

/* Dense layer under Gamma / ZPlus / WSquare / Flat (reference pf.py:18-27, 257-292: the dense rule
 * comes from the same rule_mapper as the conv rule; zennit rule semantics per SURVEY Appendix A).
 * Wp / Wn and bias_p / bias_n are the rule's modified parameter sets, prepared once by the plan
 * (Gamma: W + gamma W+-; ZPlus: W+-, b+).
 *
 * Forward, one launch: z = x W^T + b (bit-identical to drsa_amd_linear_fwd) [, relu(z)] and
 *   den_p = f(x+; Wp, bias_p) + f(x-; Wn, 0)
 *   den_n = f(x+; Wn, bias_n) + f(x-; Wp, 0)      (only when den_n is given: Gamma without a ReLU after)
 * every term its own k-ordered chain with its bias added last.  x_signed = 0 declares x >= 0: the x-
 * terms are dropped (exactly zero) and x+ = x.  Wn is required when x_signed or den_n.  A null bias,
 * bias_p or bias_n is a layer without that bias: 0 is added to its chain (den_n with a null bias_n is
 * f(x+; Wn, 0) + f(x-; Wp, 0)).  The long-K (K % 4 == 0, K >= 128) float4 path runs only when x and every
 * weight set passed are 16-byte aligned; otherwise the element-wise kernel gives the same bits.
 *
 * Backward, one launch: with R = seed | incoming relevance (through the ReLU mask),
 *   g_p = R [z > 0 when zsign] / stab(den_p, eps),  g_n = R [z < 0] / stab(den_n, eps)  (den_n given)
 *   out = epi( x+ (g_p Wp) + x- (g_p Wn) + x+ (g_n Wn) + x- (g_n Wp) )   summed left to right,
 * the x- terms only when x_signed, the g_n terms only when den_n is given.  xmul = 0 (WSquare / Flat,
 * Wp = W2): out = epi(g_p Wp) with den_p the plan's constant [Nout] (den_bcast = 1).  seed_cls and
 * den / post / eps_post as for drsa_amd_linear_bwd (POST_NONE, POST_DIV or POST_MASK). */
int drsa_amd_linear_rule_fwd(const float* x, const float* W, const float* Wp, const float* Wn, const float* bias,
                             const float* bias_p, const float* bias_n, float* z_out, float* relu_out, float* den_p,
                             float* den_n, int x_signed, int M, int N, int K, void* stream);
int drsa_amd_linear_rule_bwd(const float* R, const int* seed_cls, int one_hot, const float* z, int relu_mask,
                             const float* den_p, const float* den_n, int den_bcast, int zsign, float eps,
                             const float* Wp, const float* Wn, const float* x, int xmul, int x_signed,
                             const float* den, int post, float eps_post, float* out, int M, int Nout, int Kin,
                             void* stream);

/* Projection residual P = U U^T - I (d x d, d <= 128): each entry a float64 fma chain over k
 * ascending minus the identity, rounded once to fp32 (symmetric bit for bit).  Computed once per
 * U (plan preparation); the projection calls below evaluate a' = h U^T as a + a P, so that a' at
 * dead ReLU channels is exact to its rounding. */
int drsa_amd_projection_residual(const float* U, int d, float* P, void* stream);

/* ProjectionModel forward (modify_model.py:75-123): h = a_vec U, a' = h U^T (as a + a P, P from
 * drsa_amd_projection_residual) [, 2x2 pool].
 * h and ap may be NULL (not stored); ap is required when pool == 0 (it is the output).
 * Any D <= 128 (VGGish layer 19: D = 100): zero-padded embedding in the kernel; for D % 4 == 0
 * every value is the unpadded D-term chain. */
int drsa_amd_projection_fwd(const float* a, const float* U, const float* P, float* h, float* ap, float* pooled,
                            uint8_t* amax, int B, int D, int H, int W, int pool, void* stream);

/* Epsilon(invprojection) -> SubspaceHook mask -> Epsilon(projection) -> ReLU backward ->
 * division of the conv rule below (explainer.py:198-203, attribute.py:42-60).
 * fanout == 1: each sample yields K+1 clones (standard + K subspaces); fanout == 2: the K subspace
 * clones only (the standard heatmap is then their sum, drsa_amd_heatmap_sort std_from_sum);
 * fanout == 0: row b is clone (b mod (K+1)) of a replicated batch (explainer.py:92 semantics).
 * ap or h NULL: h and a' are recomputed from a in the kernel (same MFMA order as
 * drsa_amd_projection_fwd, so the result is bit-identical to passing the stored buffers); P is
 * then required. */
int drsa_amd_projection_bwd(const float* gp, const uint8_t* amax, const float* ap, const float* h, const float* a,
                            const float* den, const float* U, const float* P, float* G, int B, int D, int H, int W,
                            int K, float eps_proj, float eps_den, int fanout, void* stream);

/* The two calls above with a matrix per row (mixed-class batches: one DRSA matrix per class).
 * U_tab and P_tab are [n_u][D][D] (each P by drsa_amd_projection_residual); u_row is device int32 [B], one
 * entry per row of a (fanout == 0: per replicated row), and row b runs on matrix u_row[b].  Row b of every
 * output is, bit for bit, what the single-matrix call gives for that row alone with U_tab[u_row[b]].  The
 * kernels clamp an index into [0, n_u - 1], so a bad one reads a wrong matrix of the table, never outside it;
 * validating u_row is the caller's (it is device data).  U_tab, P_tab, u_row non-NULL, n_u >= 1 and
 * 1 <= D <= 128 are required (DRSA_EINVAL), then every check of the single-matrix call. */
int drsa_amd_projection_fwd_multi(const float* a, const float* U_tab, const float* P_tab, const int* u_row, int n_u,
                                  float* h, float* ap, float* pooled, uint8_t* amax, int B, int D, int H, int W,
                                  int pool, void* stream);
int drsa_amd_projection_bwd_multi(const float* gp, const uint8_t* amax, const float* ap, const float* h,
                                  const float* a, const float* den, const float* U_tab, const float* P_tab,
                                  const int* u_row, int n_u, float* G, int B, int D, int H, int W, int K,
                                  float eps_proj, float eps_den, int fanout, void* stream);

/* AlphaBeta on a conv with non-negative input (zennit AlphaBeta as configured at pf.py:285-289,
 * restated in oracle/lrp_ref.py): split R at the conv output into gp = R / stab(den_p) and
 * gn = R / stab(den_n) (den per sample, R rows = sample*clones + clone, n elements per row) ... */
int drsa_amd_ab_split(const float* g, const float* den_p, const float* den_n, float* gp, float* gn, int Bq,
                      int clones, int64_t n, float eps, void* stream);
/* ... and after the two backward convs pos = x J^T_{W+} gp, neg = x J^T_{W-} gn:
 * R_in = alpha*pos - beta*neg, then the post step of the layer below (post as conv_bwd). */
int drsa_amd_ab_combine(const float* pos, const float* neg, float alpha, float beta, const float* x, const float* den,
                        float* out, int Bq, int clones, int64_t n, int post, float eps, void* stream);

/* The post step of a layer as a launch of its own, for a relevance R that the backward above wrote raw
 * (post 0) so that it could be kept (multi-layer DRSA capture): R, out [Bq][n] (out may be R), x, den
 * [Bq / clones][n], x the layer's output.  post 1 (POST_DIV): out = x > 0 ? R / stab(den, eps) : 0;
 * post 2 (POST_MASK): out = x > 0 ? R : 0 (den may be NULL).  The arithmetic of the conv epilogue's
 * post step (IEEE division, no fma), so the result equals a backward launched with that post.  float4
 * loads and stores when n % 4 == 0 and every pointer is 16-byte aligned, scalar ones otherwise (same
 * values).  Any other post, a NULL pointer or a bad shape: DRSA_EINVAL. */
int drsa_amd_relevance_post(const float* R, const float* x, const float* den, float* out, int Bq, int clones,
                            int64_t n, int post, float eps, void* stream);

/* First-layer (one input channel) WSquare / Flat backward: R = J^T_{W2} g.  amax != NULL: g is the
 * pooled relevance (even H, W % 4 == 0, out 16-byte aligned).  amax == NULL: g is dense, any H, W and
 * alignment (float4 loads when W % 4 == 0 and g is 16-byte aligned, scalar loads otherwise; same values). */
int drsa_amd_first_layer_bwd(const float* g, const uint8_t* amax, const float* w2, float* out, int Bq, int clones,
                             int C, int H, int W, void* stream);

/* Input-independent WSquare / Flat denominator map conv(1; W2, b2): [C][H][W]. */
int drsa_amd_first_layer_den(const float* w2, const float* b2, float* den, int C, int CI, int H, int W, void* stream);

/* First-layer (one input channel) ZBox rule (zennit 0.5.1 ZBox) for an input in the box low <= x <= high,
 * W+ = max(W, 0), W- = min(W, 0), b+- likewise; low_img / high_img [H][W] are the bounds spread over one sample.
 *
 * The rule's input-independent maps, [C][H][W] each, wp / wn [C][9], bp / bn [C] or NULL:
 *   zl = conv(low_img; wp) + bp,  zh = conv(high_img; wn) + bn
 * (zero padding: out-of-image taps are skipped; one fma chain per output, taps (ky, kx) ascending, bias last). */
int drsa_amd_first_layer_zbox_maps(const float* wp, const float* bp, const float* wn, const float* bn,
                                   const float* low_img, const float* high_img, float* zl, float* zh, int C, int H,
                                   int W, void* stream);
/* The per-sample denominator den = (a - zl[at]) - zh[at], a = the first conv's forward output of an H x W input.
 * amax != NULL: a, amax, den [B][C][H/2][W/2] (2x2-pooled; at = the cell's argmax pixel, byte = 2 row + col),
 * even H and W, zl and zh 8-byte aligned.  amax == NULL: a, den [B][C][H][W], at = the pixel itself.  C x H x W must stay below 2^31. */
int drsa_amd_first_layer_zbox_den(const float* a, const uint8_t* amax, const float* zl, const float* zh, float* den,
                                  int B, int C, int H, int W, void* stream);
/* The backward: out[q] = (x[q / clones] - low_img) S+ + (x[q / clones] - high_img) S-, S+- = J^T_{W+-} g[q], each one
 * fp32 fma chain per pixel in the order (channel, dy, dx); the products and the sum of the epilogue are rounded one
 * by one.  wpn [2][C][9]: W+ then W-; x [Bq / clones][H][W]; out [Bq][H][W].  g and amax as
 * drsa_amd_first_layer_bwd: amax != NULL: g pooled (even H, W % 4 == 0; out, x, low_img, high_img 16-byte
 * aligned); amax == NULL: g dense, any H, W and alignment.  One sample's C x H x W must stay below 2^31. */
int drsa_amd_first_layer_zbox_bwd(const float* g, const uint8_t* amax, const float* wpn, const float* x,
                                  const float* low_img, const float* high_img, float* out, int Bq, int clones, int C,
                                  int H, int W, void* stream);

/* HeatmapGenerator post-processing (explainer.py:99-123, sort_subspaces 151-176): standard
 * heatmap + relevance, subspace heatmaps sorted by descending relevance, relevances, mask
 * (int64, numpy argsort(...)[..., ::-1] order; relevances are numpy's float32 sums).
 * std_from_sum = 0: hm is [B][K+1][HW] with the standard heatmap first (clone 0);
 * std_from_sum = 1: hm is [B][K][HW] (concept maps only) and the standard heatmap is their sum,
 * k ascending (equal to clone 0 in exact arithmetic: every LRP rule is linear in the relevance). */
int drsa_amd_heatmap_sort(const float* hm, int B, int K, int HW, int std_from_sum, float* std_out, float* std_rel,
                          float* sub_out, float* rel, int64_t* mask, void* stream);

/* One DRSA problem for drsa_amd_drsa_run_multi (all pointers device memory; the fields mean what
 * the same-named arguments of drsa_amd_drsa_run mean). */
typedef struct drsa_amd_problem {
  const float* A;
  const float* C;
  int64_t N;
  int d;
  int K;
  float* U_io;
  float* U_tmp;
  float* f_traj; /* [steps + 1] */
  int* counter;
  void* ws;
  size_t ws_size;
  int dtype; /* 0: A, C fp32; 1 / 2: A, C bf16 / fp16 (uint16 bit patterns), GEMM1 on bf16 / fp16
              * MFMA with fp32 accumulation, padded d >= 32 */
} drsa_amd_problem_t;

/* drsa_amd_drsa_partial with A, C stored as bf16 (C5: bf16 input; the U-projection GEMM runs on
 * bf16 MFMA with fp32 accumulation, U rounded to bf16 per step; the gradient GEMM and every
 * reduction stay fp32).  No reference bf16 path exists: its tolerance is looser (tests).
 * Padded d >= 32 (the 16-bit MFMA tiles are 32 deep): DRSA_EUNSUPPORTED at padded d = 16. */
int drsa_amd_drsa_partial_bf16(const uint16_t* A, const uint16_t* C, int64_t N, int d, int K, const float* U,
                               float* gs_out, void* ws, size_t ws_size, void* stream);
/* The same with A, C as fp16 (C5's "fp16 MFMA projection": v_mfma_f32_16x16x32_f16, U rounded to
 * fp16 once per launch, fp32 accumulate; everything after GEMM1 fp32). */
int drsa_amd_drsa_partial_f16(const uint16_t* A, const uint16_t* C, int64_t N, int d, int K, const float* U,
                              float* gs_out, void* ws, size_t ws_size, void* stream);

/* P independent problems advanced S steps together (C5: two layers, K=16 each, one graph).
 * Replaces the sequential per-layer loop of optsubspaces.py:18-23 / drsa.main. */
/* Returns DRSA_ETIMEOUT like drsa_amd_drsa_run when a problem's cooperative finish timed out.
 * Capturable: inside a caller's stream capture it records the per-problem chains on forked side
 * streams (a per-thread pool that outlives the call) joined back into `stream`, and skips its own
 * graph and the status read-back (drsa_amd_drsa_coop_status per problem after the replay). */
int drsa_amd_drsa_run_multi(int P, const drsa_amd_problem_t* probs, int steps, int use_graph, void* stream);

/* P independent fp32 problems sharing one padded geometry (same pow2(d) and concept width; N may
 * differ) advanced together with ONE launch per phase for all of them: every problem's partial
 * on about `blocks` workgroups (0: about sixteen waves of workgroups over the chip), each owning whole
 * groups of the fixed 256-leaf row partition that drsa_amd_drsa_run uses, the slab reduces, then
 * every problem's finish on its own workgroup.  The task-parallel DRSA grid of the reference's
 * cluster driver (optsubspaces.py:17-23: classes x layers x runs, each drsa.main(..., steps=5000)).
 * Fields of probs mean what they mean for drsa_amd_drsa_run_multi (dtype must be 0).  Every
 * problem's trajectory and U equal drsa_amd_drsa_run's bit for bit, for any `blocks`.  Not stream-
 * capturable (it allocates its descriptor table); synchronises the stream before returning. */
int drsa_amd_drsa_run_batched(int P, const drsa_amd_problem_t* probs, int steps, int blocks, int use_graph,
                              void* stream);

/* ------------------------------------------------------------------------- *
 * Log-mel front end
 * Replaces cxai/utils/dataloading.py:62-74 + :138-176 (Loader: torchaudio
 * Spectrogram(n_fft, hop, power=None) -> MelScale(n_mels) -> log10(+log_eps) -> clamp ->
 * frames [frame0, frame0+width)) fused with cxai/utils/sound.py:8-44 (get_slice chunking)
 * and :67-70 (peak_normalizer).
 *   wav: songs [n_songs] at stride song_stride floats; chunk c of a song starts at
 *        c*chunk_hop and is chunk_len samples long (get_slice's unfold).
 *   window: [n_fft] analysis window (torch.hann_window(n_fft), periodic).
 *   band_*: the mel filterbank [n_fft/2+1, n_mels] in band form: filter m covers FFT bins
 *        band_lo[m] .. band_lo[m]+band_n[m]-1 with weights band_w[band_off[m] ...].
 *   peak_norm: divide each chunk by its max |x| (peak_normalizer).
 *   out: [n_songs*chunks_per_song, n_mels, width] fp32.
 * Needs n_fft/2 = 2^a 3^b 5^c; LDS footprint (drsa_amd_logmel_smem_bytes) <= 160 KB.
 * ------------------------------------------------------------------------- */
int drsa_amd_logmel_smem_bytes(int n_fft, int hop, int n_mels, int width, int band_nnz);
int drsa_amd_logmel(const float* wav, int64_t n_songs, int64_t song_stride, int chunks_per_song, int64_t chunk_hop,
                    int chunk_len, int n_fft, int hop, int n_mels, int width, int frame0, const float* window,
                    const int* band_lo, const int* band_n, const int* band_off, const float* band_w, int band_nnz,
                    int peak_norm, int clamp, float clamp_min, float log_eps, float* out, void* stream);

/* ------------------------------------------------------------------------- *
 * DRSA training data: cxai/xai/drsa/preprocessing.py:18-256 and
 * cxai/xai/drsa/cluster/getdrsadata.py:47-59.
 * ------------------------------------------------------------------------- */

/* ph x pw max-pool (stride = kernel) of a full-resolution ReLU output with the engine's argmax
 * byte (dy*pw + dx of the first maximum) and the rule denominator gathered at the argmax (den
 * may be NULL).  Keeps the layer-j activation map for DRSA data (the reference's store_hook,
 * preprocessing.py:92-103) and runs the pools the fused conv epilogue does not (VGGish (2,4),
 * create_model.py:61 pool_kernels). */
int drsa_amd_maxpool_capture(const float* a, const float* den, float* y, uint8_t* amax, float* den_pooled, int B,
                             int C, int H, int W, int ph, int pw, void* stream);

/* Full-resolution map from its pooled form + argmax (ph x pw pool): layer.output.grad of
 * get_intermediate (preprocessing.py:156-158), and the max-pool backward of pools other than
 * 2x2.  rel rows are sample*clones + clone, amax rows are samples.  out [Bq, C, H, W]. */
int drsa_amd_relevance_unpool(const float* rel, const uint8_t* amax, int Bq, int clones, int C, int H, int W, int ph,
                              int pw, float* out, void* stream);

/* ph x pw average pool (stride = kernel, no padding) of a full-resolution ReLU output a [B][C][H][W] into
 * y [B][C][H/ph][W/pw]: y = s / float(ph * pw), s one fp32 chain from 0 over the window in row-major order
 * (rows outer, columns inner), then one IEEE division: torch's CPU avg_pool2d, bit for bit.  Any window
 * that divides the map, the whole map included (a chain per output, never a tree).  float4 loads when pw is
 * 1, 2 or 4, W % 4 == 0 and both pointers are 16-byte aligned; scalar ones otherwise (same values). */
int drsa_amd_avgpool_fwd(const float* a, float* y, int B, int C, int H, int W, int ph, int pw, void* stream);

/* The way back through that block, from the relevance R_y [Bq][C][H/ph][W/pw] at the pool's output (rows
 * sample * clones + clone) to the dense g [Bq][C][H][W] of the block's conv backward, in one launch.  With
 * K = float(ph * pw) and pixel p in window (i, j):
 *   rule 0 (plain gradient of the pool):   t[p] = R_y[i,j] / K
 *   rule 1 (Epsilon / Norm on the pool):   t[p] = a[p] * ((R_y[i,j] / stab(y[i,j], eps_pool)) / K)
 *   rel_full[p] = t[p] (when rel_full != NULL: the relevance at the ReLU's output, [Bq][C][H][W])
 *   g[p] = a[p] > 0 ? (den ? t[p] / stab(den[p], eps_conv) : t[p]) : 0
 * a [Bq / clones][C][H][W] and y [Bq / clones][C][H/ph][W/pw] are the forward's; y may be NULL under rule 0.
 * den is the conv rule's denominator at full resolution: [Bq / clones][C][H][W] (den_bcast 0), the shared map
 * [C][H][W] (den_bcast 1), or NULL (a conv without a rule).  IEEE divisions, no fma.  W % 4 == 0; a, den, g
 * and rel_full 16-byte aligned (float4 rows); any other argument error: DRSA_EINVAL. */
int drsa_amd_avgpool_bwd(const float* R_y, const float* y, const float* a, const float* den, int den_bcast, int rule,
                         float eps_pool, float eps_conv, float* g, float* rel_full, int Bq, int clones, int C, int H,
                         int W, int ph, int pw, void* stream);

/* Activation vectors and context vectors C = R / (A + 1e-7) at sampled locations
 * (get_vectors_from_maps + compute_context_vectors, preprocessing.py:179-193, 234-256).
 *   act [B, C, H, W]; rel full [B, C, H, W] (rel_amax NULL) or pooled [B, C, H/ph, W/pw] + argmax.
 *   idx [B, L] int32 flat locations (sample_spatial_locations), or NULL = every location
 *   (L = H*W, inference branch, [B, H*W, C]).
 *   layout 0 = the reference's get_vectors_from_maps row order (transpose-then-reshape),
 *   layout 1 = one row per (sample, location).  A_out, C_out [B*L, C]. */
int drsa_amd_drsa_vectors(const float* act, const float* rel, const uint8_t* rel_amax, const int* idx, int B, int C,
                          int H, int W, int ph, int pw, int L, int layout, float* A_out, float* C_out, void* stream);

/* normalize_vectors (preprocessing.py:219-231): out = v / sqrt(mean(v^2)) / d^(1/4) over all
 * n elements (deterministic fp64 reduction).  out may alias v. */
size_t drsa_amd_normalize_workspace_bytes(void);
int drsa_amd_normalize_vectors(const float* v, int64_t n, int d, float* out, void* ws, size_t ws_bytes, void* stream);

/* The same normalisation over rows spread across ranks (getdrsadata.py:47-59 normalises the whole
 * 1000-sample x 20-location set at once, preprocessing.py:229-231):
 *   drsa_amd_normalize_sumsq: this rank's sum of v^2 -> sum_out[0] (fp64, device; the fixed-order
 *       reduction of drsa_amd_normalize_vectors; 0 for n == 0);
 *   drsa_amd_normalize_scale: E = sqrt((sums[0] + ... + sums[nsums-1], in that order) / n_total),
 *       out = v / E / d^(1/4) over this rank's n elements.  sums are the ranks' sum_out values in
 *       rank order (one all-gather), n_total the element count over all ranks.  out may alias v.
 * With nsums = 1 and n_total = n this is drsa_amd_normalize_vectors up to the fp64 sum's last bit. */
int drsa_amd_normalize_sumsq(const float* v, int64_t n, void* ws, size_t ws_bytes, double* sum_out, void* stream);
int drsa_amd_normalize_scale(const float* v, int64_t n, int d, const double* sums, int nsums, int64_t n_total,
                             float* out, void* stream);

/* ---------------------------------------------------------------------------
 * Concept audio (cxai/xai/explain/audiogen.py, Mel2Audio): heatmaps -> waveforms.  csrc/audiogen.hip.
 * Shape rules of the transforms: n_fft even, n_fft/2 = 2^a 3^b 5^c, 1 <= hop <= n_fft, power 1 or 2.
 * ------------------------------------------------------------------------- */

/* Analysis of n_chunks waveforms (chunk i at wav + i*chunk_stride, chunk_len samples): centred,
 * reflect-padded STFT with `window`, frames frame0..frame0+width-1.
 *   mel [n_chunks, n_mels, width]        the band-form filterbank (as drsa_amd_logmel) on |X|^power
 *   X   [n_chunks, width, n_fft/2+1, 2]  the complex spectrum (re, im), frame-major
 * peak_norm != 0 divides each chunk by its max |x| first (peak_normalizer). */
int drsa_amd_stft_mel_phase(const float* wav, int64_t n_chunks, int64_t chunk_stride, int chunk_len, int n_fft,
                            int hop, int n_mels, int width, int frame0, int power, const float* window,
                            const int* band_lo, const int* band_n, const int* band_off, const float* band_w,
                            int band_nnz, int peak_norm, float* mel, float* X, void* stream);

/* generate_mask for n_maps maps [H, W]: hp = relu(h); with a rank r >= 0 keep hp where hp > a[r]
 * (a = the map's sorted hp; r = floor(p/100 (H*W-1)) is "hp > np.percentile(hp, p)"), r = -1 keeps
 * all; then the separable Gaussian blur with `taps` [k] (k odd) and reflect padding k/2.  Map i
 * uses rank_first when i % group == 0, else rank_rest.  The map lives in LDS: DRSA_EUNSUPPORTED
 * when H*W floats and the tables exceed 160 KB. */
int drsa_amd_heatmap_mask(const float* heatmaps, int64_t n_maps, int H, int W, int group, int rank_first,
                          int rank_rest, const float* taps, int k, float* mask, void* stream);

/* Host only (no device work): envelope_host[s], s < hop*(width-1), the overlap-added window^2 at
 * padded position s + n_fft/2 for `width` frames (fp64 sums, rounded once).  DRSA_EINVAL when it
 * is not above 1e-11 everywhere in that span (torch.istft's check). */
int drsa_amd_istft_envelope(const float* window_host, int n_fft, int hop, int width, float* envelope_host);

/* For each of n_src sources and its C masks: mag = relu(P (mel * mask))^(1/power) with
 * pinv_t = P^T [n_mels, n_fft/2+1]; Y = mag * X/|X| (1 where |X| = 0); istft(Y, center=True):
 * inverse real FFT, * window, overlap-add at hop, / envelope, n_fft/2 samples dropped at each end.
 *   mask [n_src, C, n_mels, width];  audio [n_src, C, hop*(width-1)].
 * Every sample has a fixed summation order: an audio is bit-identical in any batch. */
int drsa_amd_mel_to_audio(const float* mel, const float* X, const float* mask, int64_t n_src, int C, int n_fft,
                          int hop, int n_mels, int width, int power, const float* window, const float* pinv_t,
                          const float* envelope, float* audio, void* stream);

/* In place over n_audio rows of len samples: a / max|a| (a silent row becomes NaN, as the
 * reference), then, when wav != NULL, adjust_vol against the row's source waveform
 * wav + (row / C) * wav_stride: clamp(a * |rms(wav) / rms(a)|, -1, 1). */
int drsa_amd_audio_normalize(float* audio, int64_t n_audio, int len, const float* wav, int64_t wav_stride,
                             int wav_len, int C, void* stream);

/* ---------------------------------------------------------------------------
 * Concept audio at STFT resolution: relevance through the mel filterbank.  csrc/stft_audio.hip.
 * mel and X are drsa_amd_stft_mel_phase's outputs with power = 1 (the model's front end:
 * frame0 = 1); X must be 8-byte aligned.
 * ------------------------------------------------------------------------- */

/* The LRP z-rule through the filterbank, for n_src sources and the C maps of each:
 *   q[m][t] = relevance[m][t] / (mel[m][t] + eps)          (one add, one IEEE division; eps > 0)
 *   a[f][t] = sum over the bands m that cover bin f, ascending m, one fmaf chain from 0, of fb[f][m] q[m][t]
 *   out[f][t] = |X[t][f]| a[f][t]
 * The filterbank comes bin by bin (the transposed band form of drsa_amd_logmel's tables): bin f is
 * covered by bands bin_lo[f] .. bin_lo[f]+bin_n[f]-1 with weights bin_w[bin_off[f] ..] (bin_nnz in all).
 *   relevance [n_src, C, n_mels, width];  mel [n_src, n_mels, width];  X [n_src, width, n_freq, 2];
 *   out [n_src, C, n_freq, width].
 * A source's maps are bit-identical in any batch.  DRSA_EUNSUPPORTED when the 32-frame tiles
 * (n_freq x 33 + 2 x n_mels x 32 floats and the tables) exceed 160 KB of LDS. */
int drsa_amd_mel_relevance_to_stft(const float* relevance, const float* mel, const float* X, int64_t n_src, int C,
                                   int n_mels, int width, int n_freq, const int* bin_lo, const int* bin_n,
                                   const int* bin_off, const float* bin_w, int bin_nnz, float eps, float* out,
                                   void* stream);

/* drsa_amd_heatmap_mask (same arguments, bit-identical results on every map both accept) with the
 * map in global memory instead of LDS: for maps of up to H*W = 4 194 304 (2^22) elements, e.g.
 * 401 x 128 or 513 x 512; DRSA_EUNSUPPORTED above that.  The threshold comes from integer
 * counters only and no workgroup waits for another one. */
int drsa_amd_heatmap_mask_large(const float* heatmaps, int64_t n_maps, int H, int W, int group, int rank_first,
                                int rank_rest, const float* taps, int k, float* mask, void* stream);

/* For each of n_src sources and its C masks: Y[t][f] = mask[f][t] X[t][f], then istft(Y, center=True)
 * as drsa_amd_mel_to_audio: inverse real FFT (the imaginary parts of bins 0 and n_fft/2 dropped),
 * * window, overlap-add at hop in ascending frame order, / envelope, n_fft/2 samples dropped at
 * each end.  No mel, no pseudo-inverse: an all-ones mask returns the analysed signal.
 *   X [n_src, width, n_fft/2+1, 2];  mask [n_src, C, n_fft/2+1, width];  audio [n_src, C, hop*(width-1)].
 * An audio is bit-identical in any batch.  The transforms' shape rules hold; DRSA_EUNSUPPORTED
 * when n_fft/hop overlaps more than 9 frames or the LDS need exceeds 160 KB. */
int drsa_amd_stft_mask_to_audio(const float* X, const float* mask, int64_t n_src, int C, int n_fft, int hop,
                                int width, const float* window, const float* envelope, float* audio, void* stream);

/* ---------------------------------------------------------------------------
 * Whole-track explanations: overlapping chunks' maps stitched into one track-length map per
 * concept (xai/explain/track.py, DESIGN.md "Whole-track explanations").  csrc/track_stitch.hip.
 * ------------------------------------------------------------------------- */

/* n chunks of width W, chunk c starting at track column c*h (1 <= h <= W), Wt = (n-1)*h + W:
 *   std_maps [n, 1, H, W]   standard maps; NULL: C = K output maps and no map 0
 *   sub      [n, K, H, W]   concept maps in each chunk's own slot order
 *   order    [n, K] int64   order[c][j] = the concept in slot j of chunk c (HeatmapGenerator's "mask");
 *                           NULL = identity
 *   taper    [W]            weights, strictly positive (a precondition: they are device data)
 *   out      [C, H, Wt]     C = K + 1 (K when std_maps = NULL): map 0 the standard map, map k concept k - 1
 *   act      [C, Wt]        act[k][u] = sum over the rows r of out[k][r][u]
 * Column u is covered by the chunks c = max(0, ceil((u - W + 1) / h)) .. min(n - 1, u / h), with
 * t = u - c*h.  Over them, c ascending:
 *   num = one fmaf(taper[t], x_c[r][t], num) chain from +0;  den = the plain sum of taper[t];
 *   out[k][r][u] = num / den (IEEE division).
 * act: rows go in blocks of 32; in a block, the 8 sums over the rows r = j (mod 8), r ascending, each
 * from +0, are added j ascending from +0; the blocks' sums are added block ascending from +0.
 * No atomics: out and act are bit-identical from run to run.
 * order on the device is not read on the host: the caller guarantees that every row is a permutation
 * of 0..K-1 (a slot that names no concept of 0..K-1 is ignored; a concept no slot names reads slot 0).
 * An order in host memory is checked here (DRSA_EINVAL), and refused when it is pageable memory
 * that the device cannot read.  16-byte accesses when W, h are multiples of 4 and every pointer is
 * 16-byte aligned, 4-byte accesses otherwise; the results do not depend on which.
 * ws: drsa_amd_track_stitch_workspace_bytes(C, H, Wt) bytes (0 when H <= 32): the row blocks' partial
 * act sums.  There is no empty problem: n, K, H >= 1 are required. */
size_t drsa_amd_track_stitch_workspace_bytes(int C, int H, int64_t Wt);
int drsa_amd_track_stitch(const float* std_maps, const float* sub, const int64_t* order, const float* taper, int n,
                          int K, int H, int W, int h, float* out, float* act, void* ws, size_t ws_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DRSA_AMD_H */
