/* a2s.h -- C ABI of liba2s_hip.so: hand-written HIP (gfx950 / CDNA4) kernels for the data-parallel training
 * hot path of piano-a2s (models.ScoreTranscription forward/backward, loss, clip + Adadelta).
 *
 * The reference has no native layer: every operation below replaces a torch.nn call made by
 * /root/reference/models.py (cited per function) that would otherwise run through ATen -> cuDNN/cuBLAS.
 * The boundary a maintainer binds is this file; INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - every tensor is a plain device pointer to fp32 unless stated (ids: int64 `long long` or int32);
 *     the library BORROWS pointers for the duration of the call and owns no memory;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); calls only
 *     enqueue work -- they never allocate and never synchronise, with ONE documented exception:
 *     a2s_note_decoder_fwd in greedy mode polls a device counter every `poll` steps;
 *   - return value 0 = ok, negative = error (A2S_ERR_*), message via a2s_last_error(); never throws;
 *   - scratch memory is caller-allocated; *_workspace_bytes() say how much;
 *   - one host thread per process / GPU (torchrun model); ordering is by stream.
 */
#ifndef A2S_H
#define A2S_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define A2S_OK 0
#define A2S_ERR_ARG (-1)
#define A2S_ERR_HIP (-2)
#define A2S_ERR_WORKSPACE (-3)

const char* a2s_last_error(void);
int a2s_version(void);
/* kernel launches issued by this process through the library so far (diagnostic: launches per optimizer / decode step in bench.py;
 * the reference has no native layer, nothing replaced) */
long long a2s_launch_count(void);

/* ---- dense contraction: every nn.Linear / GRU projection of models.py (:68,:123-132,:359,:444-445,:504) and
 * their backward forms.  C[m,n] = act(alpha * sum_k A(m,k) B(k,n) + beta*C + bias[n]);
 * A(m,k)=A[m*sAm+k*sAk], B(k,n)=B[k*sBk+n*sBn]; act 0 none / 1 relu / 2 tanh / 3 exp(2x) (the attention key image below); split-K is deterministic
 * (splitk 0 = pick automatically for skinny problems when a workspace is supplied). */
int a2s_gemm_f32(void* stream, int M, int N, int K, float alpha, const float* A, long sAm, long sAk,
                 const float* B, long sBk, long sBn, float beta, float* C, long ldc, const float* bias, int act,
                 int batch, long bsA, long bsB, long bsC, int splitk, float* workspace, size_t workspace_bytes);
/* The same with BatchNorm + ReLU of an operand applied while it is staged: element -> max(0, e*scale[c] + shift[c]), c = (index along
 * the operand's unit-stride dimension) / period; NULL scale = operand taken as is.  The 19200->256 Linear (models.py:537-539) reads the
 * last convolution's pre-BN output this way (forward: A; weight gradient: B), so the activated tensor is never materialised. */
int a2s_gemm_f32_affine(void* stream, int M, int N, int K, float alpha, const float* A, long sAm, long sAk, const float* B, long sBk,
                        long sBn, float beta, float* C, long ldc, const float* bias, int act, int batch, long bsA, long bsB, long bsC,
                        int splitk, float* workspace, size_t workspace_bytes, const float* a_scale, const float* a_shift, int a_period,
                        const float* b_scale, const float* b_shift, int b_period);
/* C = A B whose output (M rows x N = channels * period columns, same layout as y) is the gradient wrt relu(bn(y)) of a ConvStack layer (the
 * data gradient of the 19200->256 Linear): its BatchNorm-backward statistics (sum g', sum g' xhat per channel) are accumulated in the
 * epilogue into partial[a2s_gemm_bnstats_blocks(M, period)][N / period][2] -- the layout a2s_bn_bwd_from_partial reads. */
int a2s_gemm_f32_bnstats(void* stream, int M, int N, int K, const float* A, long sAm, long sAk, const float* B, long sBk, long sBn, float* C, long ldc,
                         const float* y, const float* mean, const float* invstd, const float* scale, const float* shift, int period, float* partial);
/* The two entries above on the two-term fp16 split (three matrix-core products instead of the six of the three-term bf16 split, same
 * fp32-level accuracy; 128x128 tiles with k- or row-contiguous operands, otherwise the call runs as the unscaled entry): a_absmax /
 * b_absmax are device scalars holding max |A| / max |B| (a2s_absmax, or the BatchNorm backward's a2s_bn_bwd_amax), from which the kernel
 * derives exact power-of-two operand scales; NULL = that operand is O(1) (post-BatchNorm activations) and is used as is.  Switch:
 * a2s_debug_set("gemm_f16x2", 0/1) (default 1; environment: A2S_ARITH). */
int a2s_gemm_f32_affine_scaled(void* stream, int M, int N, int K, float alpha, const float* A, long sAm, long sAk, const float* B, long sBk,
                               long sBn, float beta, float* C, long ldc, const float* bias, int act, int batch, long bsA, long bsB, long bsC,
                               int splitk, float* workspace, size_t workspace_bytes, const float* a_scale, const float* a_shift, int a_period,
                               const float* b_scale, const float* b_shift, int b_period, const float* a_absmax, const float* b_absmax);
int a2s_gemm_f32_bnstats_scaled(void* stream, int M, int N, int K, const float* A, long sAm, long sAk, const float* B, long sBk, long sBn, float* C, long ldc,
                                const float* y, const float* mean, const float* invstd, const float* scale, const float* shift, int period, float* partial,
                                const float* a_absmax, const float* b_absmax);
/* Round 4: the data gradient of the ConvStack's 19200 -> 256 Linear (reference models.py:68; backward of y = relu(bn4(y4)) W^T) as a kernel of
 * its own (csrc/a2s_linear.hip): da (M x N) = dz (M x 256, leading dimension lda) * Wt^T with Wt (N x 256) the k-contiguous copy of the weight,
 * plus the BatchNorm-backward statistics of a2s_gemm_f32_bnstats_scaled into partial[a2s_linear_dgrad_blocks(M)][N / period][2] (same
 * consumer).  K must be 256, N % 32 == 0, period % 32 == 0; workspace: a2s_linear_dgrad_ws_bytes(N, 256) bytes (the weight as fp16 term
 * planes), 16-byte aligned.  da_absmax_out (device scalar, may be NULL): max |da| is folded into it by atomic max (zero it before the call).
 * a2s_linear_dgrad_eligible says whether a shape qualifies (otherwise call a2s_gemm_f32_bnstats_scaled). */
int a2s_linear_dgrad_bnstats(void* stream, int M, int N, int K, const float* dz, long lda, const float* Wt, float* da, long ldc, const float* y,
                             const float* mean, const float* invstd, const float* scale, const float* shift, int period, float* partial,
                             const float* dz_absmax, const float* w_absmax, float* workspace, size_t workspace_bytes, float* da_absmax_out);
/* ... and its forward (reference models.py:68,537-539): z (M x 256, leading dimension ldc) = relu(y * scale[k / period] + shift[k / period]) W^T
 * with y (M x K, leading dimension lda) and W (256 x K) row-major; scale / shift NULL: y as it is.  N must be 256, K % 64 == 0, period % 32 == 0;
 * y_absmax: device scalar bounding the ACTIVATED operand (a2s_act_bound; NULL: O(1)); workspace: a2s_linear_dgrad_ws_bytes(256, K) bytes.
 * a2s_linear_fwd_eligible says whether a shape qualifies (otherwise a2s_gemm_f32_affine_scaled). */
int a2s_linear_fwd(void* stream, int M, int N, int K, const float* y, long lda, const float* W, float* z, long ldc, const float* scale, const float* shift,
                   int period, const float* y_absmax, const float* w_absmax, float* workspace, size_t workspace_bytes);
int a2s_linear_fwd_eligible(int M, int N, int K, int period);
/* ... and its weight gradient: G (256 x K, leading dimension ldg) += dz^T relu(y * scale[k / period] + shift[k / period]) with dz (M x 256, leading
 * dimension ldz); N must be 256, K % 128 == 0, period % 4 == 0, M >= 64; dz_absmax: device scalar max |dz|; y_absmax as in a2s_linear_fwd;
 * workspace: a2s_linear_wgrad_ws_bytes(M, K) bytes (dz as fp16 term planes + the split-K slabs).  Deterministic (fixed-order reduction). */
int a2s_linear_wgrad(void* stream, int M, int N, int K, const float* dz, long ldz, const float* y, long lda, float* G, long ldg, const float* scale,
                     const float* shift, int period, const float* dz_absmax, const float* y_absmax, float* workspace, size_t workspace_bytes);
size_t a2s_linear_wgrad_ws_bytes(int M, int K);
int a2s_linear_wgrad_eligible(int M, int N, int K, int period);
/* The same kernel for any product over a tall reduction index (M = B*T rows; the encoder GRU's weight gradients, the attention key products):
 *   transposed = 0:  G[n][k] += sum_m P[m][n] A[m][k]   (G: Np x K, leading dimension ldg)
 *   transposed = 1:  G[k][n] += sum_m P[m][n] A[m][k]   (G: K x Np)
 *   bias (may be NULL):  bias[k] += sum_m A[m][k]
 * P (M x Np, leading dimension ldp, Np % 256 == 0) is packed once into fp16 term planes, A (M x K, leading dimension lda, K % 128 == 0) is streamed
 * from memory exactly once when Np == 256; a column offset into a wider tensor is part of the pointer.  Every base address 16-byte aligned, lda % 4 == 0,
 * ldg % 4 == 0, M >= 64.  p_absmax / a_absmax: device scalars bounding |P| / |A|.  workspace: a2s_tallk_wgrad_ws_bytes(M, Np, K) bytes.
 * Deterministic: fixed-order reduction over the row ranges, for G and for bias.  a2s_tallk_wgrad_eligible says whether a shape qualifies and the
 * switch "tallk_wgrad" (a2s_debug_set) is on; otherwise call a2s_gemm_f32_affine_scaled and a2s_col_sum. */
int a2s_tallk_wgrad(void* stream, int M, int Np, int K, const float* P, long ldp, const float* A, long lda, float* G, long ldg, int transposed, float* bias,
                    const float* p_absmax, const float* a_absmax, float* workspace, size_t workspace_bytes);
size_t a2s_tallk_wgrad_ws_bytes(int M, int Np, int K);
int a2s_tallk_wgrad_eligible(int M, int Np, int K, long ldp, long lda, long ldg, int transposed);
size_t a2s_linear_dgrad_ws_bytes(int N, int K);
int a2s_linear_dgrad_blocks(int M);
int a2s_linear_dgrad_eligible(int M, int N, int K, int period);
/* out[0] = max |x[i]| over n floats (device scalar) */
int a2s_absmax(void* stream, const float* x, long n, float* out);
int a2s_gemm_bnstats_blocks(int M, int period);
size_t a2s_gemm_workspace_bytes(int M, int N, int batch, int splitk);
int a2s_gemm_pick_splitk(int M, int N, int K, int batch);
/* tuning aid (tools/gemm_sweep.py): force the tile configuration for M > 64 (1: 32x64, 2: 64x32, 3: 64x64, 4: 128x128; 0: heuristic) */
void a2s_gemm_debug_tile(int cfg);
/* measurement switches for A/B runs (tools/ab_step.py): "gru_fused" 0/1 (one-launch recurrent step), "gemm_tile" as above,
 * "conv_bf16x3" bit mask -- which 3x3 convolutions run on the bf16 matrix pipes with every fp32 operand split exactly into three bf16
 * terms (six products, fp32-level accuracy; csrc/a2s_conv.hip conv3x3_bf16x3): bit 0 forward launches, bit 1 data-gradient launches
 * (default 3; 0 = the fp32-input MFMA kernel everywhere); "gemm_bf16x3" 0/1 -- the same split for 128x128 GEMM tiles whose two
 * operands are k- or row-contiguous (default 1); "wgrad_bf16x3" 0/1/2 -- the split-operand weight-gradient convolution: 1 (default) where it is
 * faster than conv3x3_wgrad (40 -> 40 channels), 2 every eligible launch;
 * "attn_defer_combine" 0/1 (default 1): inside a2s_note_decoder_fwd, the few-clip attention launches of a training call
 * leave their softmax combine to the GRU-step kernel that consumes the contexts (csrc/a2s_step.hip dec_gru_step_cmb; same bits as the combine
 * kernel); "dec_mid" 0/1 (default 1, round 6): the launch-per-step loop's GRU cell, output + next query and backward products on the mid-size
 * fused kernels (0: library-style products; read-only "dec_mid_launches" counts them);
 * "attn_deep" n (default 24): training launches over at most n clips use the one-round-trip forward sweep */
int a2s_debug_set(const char* key, int value);
int a2s_debug_get(const char* key);   /* current value of "conv_bf16x3" / "gemm_bf16x3" / "wgrad_bf16x3" / "gru_fused"; -1 for an unknown key;
                                        * also "device_cus" / "device_xccs": compute units and XCDs the runtime reports for the current device */
/* The library reads the environment variables that override a switch's default (A2S_CONV_ROWS, A2S_WGRAD_ROWS: decimal bit masks; A2S_GRU_PERSIST,
 * A2S_DEC_PERSIST, A2S_DEC_FUSED: off when the text starts with 0) once, when it is loaded.  0, or A2S_ERR_ARG with the variable it could not
 * parse in a2s_last_error() (that switch keeps its default). */
int a2s_env_check(void);
/* Persistent kernels (encoder recurrences, few-clip note decoder: one launch whose workgroups wait for each other, replacing the per-step
 * launches of nn.GRU / NoteDecoder.decode_notes, models.py:63-67,388-419).  Their waits are bounded; a launch that gives up poisons its outputs
 * with NaN (the loss becomes non-finite, the update is skipped) and ORs a bit into *device_word (a 4-byte device word the caller owns, zeroed by
 * the caller; NULL unregisters).  The host reads the word at a synchronisation point it has anyway and switches the persistent paths off
 * (a2s_debug_set("gru_persist" / "dec_persist", 0)) for the rest of the process.  The paths are only taken when the runtime reports a chip
 * they fit (compute units x workgroups per CU >= the launch; 8 XCDs x 32 CUs for the decoder).
 * Test hooks: a2s_debug_set("persist_force_agent", 1) = never use the one-XCD plain-store hand-off, "persist_inject_abort", 1 = every
 * persistent launch behaves as if a wait had timed out. */
int a2s_persist_abort_latch(void* device_word);

/* ---- ConvStack (models.py:475-502,:523-534).  Activations are (B, T, C, F); see csrc/a2s_conv.hip (weight gradients: a2s_conv_wgrad.hip, BatchNorm: a2s_bn.hip).
 * conv3x3: y = conv(relu(x*in_scale+in_shift)) (scale/shift NULL: plain x), zero padding 1, no bias;
 * stat_partial [blocks][Cout][2] receives per-block sum / sum-of-squares of y (NULL to skip);
 * flip=1 runs the data-gradient form with w read as w'[ci][co][2-dt][2-df]. */
int a2s_conv3x3(void* stream, const float* x, const float* w, float* y, const float* in_scale, const float* in_shift,
                float* stat_partial, int B, int T, int F, int Cin, int Cout, int flip, float* workspace);
/* The same forward convolution with operand RANGES (round 3; replaces nothing new in the reference: models.py:525-534 as a2s_conv3x3):
 * in_absmax[Cin] = max |x| per input channel (as written into `out_absmax` by the launch that produced x; NULL: measured here by an
 * extra pass), out_absmax[Cout] = max |y| per output channel, written by this launch (NULL: not wanted).  The row-streaming kernel
 * (csrc/a2s_conv_rows.hip) derives exact power-of-two operand scales from them, so that its fp16 operand terms never overflow or lose
 * precision whatever BatchNorm's scale is; the tiled two-term kernel (F % 4 != 0, "conv_rows" 0) scales the activated operand by the power
 * of two of its bound max_c(|in_scale_c| in_absmax_c + |in_shift_c|). */
int a2s_conv3x3_ranged(void* stream, const float* x, const float* w, float* y, const float* in_scale, const float* in_shift, const float* in_absmax,
                       float* stat_partial, float* out_absmax, int B, int T, int F, int Cin, int Cout, float* workspace);
int a2s_conv3x3_stat_blocks(int B, int T, int F, int Cin);
/* Data gradient of a convolution (flip form: g = dy (*) w') whose output is the gradient wrt relu(bn(yl)) of the layer below, with that
 * layer's BatchNorm-backward statistics (sum g', sum g' xhat; g' = g where bn(yl) > 0) accumulated in the epilogue into stat_partial
 * [a2s_conv3x3_stat_blocks(B,T,F,Cin)][Cout][2] -- pass it to a2s_bn_bwd_from_partial instead of running the statistics pass of
 * a2s_bn_bwd.  Cin / Cout are those of THIS launch (Cin = channels of dy, Cout = channels of g and yl). */
int a2s_conv3x3_dgrad_bnstats(void* stream, const float* dy, const float* w, float* g, const float* yl, const float* yl_mean, const float* yl_invstd,
                              const float* yl_scale, const float* yl_shift, float* stat_partial, int B, int T, int F, int Cin, int Cout,
                              float* workspace);
int a2s_bn_bwd_from_partial(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale, const float* shift,
                            float* dgamma, float* dbeta, float* dx /* may be NULL */, const float* partial, int nblocks, float* c12, long rows, int C, int F);
/* The same two calls for the TWO-TERM fp16 convolution path (csrc/a2s_conv.hip conv3x3_split<.., 2>: every fp32 operand as two fp16
 * terms, three products instead of the six of the three-term bf16 split).  fp16 has no exponent range to spare for gradients, so the
 * kernel that WRITES a gradient tensor also reduces max |dx| into a device scalar (dx_absmax, 1 float) and the data-gradient convolution
 * that READS it scales its operand by the exact power of two that brings that maximum to 2^12 (dy_absmax; NULL = three-term path). */
int a2s_conv3x3_dgrad_bnstats_scaled(void* stream, const float* dy, const float* w, float* g, const float* yl, const float* yl_mean, const float* yl_invstd,
                                     const float* yl_scale, const float* yl_shift, float* stat_partial, int B, int T, int F, int Cin, int Cout,
                                     float* workspace, const float* dy_absmax);
/* Round 4: the same, also writing the range of the gradient it writes into g_absmax_out[Cout] (the launch zeroes it): the MAXIMUM over the Cout
 * entries is max |g| exactly, every entry is >= 0 and none exceeds that maximum -- nothing more (the first-generation row-streaming kernels keep
 * one running maximum per lane whatever the channel, so an entry is NOT the maximum of its channel; conv3x3_rows16, one channel per lane, and the
 * tiled kernels, which run a per-channel pass, happen to write max |g_c|).  The consumer, a2s_conv3x3_wgrad_bn_ranged (g_absmax, g_absmax_n = Cout), takes the
 * maximum over the entries to bound the BatchNorm backward of the layer below. */
int a2s_conv3x3_dgrad_bnstats_ranged(void* stream, const float* dy, const float* w, float* g, const float* yl, const float* yl_mean, const float* yl_invstd,
                                     const float* yl_scale, const float* yl_shift, float* stat_partial, int B, int T, int F, int Cin, int Cout,
                                     float* workspace, const float* dy_absmax, float* g_absmax_out);
int a2s_bn_bwd_from_partial_amax(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale, const float* shift,
                                 float* dgamma, float* dbeta, float* dx, const float* partial, int nblocks, float* c12, long rows, int C, int F,
                                 float* dx_absmax);
size_t a2s_conv3x3_workspace_floats(int Cin);   /* scratch for the packed weight image (0 for Cin = 1) */
/* BatchNorm2d/1d statistics -> affine (models.py:499-505): reduces the partials in fixed order (double),
 * updates running stats (momentum, unbiased var) and num_batches_tracked when training, emits mean/invstd
 * (for backward) and scale/shift with y = x*scale+shift.  training=0: uses the running statistics. */
int a2s_bn_finalize(void* stream, const float* partial, int nblocks, int C, double count, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                    float* mean, float* invstd, float* scale, float* shift, float eps, float momentum, int training);
int a2s_bn_relu_apply(void* stream, const float* x, float* y, const float* scale, const float* shift, long n, int C, int F);
int a2s_col_stats(void* stream, const float* x, float* partial, long rows, int C, int rows_per_block);
/* Column sums and sums of squares of x (rows, C) accumulated in double and written as two fp32 terms: partial[2 * nblocks][C][2] with
 * nblocks = ceil(rows / rows_per_block) -- entries [0, nblocks) the fp32 heads, [nblocks, 2 nblocks) the remainders.  a2s_bn_finalize over
 * 2 * nblocks entries then has the sums to ~48 bits: the variance of a few nearly equal rows is not lost in 2^-24 mean^2. */
/* z (M, N) = relu(x * scale[k / period] + shift[k / period]) W^T for contiguous x (M, K) and W (N, K), products and sums in double (K % period == 0):
 * the ConvStack's Linear in a training call of few rows, whose BatchNorm1d returns an error of z up to 1 / sqrt(eps) = 316-fold. */
int a2s_linear_fwd_f64(void* stream, int M, int N, int K, const float* x, const float* W, float* z, const float* scale, const float* shift, int period);
int a2s_col_stats_split(void* stream, const float* x, float* partial, long rows, int C, int rows_per_block);
int a2s_bn1d_relu_dropout(void* stream, const float* x, float* y, const float* scale, const float* shift,
                          const uint8_t* keep_mask, float inv_keep, long n, int C);

/* ---- GRU (nn.GRU, gate packing [r;z;n]; models.py:63-67,:107-111,:117-120,:353-356) */
int a2s_gru_gates_fwd(void* stream, const float* gi, long ldgi, const float* gh, long ldgh, const float* hprev, long ldhp,
                      float* hout, long ldho, float* hout2, long ldho2, float* save, int R, int H);
/* one direction of one encoder layer over T steps, h0 = 0 (Encoder.forward, models.py:77) */
int a2s_gru_seq_fwd(void* stream, const float* gi_all, long gi_bstride, long gi_tstride, const float* w_hh,
                    const float* b_hh, float* out, long out_bstride, long out_tstride, float* hbuf, float* gh,
                    float* save, float* hn, int B, int T, int H, int reverse, float* workspace, size_t workspace_bytes);
/* workspace (optional): split-K scratch for the per-step recurrent GEMM (M = B rows, few output tiles) */

/* ---- additive attention step (AttentionLayer.forward models.py:452-461 + bmm :242,:394), keys hoisted:
 * score_t = v . tanh(K[b,t,:] + q[b,:]); a = softmax_t; ctx = sum_t a_t enc[b,t,:].
 * `keys` of every attention entry point is the KEY IMAGE exp(2 K) (a2s_gemm_f32 with act 3 on K = enc W_e^T; |K| clamped to 43), not K:
 * tanh(k + q) = 1 - 2 / (1 + exp(2k) exp(2q)) then costs one transcendental per (frame, unit).  q is passed as is; the gradient
 * a2s_attn_dk_accum returns is the one with respect to K.
 * DOMAIN.  The image clamps k to +-43 and every kernel clamps q to +-43, each without looking at the other, so the energies are those of
 * tanh(k + q) -- to within 3.05e-8 = 1 - tanh(9) -- only on
 *     D = (|k| <= 43 and |q| <= 43)  or  min(|k|, |q|) <= 34.
 * Outside D the result is finite, looks like any other and is wrong by up to 1.0 (k = 50, q = -45 gives 0 where tanh(5) = 0.9999); the
 * gradients likewise.  No entry point checks this: a caller whose attention Linear is unconstrained (a trained checkpoint) must.  The host
 * side does, for every pass that decodes in eval mode: piano_a2s_amd/attn_range.py reads max |k| back from the image (0.5 max |ln image|,
 * which saturates at 43: "43 or more"), bounds |q| by max_j (sum |W_h[j, :]| + |b_j|) (the states are GRU states in (-1, 1)) and raises
 * A2SError outside D.  Inside D an image entry is within 2^-23 + |k| 2^-22 relative of exp(2k). */
int a2s_attn_step_fwd(void* stream, const float* keys, const float* enc, const float* q, long ldq, const float* v,
                      float* ctx, long ldctx, float* ctx2, long ldctx2, float* attw, int B, int T, int H,
                      const int* n_done, int n_rows_total, float* workspace);
/* the same step over the R = groups * n_clips rows of a fused-bars decoder call (row = group * n_clips + clip; see a2s_note_dec_args):
 * rows of a clip share its keys / enc; clip_order / clip_rank / row_until may be NULL (identity, never finished), n_active = clips
 * computed (prefix of clip_order), step = decode step compared with row_until.  Skipped rows get ctx = 0, attw = 0. */
int a2s_attn_step_fwd_rows(void* stream, const float* keys, const float* enc, const float* q, long ldq, const float* v, float* ctx,
                           long ldctx, float* ctx2, long ldctx2, float* attw, int R, int T, int H, float* workspace, int n_clips,
                           const int* clip_order, const int* clip_rank, const int* row_until, int n_active, int step);
/* workspace (a2s_attn_workspace_floats floats, shared by forward and backward) selects the split-T kernels: the frames of a
 * clip are spread over several workgroups and merged by a combine kernel -- or, with a2s_debug_set("attn_fused_combine", 1), by the
 * workgroup that finishes last for the clip (measured slower on MI355X, off by default); NULL (or hidden_size != 256) = one workgroup
 * per clip.  The workspace must be ZERO-INITIALISED ONCE after allocation (its head holds the workgroups' arrival counters, which
 * every launch leaves at zero) and must not be shared by launches that may run concurrently. */
size_t a2s_attn_workspace_floats(int B, int T, int H);
/* the same for a fused-bars decoder call (a2s_note_dec_args.n_clips): `groups` bars of n_clips clips in one call */
size_t a2s_attn_workspace_floats_fused(int n_clips, int T, int H, int groups);

/* y[r, :V] = log_softmax(x[r, :V]) over R rows with row strides ldx / ldy; argmax_out (R ints, may be NULL) = the lowest index among the
 * row's maxima.  The index written is always in [0, V): a row without an ordered value (all NaN, all -inf) gives 0 -- its
 * log-probabilities are NaN all the same. */
int a2s_log_softmax_rows(void* stream, const float* x, long ldx, float* y, long ldy, int* argmax_out, int R, int V);
int a2s_embed_rows(void* stream, const float* table, const long long* ids64, const int* ids32, long id_stride,
                   int const_id, float* out, long ldo, int col0, int R, int E, const uint8_t* keep_mask, float inv_keep);

/* ---- one (bar, staff) note decode: NoteDecoder.decode_notes, models.py:366-420 */
typedef struct a2s_note_dec_args {
    const float* attn_w; const float* attn_b; const float* attn_v;
    const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh;
    const float* out_w; const float* out_b; const float* emb;
    const float* keys; const float* enc;
    float* h; float* x; float* q; float* gates; float* attw; float* o;
    float* gh; float* gi; float* logits;
    float* probs; long probs_bstride;
    const long long* gt; long gt_bstride;
    const uint8_t* tf_flags;          /* HOST array, one entry per step: bit g = teacher-force the rows of group g (bit 0 when not fused) */
    const uint8_t* drop; float inv_keep;
    int* argmax_out; long am_bstride;
    int* eos_seen; long long* lengths; int* n_done;
    int* steps_exec;                  /* device counter: +1 per step that actually decoded (greedy early break) */
    float* attn_ws;                   /* a2s_attn_workspace_floats(R,T,H) [_fused(n_clips,T,H,R/n_clips)] floats or NULL */
    float* gemm_ws; size_t gemm_ws_bytes;   /* split-K scratch for the per-step skinny GEMMs (NULL: no split-K) */
    int* t_base;                      /* device int (graph mode): base step index of the chunk being replayed */
    /* optional, training only (the fused training step, not the drop-in module):
       (1) fused bars -- the R rows are R/n_clips bars ("groups", <= 5) of the same n_clips clips, row = group * n_clips + clip; the
           bars' decoders are independent once the bar-level recurrence is teacher-forced, and rows of one clip share its keys and
           encoder outputs, which the attention kernels then stream once for all of them;
       (2) finished rows -- from step row_until[row] on a row's remaining targets are all <pad>: nothing reaching the loss depends
           on it any more, its attention is skipped (context = 0) and its outputs are left untouched.
       Clips sorted by the step their last row finishes at, latest first, so the clips still running are a prefix: */
    const int* clip_order;            /* device, n_clips ints: clip ids in that order */
    const int* clip_rank;             /* device, n_clips ints: inverse permutation */
    const int* row_until;             /* device, R ints */
    const int* n_active;              /* HOST, `steps` ints: clips with an unfinished row at step t; NULL = none of (1)/(2) */
    int n_clips;                      /* 0 = R (one group) */
    const int* m_active;              /* HOST, `steps` ints or NULL: 1 + the largest clip index (position in the call, not in clip_order)
                                         that still has an unfinished row at step t.  When that is at most half of n_clips the per-step
                                         products run on the leading m_active[t] clips of every fused bar only (round 3: the few
                                         full-length rows of a large call no longer drag every row through ~100 further steps) */
    const int* row_list;              /* device, R ints or NULL: the rows sorted by row_until, latest first (stable) -- the rows still running
                                         at step t are its first n_rows_active[t] entries; the few-row step kernels then cover those only */
    const int* n_rows_active;         /* HOST, `steps` ints (with row_list) */
    int R, T, H, E, V, steps, poll, eos_id;
    int use_graph;                    /* greedy decode (gt NULL, nothing saved for backward): capture `poll` steps into a hipGraph and replay */
    float* step_ws; size_t step_ws_floats;   /* a2s_note_step_workspace_floats(H, E) floats or NULL: scratch of the fused few-row step kernels
                                                (csrc/a2s_step.hip: 4 launches per step instead of 9-13; used when R <= "dec_fused_max_rows", default 192; above that the launch-per-step loop with the mid-size kernels dec_gru_mid / dec_outq_mid / dec_bwd_mid) */
    /* round 4: ONE persistent launch for every step of the call when it covers at most 8 clips (csrc/a2s_dec_persist.hip: one clip per XCD,
       keys / encoder outputs resident in LDS, weights in registers).  Needs the teacher-forcing flags on the device too and a scratch area: */
    const int* tf_flags_dev;          /* device, `steps` ints: the same bits as tf_flags (NULL with tf_flags NULL) */
    float* persist_ws; size_t persist_ws_bytes;   /* a2s_note_decoder_persist_ws_bytes(n_clips, R, steps) bytes, 256-byte aligned, or NULL */
} a2s_note_dec_args;
/* The id a step chooses -- written to argmax_out, compared with eos_id, and the row of `emb` the next step's input is gathered from when the
 * step is not teacher-forced -- is always in [0, V), on every path (launch per step, few-row, persistent): a row of logits without an ordered
 * value (all NaN, all -inf) chooses 0.  Its log-probabilities stay NaN, so the loss stays non-finite and the update is skipped. */
int a2s_note_decoder_fwd(void* stream, const a2s_note_dec_args* args, int* steps_done);
/* ---- grammar-constrained greedy decoding (csrc/a2s_grammar.hip).  A token grammar is a finite automaton given as a
 * device table next_state[s * V + v] (n_states x V signed bytes, 1 <= n_states <= 127, V <= 256): the state after token v in state s, negative
 * where v is illegal in s; every row carries one state in row_state (device ints, updated in place).  A row emits the legal token with the
 * largest logit (lowest index on ties) and moves to its next state; the log-probabilities written stay the UNCONSTRAINED log_softmax.
 * a2s_grammar_argmax_rows: the constrained sibling of a2s_log_softmax_rows for R rows of V logits (y may be NULL; choice_out: R ints).
 * a2s_note_decoder_fwd_grammar: a2s_note_decoder_fwd for greedy calls (args->gt, the training buffers and the row bookkeeping must be NULL:
 * A2S_ERR_ARG otherwise), always on the launch-per-step loop (mid-size kernels at H = 256, library-style products otherwise; args->use_graph
 * replays it as a graph) with the grammar kernel as the step epilogue -- never the persistent or the few-row decoders, whose epilogues hold
 * their own argmax.  args->argmax_out receives the EMITTED ids; <eos> bookkeeping as a2s_note_decoder_fwd (a table that allows only <pad>
 * behind <eos> makes a row's length final at its first <eos>).  a2s_grammar_launches: step epilogues launched so far (proof of the path). */
int a2s_grammar_argmax_rows(void* stream, const float* x, long ldx, float* y, long ldy, const signed char* next_state, int n_states, int* row_state,
                            int* choice_out, int R, int V);
int a2s_note_decoder_fwd_grammar(void* stream, const a2s_note_dec_args* args, const signed char* next_state, int n_states, int* row_state, int* steps_done);
int a2s_grammar_launches(void);
/* ---- metre-aware constrained decoding (csrc/a2s_grammar.hip): the grammar above plus the metre of the bar.  A token the
 * table allows must also pass the row's metre: a note starts in a spine only where its previous note ends, a `.` stands only where one still
 * sounds, a duration neither overfills the bar nor leaves a remainder no sum of duration symbols fills, chord members share one duration, later
 * lines have the first line's field count, a line break needs the earliest spine end m below the bar length L and <eos> needs m == L (the empty
 * bar stays legal).  row_metre holds A2S_METRE_INTS ints per row, read and updated in place:
 *     [0] L: bar length in ticks of 1/147840 whole note; L <= 0: the row is unmetred and obeys the table alone (its ints are never written)
 *     [1] t: onset of the current line   [2] first_line (1 / 0)   [3] n_fields (fixed by the first line break)   [4] field: current spine, 0 .. 7
 *     [5] in_chord (1 behind a chord separator, until the field ends)   [6] field_dur: ticks of the field's first note   [7] reserved, 0
 *     [8 .. 15] end[0 .. 7]: where each spine's last note ends
 * A fresh row is {L, 0, 1, 0, 0, 0, 0, 0, 0 x 8}.  The metre reference (the library's a2s_metre_ref; like the grammar's table it is passed member by
 * member, all device memory): dur_ticks: V ints, ticks of a duration symbol; cls: V bytes of A2S_METRE_CLS_* (0: a class the metre does not look
 * at); fillable: n_fillable bytes (max L + 1), fillable[r] != 0 where r ticks are a sum of duration symbols (an index outside the table reads as
 * not fillable); row_metre: R x A2S_METRE_INTS ints.  Values read from row_metre are clamped before they index anything.
 * a2s_metre_argmax_rows / a2s_note_decoder_fwd_metre: a2s_grammar_argmax_rows / a2s_note_decoder_fwd_grammar with that predicate -- the same
 * argument rules, the same loop (launch per step, or replayed as a graph), the same log-probabilities; a NULL member of the metre reference or
 * n_fillable < 1: A2S_ERR_ARG, nothing is launched.  With every L <= 0 they compute what the grammar entry points compute, bit for bit.
 * a2s_metre_launches: metre step epilogues launched so far (proof of the path). */
#define A2S_METRE_INTS 16
#define A2S_METRE_FIELDS 8
#define A2S_METRE_L 0
#define A2S_METRE_T 1
#define A2S_METRE_FIRST 2
#define A2S_METRE_NFIELDS 3
#define A2S_METRE_FIELD 4
#define A2S_METRE_CHORD 5
#define A2S_METRE_FDUR 6
#define A2S_METRE_END 8
#define A2S_METRE_CLS_DUR 1
#define A2S_METRE_CLS_NULL 2
#define A2S_METRE_CLS_OPEN 3
#define A2S_METRE_CLS_TAB 4
#define A2S_METRE_CLS_NL 5
#define A2S_METRE_CLS_SP 6
#define A2S_METRE_CLS_EOS 7
int a2s_metre_argmax_rows(void* stream, const float* x, long ldx, float* y, long ldy, const signed char* next_state, int n_states, int* row_state,
                          const int* dur_ticks, const uint8_t* cls, const uint8_t* fillable, int n_fillable, int* row_metre, int* choice_out, int R, int V);
int a2s_note_decoder_fwd_metre(void* stream, const a2s_note_dec_args* args, const signed char* next_state, int n_states, int* row_state,
                               const int* dur_ticks, const uint8_t* cls, const uint8_t* fillable, int n_fillable, int* row_metre, int* steps_done);
int a2s_metre_launches(void);
/* ---- beam-search decoding of one (bar, staff) call (csrc/a2s_beam.hip).  The call runs over B clips with K beam slots
 * each, 1 <= K <= A2S_BEAM_MAX: args->R = K * B, args->n_clips = B, row = slot * B + clip (the fused-bars layout, so the attention kernels read a
 * clip's key image and encoder rows once for its K rows); every row of args->h / args->x starts from the same state and the <sos> embedding.
 * Nothing is kept per step: args->h, args->x, args->q and args->o hold TWO slots of K * B rows each (step parity).
 * A candidate (slot k, token v) scores score[k] + log_softmax(logits_k)[v] (one fp32 add), -inf where next_state forbids v in the slot's state; a
 * finished slot has the one candidate (k, <pad>) at its score; the new beam is the K best candidates of the clip, ties to the lowest k * V + v,
 * best first.  Behind the loop each clip keeps the slot with the largest score / len^alpha (alpha = 0: the raw score; ties to the lowest slot).
 * a2s_note_decoder_fwd_beam: greedy calls only (args->gt, the training buffers and the row bookkeeping must be NULL; K outside 1 .. 4 or
 * R != K * n_clips: A2S_ERR_ARG), always the launch-per-step loop (mid-size kernels at H = 256, library-style products otherwise; never the
 * persistent or the few-row decoders; args->use_graph is ignored) with beam_step_finalize as the step epilogue, then one beam_backtrack launch.
 * It initialises score / finished / done_count / args->n_done itself; row_state holds the start state of every row.  args->probs receives, at
 * step t, the UNCONSTRAINED log-probabilities computed at step t in the slot the winning hypothesis then occupied; args->argmax_out,
 * args->lengths and args->eos_seen are not used.  a2s_beam_launches: step epilogues launched so far (proof of the path). */
#define A2S_BEAM_MAX 4
typedef struct a2s_beam_args {
    int K; float alpha;                      /* beam slots per clip; length penalty of the final pick */
    const signed char* next_state; int n_states;   /* the grammar's table as in a2s_note_decoder_fwd_grammar; NULL / 0: none */
    int pad_id;                              /* what a finished slot emits, and the ids behind the executed steps */
    int* row_state;                          /* device, K * B ints (read and written also without a grammar) */
    float* score; int* finished;             /* device, K * B each */
    int* done_count;                         /* device, max_steps + 1 ints: finished slots BEFORE step t (a step is a no-op at K * B) */
    int* token_hist; int* parent_hist; float* score_hist;      /* device, (max_steps, K * B) each: per step the new slots' token, parent slot, score */
    float* probs_scratch;                    /* device, (K * B, max_steps, V), zero-filled: every row's log-probabilities per step */
    int* ids_out; long long* lengths_out; float* score_out;    /* device: (B, max_steps) ids, (B) lengths, (B) raw scores of the winners */
} a2s_beam_args;
int a2s_note_decoder_fwd_beam(void* stream, const a2s_note_dec_args* args, const a2s_beam_args* beam, int* steps_done);
/* one step epilogue on its own (tests): logits (K * B, ldl), step t of max_steps; emb (V, E) -> xnext (K * B, ldx); h (K * B, h_cols) and, if not
 * NULL, q (K * B, q_cols) are re-parented in place; n_done / steps_exec: device ints.  a2s_beam_backtrack: the pick and the walk back, probs row
 * b at probs + b * probs_bstride (max_steps x V); steps_exec: device int, the steps that ran. */
int a2s_beam_step(void* stream, const a2s_beam_args* beam, const float* logits, long ldl, const float* emb, float* xnext, long ldx, float* h, int h_cols,
                  float* q, int q_cols, int* n_done, int* steps_exec, int B, int V, int E, int t, int max_steps, int eos_id);
int a2s_beam_backtrack(void* stream, const a2s_beam_args* beam, float* probs, long probs_bstride, const int* steps_exec, int B, int V, int max_steps, int eos_id);
int a2s_beam_launches(void);
/* ---- audio alignment from the attention weights (csrc/a2s_align.hip).  Frame t of the encoder outputs is t * hop_length /
 * sample_rate seconds of audio, and every bar step and note step forms softmax weights over the T frames.  a2s_attn_align_rows reduces R rows of
 * such weights (attw, row stride ldw >= T floats: what the attention entry points write through `attw`) to peak = the lowest frame index among the
 * row's maxima (int32), weight = attw[peak] bit for bit, and centroid = sum_t t * attw[t] in fp32 (not renormalised); row r's results go to
 * peak_out / weight_out / centroid_out[r * out_stride], so that a decode step writes one column of an (R, max_steps) array.  A row of zeros (its
 * attention was skipped) gives (0, 0, 0).  One wave per row.  Null pointers, R < 0, T < 1, ldw < T or out_stride < 1: A2S_ERR_ARG, nothing is
 * launched; R = 0 returns 0 and launches nothing.  a2s_align_launches: launches so far (proof of the path).
 * a2s_note_decoder_fwd_align: a2s_note_decoder_fwd that also records, per step t and row, where the row attended to.  It takes GREEDY calls
 * (args->gt NULL; with align->next_state the constrained decoder of a2s_note_decoder_fwd_grammar) and TEACHER-FORCED calls (args->gt and
 * args->tf_flags given, args->poll 0; a grammar is then an argument error) -- the forced alignment of a known score; neither may carry the training
 * buffers (gates, attw, drop) or the row bookkeeping (n_active, row_list, m_active, clip_order, row_until): A2S_ERR_ARG otherwise, nothing is
 * launched.  Always the launch-per-step loop (mid-size kernels at H = 256, library-style products otherwise; never the persistent or the few-row
 * decoders; args->use_graph is ignored): every step's attention writes its weights to align->attw_step, a2s_attn_align_rows follows on the same
 * stream and writes column t.  Everything else of a step, and so every output of a2s_note_decoder_fwd, is unchanged.  Columns of steps the call
 * never runs are left untouched: the caller pre-fills peak -1, weight 0, centroid -1. */
typedef struct a2s_align_args {
    float* attw_step;                        /* device, (R, T) floats: the weights of ONE step, the same slot every step */
    int* peak; float* weight; float* centroid;     /* device, (R, max_steps) each: row r, step t at r * out_stride + t */
    long out_stride;                         /* >= args->steps */
    const signed char* next_state; int n_states;   /* the grammar's table as in a2s_note_decoder_fwd_grammar; NULL / 0: none */
    int* row_state;                          /* device, R ints (with a grammar) */
} a2s_align_args;
int a2s_attn_align_rows(void* stream, const float* attw, long ldw, int R, int T, int* peak_out, float* weight_out, float* centroid_out, long out_stride);
int a2s_note_decoder_fwd_align(void* stream, const a2s_note_dec_args* args, const a2s_align_args* align, int* steps_done);
int a2s_align_launches(void);

/* ---- note synthesiser of the rendered synthetic corpus (csrc/a2s_render.hip).  a2s_render_notes writes the 16 kHz waveforms of B
 * clips from their render programs: `programs` = device, B * rows_per_clip rows of 8 int32 (floats bit-cast), 16-byte aligned; per clip
 *     row 0      [n_samples, n_rows, attack, rel_len, rel_rate f32, gain f32, noise_level f32, noise_seed u32]
 *     rows 1 ..  [onset >= 0, length, inc1 u32 = rint(f0 / 16000 * 2^32), amp f32, decay f32 per sample, g f32, n_harm 1 .. 16, 0]
 * (rows behind min(n_rows, rows_per_clip - 1), and rows with length <= 0, onset >= n_samples or onset < 0, are padding and skipped whatever else they
 * hold).  Sample n of clip b goes to wave[b * wave_bstride + n], n in [0, n_samples):
 *     gain * sum_rows(ascending) amp * env(m) * sum_{h = 1 .. n_harm, h * inc1 < 2^31} g^(h-1) * sin(2 pi x_h(m))  +  noise_level * u(n)
 *     m = n - onset in [0, length + rel_len),  x_h(m) = ((uint32)(m * h * inc1) >> 8) * 2^-24,
 *     env(m) = min(1, (m + 1) / attack) * exp(-m * decay) * (m >= length ? exp(-(m - length) * rel_rate) : 1),
 *     u(n) = (hash32(noise_seed + n * 0x9E3779B9) >> 8) * 2^-23 - 1;  hash32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 * `n_samples` is the caller's (the library reads no device memory back and does not synchronise): the same for every clip of the call; a clip whose
 * header says less gets zeros behind its own length.  One thread forms a sample's whole sum in a fixed order: the output is bit-identical from run to
 * run and does not depend on the other clips.  Nothing outside [0, n_samples) of a clip's row of `wave` is written.  Null pointers, B < 0 or > 65535,
 * rows_per_clip < 1, n_samples < 1, wave_bstride < n_samples, misaligned programs: A2S_ERR_ARG, nothing is launched; B = 0 returns 0 and launches
 * nothing.  One launch per call; a2s_render_launches: launches so far (proof of the path). */
int a2s_render_notes(void* stream, const int* programs, int rows_per_clip, int n_samples, float* wave, long wave_bstride, int B);
int a2s_render_launches(void);

/* ---- transposition augmentation of a training batch (csrc/a2s_augment.hip).  Both entry points take borrowed device pointers
 * and a stream; they allocate nothing, do not synchronise and read nothing back.
 * a2s_transpose_targets respells the targets of B clips in place, one workgroup per clip.  Tables (device, int32, piano_a2s_amd/kern_transpose.py):
 * new_key (13, 14): [s + 6][key class] -> key class; interval (13, 14): [s + 6][key class] -> row of token_map; token_map (n_rows, V): token id ->
 * token id, or -1 where the transposed pitch has no symbol.  Per clip b: semitones[b] = s in -6 .. 6 (int32) and detune[b] (float32, in bins); key
 * (B, bars), upper (B, bars, U), lower (B, bars, L): int64, contiguous.  A bar's row is interval[s + 6][key[b][bar]]: the bars of a clip share s and may
 * differ in their key.  A clip is NOT REPRESENTABLE when any of its tokens maps to -1, or s, a key, a row or a token id is out of range; such a clip
 * keeps its tokens and keys.  Otherwise every token and key of the clip is rewritten through the tables.  In both cases
 *     eff_bins[b] = float(bins_per_semitone * s) + detune[b]  (representable: one fp32 add)   |   detune[b]  (not representable),
 * and counters[0 .. 2] (device int32; global atomic adds) grow by: clips seen, clips transposed (s != 0 and representable), clips kept because not
 * representable.  Null pointers, B < 0, n_rows < 1, V < 1, bars < 1, U < 1, L < 1, bins_per_semitone < 1: A2S_ERR_ARG, nothing is launched; B = 0
 * returns 0 and launches nothing.
 * a2s_shift_bins shifts the feature rows, out of place: x, y = (B, rows, F) float32, contiguous, x != y; with n = eff_bins[b] (read on the device),
 * m = floor(n), a = n - m:
 *     y[b][t][j] = (1 - a) * x[b][t][j - m] + a * x[b][t][j - m - 1],   x taken as 0 outside [0, F).
 * a == 0 writes x[b][t][j - m] itself (bit for bit; n == 0: a copy); |n| >= F + 1 or n not finite writes zeros.  Nothing outside the B * rows * F
 * floats of y is written and nothing outside those of x is read.  16-byte stores when F % 4 == 0 and y is 16-byte aligned, 4-byte stores otherwise.
 * Null pointers, x == y, B < 0 or > 65535, rows < 1, F < 1, rows * F >= 2^31: A2S_ERR_ARG, nothing is launched; B = 0 returns 0 and launches nothing.
 * One launch per call each; a2s_augment_launches: launches of the two so far (proof of the path). */
int a2s_transpose_targets(void* stream, const int* new_key, const int* interval, const int* token_map, int n_rows, int V, const int* semitones,
                          const float* detune, long long* key, long long* upper, long long* lower, int bars, int U, int L, int bins_per_semitone,
                          float* eff_bins, int* counters, int B);
int a2s_shift_bins(void* stream, const float* x, float* y, const float* eff_bins, int B, int rows, int F);
int a2s_augment_launches(void);

/* ---- tempo augmentation of a training batch (csrc/a2s_tempo.hip): every clip's feature rows are resampled along time, the
 * targets stay.  Both entry points take borrowed device pointers and a stream; they allocate nothing, do not synchronise and read nothing back.
 * Positions are integers in Q16: step[b] = rint(65536 / c) is the source advance per output row of clip b, c the factor on durations (c > 1: slower).
 * a2s_tempo_plan, one workgroup per clip of x (B, rows, F) float32, contiguous: content[b] = 1 + the last row that holds a value != 0 (a NaN is
 * content, -0.0 is not; 0 for an all-zero clip), found by scanning backwards from the last row in chunks of 16 rows up to the first chunk with content.
 * Then, in fp32 and in this form, with n = content[b] and u[b] in [0, 1) drawn by the host:
 *     lo = max(1 - R, (float)min_frames / n),  hi = min(1 + R, (float)rows / n);
 *     n == 0 or lo > hi: step[b] = 65536 and the clip counts as kept;
 *     otherwise c = fmaf(u[b], hi - lo, lo) and step[b] = clamp((int)rintf(65536.0f / c), 52429, 87381):
 * a stretched clip still holds at least min_frames rows of content and does not run off its rows.  counters[0 .. 2] (device int32; global atomic
 * adds) grow by: clips seen, clips with step != 65536, clips kept for want of a feasible interval.  content, step: (B,) int32.  Null pointers, B < 0
 * or > 65535, rows < 1 or > 16384, F < 1, R outside [0, 0.25] or not finite, min_frames < 1: A2S_ERR_ARG, nothing is launched; B = 0 returns 0 and
 * launches nothing.
 * a2s_stretch_frames resamples the rows, out of place: x, y = (B, rows, F) float32, contiguous, x != y; step (B,) int32 is read on the device.  For
 * output row t: pos = t * step, h = max(65536, step), w_k = h - |k * 65536 - pos| where that is > 0, W = the sum of w_k over all integer k, and
 *     y[b][t][f] = sum_k (w_k / W) * x[b][k][f],   x taken as 0 for k outside [0, rows).
 * step <= 65536 is linear interpolation between rows pos >> 16 and the next (W = 65536, exact weights); step > 65536 widens the tent to the source
 * advance (at most three taps), so that no source row is skipped.  A tap of weight 0 is neither read nor added: step == 65536 writes x bit for bit.
 * step outside [52429, 87381] (c outside 0.75 .. 1.25) writes zeros for that clip.  Nothing outside the B * rows * F floats of y is written and
 * nothing outside those of x is read.  16-byte loads and stores when F % 4 == 0 and y is 16-byte aligned, 4-byte ones otherwise.  Null pointers,
 * x == y, B < 0 or > 65535, rows < 1 or > 16384 (pos stays below 2^31), F < 1: A2S_ERR_ARG, nothing is launched; B = 0 returns 0 and launches
 * nothing.  One launch per call each; a2s_tempo_launches: launches of the two so far (a2s_augment_launches does not count them). */
int a2s_tempo_plan(void* stream, const float* x, int B, int rows, int F, const float* u, float R, int min_frames, int* content, int* step,
                   int* counters);
int a2s_stretch_frames(void* stream, const float* x, float* y, const int* step, int B, int rows, int F);
int a2s_tempo_launches(void);

/* ---- spectrogram augmentation of a training batch (csrc/a2s_specaug.hip): per clip a per-bin gain that respects the front
 * end's floor, an additive noise floor, the front end's re-normalisation, and masks along time and frequency; the targets stay.  Both entry points take
 * borrowed device pointers and a stream; they allocate nothing, do not synchronise and read nothing back.  x (B, rows, F) float32, contiguous, holds
 * dB / 80 + 1 relative to the clip's peak: P(x) = 10^(8 (x - 1)) is a cell's power relative to that peak.  Per clip b:
 *     n = content[b] = 1 + the last row that holds a value != 0 (a2s_tempo_plan's rule: a NaN is content, -0.0 is not, 0 for an all-zero clip);
 *     x_min = min of x over rows < n;  a cell is at the floor iff x - x_min <= 2^-18 (in fp32);  p_min = P(x_min);
 *     y = max(p_min, q + v_k),  q = 0 for a floor cell, else G_k * P(x);  M = max of y over rows < n;
 *     out = clamp(1 + log10(y / M) / 8, 0, 1): the cell that attains M comes out as exactly 1.0;
 *     then exact 0.0 in the rows >= n, in the rows [t0_i, t0_i + w_i) and, in rows < n, in the bins [k0_i, k0_i + wk_i), i < 4.
 * table (B, 2, F) float32: per clip the power gains G_k > 0, then the noise powers v_k >= 0 (relative to the clip's peak).
 * a2s_specaug_plan, one workgroup per clip, which sweeps its clip twice (x_min, then M): content (B,) int32, stats (B, 2) float32 = [x_min, M]
 * ([0, 0] for an all-zero clip), plan (B, 16) int32 = 4 x [t0, w] then 4 x [k0, wk], from draws (B, 16) 32-bit words, four per mask (u0 .. u3),
 * in integer arithmetic with 64-bit products:
 *     wmax_t = min(Wt, n / 5),  w  = (u0 * (wmax_t + 1)) >> 32,  t0 = (u1 * (n - w  + 1)) >> 32;
 *     wmax_f = min(Wf, F / 5),  wk = (u2 * (wmax_f + 1)) >> 32,  k0 = (u3 * (F - wk + 1)) >> 32;     masks i >= m: [0, 0].
 * counters[0 .. 2] (device int32; global atomic adds) grow by: clips seen, clips with a time mask of width > 0, clips with a frequency mask of width
 * > 0.  Null pointers, B < 0 or > 65535, rows < 1, F < 1, Wt < 0, Wf < 0, m < 0 or > 4: A2S_ERR_ARG, nothing is launched; B = 0 returns 0 and launches
 * nothing.
 * a2s_specaug_apply writes out (above) to y, out of place: x != y, same shape; table, content, plan and stats as the plan left them (content[b] is
 * clamped to [0, rows] before it bounds a load).  Nothing outside the B * rows * F floats of y is written and nothing outside those of x is read.
 * 16-byte loads and stores when F % 4 == 0 and y is 16-byte aligned, 4-byte ones otherwise.  A clip's output bits do not depend on B or on its
 * position in the batch.  Null pointers, x == y, B < 0 or > 65535, rows < 1, F < 1: A2S_ERR_ARG, nothing is launched; B = 0 returns 0 and launches
 * nothing.  One launch per call each; a2s_specaug_launches: launches of the two so far (a2s_augment_launches and a2s_tempo_launches do not count them). */
int a2s_specaug_plan(void* stream, const float* x, int B, int rows, int F, const float* table, const unsigned* draws, int Wt, int Wf, int m,
                     int* content, int* plan, float* stats, int* counters);
int a2s_specaug_apply(void* stream, const float* x, float* y, const float* table, const int* content, const int* plan, const float* stats, int B,
                      int rows, int F);
int a2s_specaug_launches(void);

/* ---- room acoustics of the rendered synthetic corpus (csrc/a2s_room.hip): every clip's waveform is convolved with a synthetic
 * impulse response of its own, between the synthesiser and the VQT.  Both entry points take borrowed device pointers and a stream; they allocate
 * nothing, do not synchronise and read nothing back.  `params` = device, (B, 4) int32 per clip, computed by the host in float64:
 *     [pre >= 1 (pre-delay in samples), L (taps), wet (float32 bits), decay per sample (float32 bits)];  the device clamps L to [1, L_max].
 * a2s_room_ir writes ir[b * ir_bstride + k], k in [0, L_max), from `params` and the clips' 32-bit seeds (room_seed: device, B words):
 *     1 at k = 0;  0 at 0 < k < pre and at k >= L;  wet * u(k) * exp(-(k - pre) * decay) at pre <= k < L,
 *     u(k) = (hash32(room_seed[b] + (k + 3) * 0x9E3779B9) >> 8) * 2^-23 - 1  (hash32 as for a2s_render_notes).
 * a2s_fir_rows is the direct-form convolution, out of place, in fp32 products and sums (FMAs, k ascending, one thread per sample's whole sum):
 *     y[b * y_bstride + n] = sum_{k = 0 .. min(L - 1, n)} ir[b * ir_bstride + k] * x[b * x_bstride + n - k],   n in [0, n_samples),
 * L = clamp(params[b * 4 + 1], 1, L_max): the history before sample 0 is zero and never read, ir at and behind L never reaches the result (it may hold
 * anything), a short room costs less.  The output is not rescaled: |y| <= sum|ir| * max|x|.  ir is expected to be finite in [0, L): a tile skips the
 * taps that meet nothing but the zero history.  A sample's bits do not depend on B, on the other clips, on n_samples or on the alignment of x and y
 * (16-byte accesses where a row allows them, 4-byte ones otherwise).  Nothing outside [0, n_samples) of a clip's row of y is written, nothing outside
 * [0, n_samples) of its row of x and [0, L) of its row of ir is read.  a2s_fir_tile_samples: samples per workgroup; a2s_fir_tap_chunk: taps per staged
 * window of x.  Null pointers, B < 0 or > 65535, n_samples < 1, L_max < 1, x_bstride or y_bstride < n_samples, ir_bstride < L_max, x == y: A2S_ERR_ARG,
 * nothing is launched; B = 0 returns 0 and launches nothing.  One launch per call each; a2s_room_launches: launches of the two so far. */
int a2s_room_ir(void* stream, const unsigned* room_seed, const int* params, int B, float* ir, long ir_bstride, int L_max);
int a2s_fir_rows(void* stream, const float* x, long x_bstride, const float* ir, long ir_bstride, const int* params, float* y, long y_bstride, int B,
                 int n_samples, int L_max);
int a2s_fir_tile_samples(void);
int a2s_fir_tap_chunk(void);
int a2s_room_launches(void);

/* ---- sample-rate conversion of recordings (csrc/a2s_resample.hip): a rational polyphase resampler with the mono mix in front of
 * it, between an audio file and the VQT.  Borrowed device pointers and a stream; allocates nothing, does not synchronise, reads nothing back.
 *     y[b * y_bstride + n] = sum_{i = 0 .. K-1} table[p * K + i] * mono_b[m0 + Hh - i],        n in [0, n_out[b]),
 *       q = n * M (64-bit),  p = q mod L,  m0 = q div L,
 *       mono_b[m] = (sum_{c = 0 .. C-1, ascending} x[b * x_bstride + m * C + c]) * (1.0f / C)  for m in [0, n_in[b]),  0 elsewhere,
 *       n_out[b] = ceil(n_in[b] * L / M) (64-bit);   y[b * y_bstride + n] = 0 for n in [n_out[b], n_out_max).
 * x: rows of interleaved frames, C channels (1 .. 8) each; n_in: device, B int32, frames per clip, clamped to [0, n_in_max] on the device; table:
 * device, (L, K) float32, row p = the taps of phase p; 0 <= Hh < K.  The sum is an fp32 FMA chain with i ascending and one thread forms the whole
 * sum of an output: its bits do not depend on B, on the other clips, on n_out_max, on the tiling or on the alignment of x, table and y (16-byte
 * accesses where a row allows them, 4-byte ones otherwise).  Nothing of x at or behind n_in[b] frames reaches a result (it may hold NaN) and nothing
 * outside [0, n_in_max * C) of a clip's row of x is read; nothing outside [0, n_out_max) of a clip's row of y is written.  A workgroup keeps the
 * window of mono its a2s_resample_tile_samples() outputs need in LDS: (tile - 1) * M / L + K + 8 may not exceed 15104 samples.
 * Null pointers, B < 0 or > 65535, C outside 1 .. 8, L or M outside 1 .. 4096, K outside 1 .. 8192, Hh outside 0 .. K - 1, a window beyond the
 * limit above, n_in_max < 0, n_out_max < 1, x_bstride < n_in_max * C, y_bstride < n_out_max, x == y: A2S_ERR_ARG, nothing is launched; B = 0
 * returns 0 and launches nothing.  One launch per call; a2s_resample_launches: launches so far. */
int a2s_resample_rows(void* stream, const float* x, long x_bstride, const int* n_in, int n_in_max, int C, const float* table, int L, int M, int K, int Hh,
                      float* y, long y_bstride, int n_out_max, int B);
int a2s_resample_tile_samples(void);
int a2s_resample_launches(void);

/* ---- beat and downbeat tracking on the model's own features (csrc/a2s_beat.hip): the three device stages between the VQT and
 * the host's decision stages (piano_a2s_amd/beats.py).  Every entry point takes borrowed device pointers and a stream; it allocates nothing, does not
 * synchronise and reads nothing back.  One launch per call each; a2s_beat_launches: launches of the three so far.
 * a2s_onset_strength: x = B clips of `rows` rows of F float32 (dB / 80 + 1), row t of clip b at x + b * x_bstride + t * x_rstride; n_rows (B,) int32,
 * clamped to [0, rows] on the device.  env_full, env_low: row b at + b * env_bstride, `rows` floats each:
 *     env_full[b][t] = sum_{f < F} max(0, x[b][t][f] - x[b][t - lag][f])   for lag <= t < n_rows[b],   0 elsewhere in [0, rows);
 *     env_low[b][t]  = the same sum over f < f_split.
 * Plain fp32 sums, no division: inputs on a grid of 1/8 give exact results.  Nothing at or behind row n_rows[b] is read (it may hold NaN).  A clip's
 * bits depend on (F, lag, f_split, the alignment class below) and its own rows alone, not on B, on its place in the batch or on n_rows.  16-byte
 * loads where F % 4 == 0, x is 16-byte aligned and both strides are multiples of 4, 4-byte loads otherwise; 16-byte stores where env_full and env_low
 * are 16-byte aligned and env_bstride is a multiple of 4.  Every element is loaded once, but for the `lag` rows in front of each run of 64 rows, which
 * the workgroup of that run loads again.  Null pointers, B < 0 or > 65535, rows < 1, F < 1, lag < 1, lag * F above 12288, f_split outside 0 .. F,
 * x_rstride < F, x_bstride < (rows - 1) * x_rstride + F, env_bstride < rows: A2S_ERR_ARG, nothing is launched; B = 0 returns 0 and launches nothing.
 * a2s_tempogram: env = R recordings, recording r at env + r * stride, n (R,) int32 frames each (clamped to [0, stride]); out (R, J, lag_max - lag_min + 1).
 * Block j is centred at frame j * hop_b: its window holds the frames g = j * hop_b - win / 2 + u, u in [0, win);
 *     d[u] = env[g] - (mean of env over the window's frames inside [0, n[r])) for g inside [0, n[r]), 0 outside;
 *     out[r][j][l - lag_min] = sum_{u = 0}^{win - 1 - l} d[u] d[u + l] / sum_u d[u]^2,   0 where the denominator is 0.
 * fp32 FMAs.  Null pointers, R < 0 or > 65535, stride < 1, J < 1, win < 1 or > 8192, hop_b < 1, lag_min < 0, lag_min > lag_max, more than 4096 lags:
 * A2S_ERR_ARG, nothing is launched; R = 0 returns 0 and launches nothing.
 * a2s_beat_dp: ls = R rows of `stride` floats (the envelope over its standard deviation), n (R,) int32 (clamped to [0, stride]), period (R, J) int32,
 * pen = (lag_max - lag_min + 1) rows of 2 * lag_max + 1 floats, pen[tau - lag_min][d] the price of a beat interval of d frames at the period tau.
 * For t = 0 .. n - 1, tau = clamp(period[r][min(t / hop_b, J - 1)], lag_min, lag_max), over the candidates p in [max(0, t - 2 tau), t - ceil(tau / 2)]:
 *     c(p) = S[p] - pen[tau - lag_min][t - p];   S[t] = ls[t] + max(0, max_p c(p));   back[t] = the arg max, the one nearest to t among equals, -1
 *     where no candidate is above 0.
 * One fp32 subtraction and one fp32 addition per value, no multiply: a float32 restatement gives the same bits.  The last beat is the first arg max
 * of S over the last tau(n - 1) frames; beats[r * max_beats + k] receives the beats, ascending, as many as fit, count[r] their true number (0 for
 * n = 0); entries of beats at and behind count[r] are not written.  S, back: R rows of `stride`, written at [0, n).  Null pointers, R < 0 or > 65535,
 * stride < 1, J < 1, hop_b < 1, lag_min < 1, lag_min > lag_max, lag_max > 4096, max_beats < 1: A2S_ERR_ARG, nothing is launched; R = 0 returns 0 and
 * launches nothing. */
int a2s_onset_strength(void* stream, const float* x, long x_bstride, long x_rstride, const int* n_rows, int B, int rows, int F, int lag, int f_split,
                       float* env_full, float* env_low, long env_bstride);
int a2s_tempogram(void* stream, const float* env, long stride, const int* n, int R, int J, int win, int hop_b, int lag_min, int lag_max, float* out);
int a2s_beat_dp(void* stream, const float* ls, long stride, const int* period, int J, int hop_b, const float* pen, int lag_min, int lag_max, const int* n,
                int R, float* S, int* back, int* beats, int max_beats, int* count);
int a2s_beat_launches(void);
/* ---- agreement of two feature tensors, segment by segment (csrc/a2s_agree.hip): what the resynthesis of a decoded score is
 * compared with the recording by (piano_a2s_amd/resynth.py).  x, y: device, B clips of T rows of F float32 each, rows contiguous, clip b at
 * + b * clip_stride (the same layout for both); seg: device, S x 4 int32 = [clip, f0, f1, 0]; out: device, S x 5 doubles.  Over the cells
 * x[clip][f0:f1][0:F] of segment s and the same cells of y,
 *     out[s] = [sum x, sum y, sum x^2, sum y^2, sum x y].
 * A clip outside [0, B) gives five zeros; f0 and f1 are clamped to [0, T] and an empty range gives five zeros.  Segments may overlap, repeat and come
 * in any order.  Nothing outside a clip's T * F cells is read (the stride padding may hold NaN) and nothing outside out[0 : 5 S] is written.
 * Summation: the segment's run of n = (f1 - f0) * F cells is cut into chunks of 8192 cells; inside a chunk each of 256 lanes keeps fp32 partial sums
 * over at most a2s_agreement_partial_cells() = 32 cells; everything above the lane partials is added in double, in an order that n alone fixes
 * (the lanes by a tree, chunk c into slot c mod 64 in ascending order, the slots in ascending order).  A segment's five doubles are therefore
 * bit-identical from run to run and do not depend on S, on its place in the table, on B, on T or on the other segments; inputs on a grid of 1/8 in
 * [0, 1] give the exact sums.  16-byte loads where F % 4 == 0, clip_stride % 4 == 0 and x and y are 16-byte aligned, 4-byte loads otherwise (the two
 * paths give a lane different cells, so the bits depend on which one runs).  No float atomics.  Two launches per 2048 segments; the slots are a device
 * array of the library's own, so calls that may overlap must be on one stream.  The entry point allocates nothing, does not synchronise and reads
 * nothing back.  Null pointers, B, T or F < 1, S < 0, clip_stride < T * F: A2S_ERR_ARG, nothing is launched; S = 0 returns 0 and launches nothing.
 * a2s_agreement_launches: launches so far (proof of the path). */
int a2s_segment_agreement(void* stream, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* seg, int S, double* out);
int a2s_agreement_launches(void);
int a2s_agreement_partial_cells(void);
/* ---- dynamic time warping of two feature tensors, segment by segment (csrc/a2s_dtw.hip): where inside its bar the resynthesis
 * of a decoded score is heard in the recording.  x, y, clip_stride, B, T, F: as for a2s_segment_agreement.  seg: device, S x 4 int32 =
 * [clip, f0, f1, r]; f0 and f1 are clamped to [0, T], n = f1 - f0 rows, the same rows of both tensors; r is the Sakoe-Chiba half-width: cell (i, j),
 * 0 <= i, j < n, is inside the band when |i - j| <= r, and r < 0 or r >= n means no band.  A clip outside [0, B) and an empty range give an empty
 * segment.  Segments may overlap, repeat and come in any order.
 * Buffers: n_max >= the longest segment, r_max >= the widest band (r_max < 0: some segment has none); w_max = n_max where r_max < 0 or
 * 2 r_max + 1 > n_max, else 2 r_max + 1.  The block of segment s starts at element s * n_max * w_max of the cost buffer (float32) and of the
 * workspace (one byte per cell), and holds, with W = 2 r + 1 where the segment has a band and 2 r + 1 < n, W = n otherwise,
 *     W < n:   n rows of W cells, cell (i, j) at i * W + (j - i + r)           (banded);
 *     W = n:   n rows of n cells, cell (i, j) at i * n + j                     (dense; cells outside a band are neither written nor read).
 * A segment with n > n_max or W > w_max does not fit and is treated as empty.  a2s_dtw_cost_bytes / a2s_dtw_workspace_bytes: the bytes both need.
 * a2s_dtw_cost: d[s][i][j] = sum_f e^2, e = (x[clip][f0 + i][f] - y[clip][f0 + j][f]) - off[s]; fp32, one chain per cell in ascending f,
 * acc = fmaf(e, e, acc).  off: device, S floats, NULL = 0 (the subtraction is then left out; e - 0 is e).  Only cells inside the band are computed.
 * Inputs on a grid of 1/8 in [0, 1] with off = 0 and F <= 2^18 give exact sums.  16-byte loads where F % 4 == 0, clip_stride % 4 == 0 and x and y are
 * 16-byte aligned, 4-byte loads otherwise; the arithmetic is the same on both paths.  Nothing outside a clip's T * F cells is read (the stride padding
 * may hold NaN).  One launch per 32768 segments.
 * a2s_dtw_path: D[0][0] = d[0][0], D[i][j] = d[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) over the predecessors that exist and lie in the band;
 * among equals the first in that order wins.  One fp32 addition per cell, no multiply: a float32 restatement on the same costs gives the same bits
 * and the same path.  path: S rows of 2 n_max - 1 int32; row s receives steps[s] <= 2 n - 1 entries (i << 16) | j from (0, 0) to (n - 1, n - 1),
 * ascending; entries behind steps[s] are not written.  total[s] = D[n-1][n-1].  An empty segment gives steps = 0 and total = 0 and writes nothing
 * else.  The direction of every cell goes to the workspace; what is read back from it is clamped before it steers the walk, and the walk ends after
 * 2 n - 1 cells whatever the workspace holds.  One launch per call, one workgroup per segment.
 * Both: a segment's results do not depend on S, on its place in the table, on B, on T or on the other segments, and are bit-identical from run to
 * run.  No atomics.  The entry points allocate nothing, do not synchronise and read nothing back.  Null pointers (off excepted), B, T or F < 1,
 * T > 4096, S < 0, clip_stride < T * F, n_max outside [1, T], a cost buffer or workspace smaller than the bytes above: A2S_ERR_ARG, nothing is
 * launched; S = 0 returns 0 and launches nothing.  a2s_dtw_launches: launches of the two kernels so far (proof of the path). */
size_t a2s_dtw_cost_bytes(int S, int n_max, int r_max);
size_t a2s_dtw_workspace_bytes(int S, int n_max, int r_max);
int a2s_dtw_cost(void* stream, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* seg, int S, const float* off, int n_max,
                 int r_max, float* cost, size_t cost_bytes);
int a2s_dtw_path(void* stream, const int* seg, int S, int B, int T, int n_max, int r_max, const float* cost, size_t cost_bytes, uint8_t* ws,
                 size_t ws_bytes, int* path, int* steps, float* total);
int a2s_dtw_launches(void);
/* ---- note dynamics by analysis by synthesis (csrc/a2s_dynamics.hip): the two device stages between the VQT of a resynthesis and
 * its next render (piano_a2s_amd/resynth.py: estimate_dynamics).  x, y, clip_stride, B, T, F: as for a2s_segment_agreement (x the recording's features,
 * y the resynthesis's).  rows: device, S x 8 int32 = [clip, fx, fy, n, b1, b2, b3, prog_row], one row per note; the rows of one clip are contiguous and
 * first (device, B + 1 int32, ascending from 0 to S) holds the clips' offsets.
 * a2s_note_levels: the cells of a row are the frames i < n crossed with the columns b_h - 1 .. b_h + 1 of every b_h >= 0; a cell counts only if its
 * column is in [0, F) and BOTH fx + i and fy + i are in [0, T):
 *     out[s] = [sum x[clip][fx + i][col], sum y[clip][fy + i][col], count]          (three doubles).
 * A clip outside [0, B) or n <= 0 gives three zeros; n above 64 is read as 64.  Rows may repeat and come in any order.  One wavefront per row, four rows
 * per workgroup: cell k = 9 i + 3 (h - 1) + (col - b_h + 1) belongs to lane k mod 64, a lane adds its cells in ascending k in double, and the lanes are
 * combined by a butterfly.  A row's three doubles are therefore bit-identical from run to run and do not depend on S, on the row's place, on B or on T
 * (beyond which cells count); inputs on a grid of 1/8 give the exact sums.  Nothing outside a clip's T * F cells is read (the stride padding may hold
 * NaN) and nothing outside out[0 : 3 S] is written.  No atomics.  One launch per call.  Null pointers, B, T or F < 1, S < 0, clip_stride < T * F:
 * A2S_ERR_ARG, nothing is launched; S = 0 returns 0 and launches nothing.
 * a2s_note_amp_update: per clip b over its k = first[b + 1] - first[b] rows (at most 512; a longer run is cut there), in fp32, one operation per step:
 *     d = (float)(80.0 * (Sx - Sy) / count)   (the division in double; d = 0 where count = 0);        c = cum + d;
 *     med = the lower median of c, the (k - 1) / 2-th smallest;                                          cum' = min(max(c - med, -30), 12);
 *     word 3 (the amplitude) of row prog_row of clip b's program = base_amp * exp2f(cum' * (log2(10) / 20));   cum = cum'.
 * A numpy float32 restatement on the same sums gives the same bits of cum.  programs: device, B programs of program_stride rows of 8 int32 each, as
 * a2s_render_notes reads them (its rows_per_clip); only word 3 of the listed rows is written, never the header, and a clip without rows is left alone.
 * The table lives on the device and the entry point reads nothing back, so a prog_row outside 1 .. program_stride - 1 cannot be refused here: the
 * kernel writes no amplitude for such a row (its cum is still updated), and piano_a2s_amd.hip.note_table refuses it on the host table before
 * anything is uploaded.  One workgroup per clip, the median by rank counting in LDS (rank = the smaller values + the equal values at a lower index).
 * One launch per call.  Null pointers, B < 1 or > 65535, program_stride < 2, base_amp not in (0, 1e30]: A2S_ERR_ARG, nothing is launched.
 * Both entry points allocate nothing, do not synchronise and read nothing back.  a2s_dynamics_launches: launches of the two so far (proof of the path). */
int a2s_note_levels(void* stream, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* rows, int S, double* out);
int a2s_note_amp_update(void* stream, const double* sums, const int* rows, const int* first, int B, float* cum, int* programs, int program_stride,
                        float base_amp);
int a2s_dynamics_launches(void);
/* ---- the tuning of a recording, estimated from the model's own features (csrc/a2s_tuning.hip): the two device stages in front of
 * a2s_shift_bins (piano_a2s_amd/tuning.py).  The features have S = bins_per_semitone bins per semitone and bin 0 is A0 at A4 = 440 Hz; a piano c cents
 * away from that puts every partial c * S / 100 bins beside its column.  H = 100 histogram cells per semitone (one cent each), Q = 4096.  Both entry
 * points take borrowed device pointers and a stream, allocate nothing, do not synchronise and read nothing back.
 * a2s_tuning_profile: x = B clips of `rows` rows of F float32 (dB / 80 + 1), row t of clip b at x + b * x_bstride + t * x_rstride (unit stride along F);
 * n_rows (B,) int32, clamped to [0, rows]: only the rows t < n_rows[b] count.  Over those rows and the bins 1 <= f <= F - 2, with a, c, e = x[t][f - 1],
 * x[t][f], x[t][f + 1]: a peak is c > a && c >= e && c >= thr (false with a NaN: a plateau, silence and NaN give none).  For a peak, in double:
 *     delta = 0.5 (a - e) / ((a - c) + (e - c))   (a NaN, which only cells at +-inf give, reads as 0);
 *     u = ((f mod S) + delta) + S / 2, u -= S where u >= S;   cell = min(H - 1, floor(u * H / S));   weight = 1 + rint(min(c - thr, 1) * Q);
 *     hist[b][cell] += weight;   hist[b][H] += 1   (the peak count).
 * Cell k stands for a deviation of [k - 50, k - 49) cents from the equal-tempered grid at 440 Hz.  hist: B rows of H + 1 int64, OVERWRITTEN (zeroing it
 * on the stream is part of the call).  One streaming pass, every cell read once (16-byte loads where F % 4 == 0, x is 16-byte aligned and both strides
 * are multiples of 4); integer LDS atomics per wave, 64-bit integer global atomics into hist, no float atomics: the integers do not depend on the order
 * of arrival, on B, on the strides or on a clip's place in the batch, and equal tests/tuning_oracle.py's.  Nothing outside a clip's rows x F cells is
 * read (the stride padding may hold NaN).  F < 3 gives zeros (no kernel runs).  Null pointers, B < 0 or > 65535, rows < 1, F < 1, bins_per_semitone < 1
 * or > 64, thr outside [0, 1] or not finite, a row stride < F or a clip stride < (rows - 1) * row stride + F: A2S_ERR_ARG, nothing is launched; B = 0
 * returns 0 and launches nothing.
 * a2s_tuning_estimate: group g is the clips first[g] .. first[g + 1] - 1 (first: device, G + 1 int32, ascending from 0 to B; a group may be empty; the
 * kernel clamps what it reads to [0, B], the host table is checked by piano_a2s_amd.hip.tuning_estimate before it is uploaded).  h = the group's
 * histograms added (int64); sm[k] = sum_{j = -6 .. 6} (7 - |j|) h[(k + j) mod H] (int64, exact); k* = the first arg max of sm; then in double:
 *     conf = sm[k*] * H / sum(sm)   (0 where the sum is 0);      A, C, E = sm[k* - 1], sm[k*], sm[k* + 1] (circular), den = (A - C) + (E - C);
 *     delta = 0.5 (A - E) / den where den < 0, else 0;          cents = ((k* + 0.5) + delta) * 100 / H - 50, cents -= 100 where it reaches 50;
 *     est[g] = [cents, conf, peaks]   (three doubles, always written);      determined = peaks >= min_peaks && conf >= min_conf;
 *     eff_bins[b] = (float)(determined ? -cents * S / 100 : 0.0) for every clip of the group: what a2s_shift_bins reads.
 * A numpy restatement (piano_a2s_amd.tuning.estimate_host) gives the same bits.  A group of zeros (an empty one too) gives [-49.5, 0, 0] and is not
 * determined.  cents lies in [-50, 50): a detuning beyond that is a transposition and cannot be told apart.  One workgroup per group, one launch.
 * Null pointers (hist and eff_bins may be null where B = 0), G < 0 or > 65535, B < 0, bins_per_semitone < 1 or > 64, min_conf not finite,
 * min_peaks < 0: A2S_ERR_ARG, nothing is launched; G = 0 returns 0 and launches nothing.
 * Limits: real strings are inharmonic, their stretched partials pull the estimate sharp by an amount nobody has measured here; one tuning per group.
 * a2s_tuning_launches: kernel launches of the two so far (proof of the path). */
int a2s_tuning_profile(void* stream, const float* x, long x_bstride, long x_rstride, const int* n_rows, int B, int rows, int F, int bins_per_semitone,
                       float thr, long long* hist);
int a2s_tuning_estimate(void* stream, const long long* hist, const int* first, int G, int B, int bins_per_semitone, double min_conf, int min_peaks,
                        double* est, float* eff_bins);
int a2s_tuning_launches(void);
/* ---- resynthesis at the performed timing (csrc/a2s_retime.hip): the two device stages between the DTW paths of a round and its
 * next render (piano_a2s_amd/resynth.py: refine_timing).  Integers only: the device EQUALS tests/retime_oracle.py.  table: device, S x 4 int32 =
 * [clip, f0, f1, r] as a2s_dtw_cost takes it; n = f1 - f0, read as 0 where it is outside [0, n_max].
 * a2s_path_warp: paths = S rows of path_stride int32, row s holding steps[s] cells (i << 16) | j as a2s_dtw_path writes them (i the recording's frame,
 * j the score's).  A path is TAKEN if n >= 1, n <= steps <= min(2 n - 1, path_stride), its first cell is (0, 0), its last (n - 1, n - 1) and every
 * step is (1, 1), (1, 0) or (0, 1).  Then, per row s of warp2 (S rows of n_max + 1 int32):
 *     warp2[j] = (first i matched to j) + (last i matched to j), j < n;      warp2[n] = warp2[n - 1] + 2;      warp2[j] = 2 j, n < j <= n_max
 * (twice resynth.warp_from_path, and the slope 1 behind the last frame of resynth.warp_time); inverse2 (the same shape, or NULL: not written) is the
 * same with i and j swapped.  A path that is not taken -- steps = 0, n = 0, a wrong end cell, cells outside [0, n) -- gives the identity 2 j over the
 * whole row: a reader never sees an uninitialised word.  One workgroup per segment, the first and last cells of the columns and rows in LDS (a cell is
 * the first of its column when the cell before it has another j, the last when the cell after it has another j), no atomics, one launch.
 * a2s_retime_events: events = E x 8 int32 [clip, prog_row, seg, bar_start, bar_stop, 0, 0, 0]; programs = B programs of program_rows rows of 8 int32
 * as a2s_render_notes reads them.  Words 0 (onset) and 1 (length) of row prog_row of clip's program are replaced, with h = hop, the row of warp2 of
 * segment seg and
 *     move(t):  p = min(max(t - f0 h, 0), n h);  k = min(p / h, n - 1);  rem = p - k h;
 *               shift2 = (h - rem) (warp2[k] - 2 k) + rem (warp2[k + 1] - 2 (k + 1));  move = t + floor(shift2 / 2)   (towards -inf; move = t where n = 0)
 *     on'  = min(clamp(move(onset), bar_start, bar_stop), bar_stop - 1);      end' = clamp(move(onset + length), bar_start, bar_stop);
 *     len' = max(1, min(max(end' - on', h), bar_stop - on'))
 * -- resynth.performed_notes in integers: within one sample per edge of it, non-decreasing in t, and the identity warp leaves every onset inside its
 * bar as it is.  With n <= 4096 and h <= 65535 every step fits an int32.  A row writes NOTHING if clip is outside [0, B), prog_row outside
 * [1, program_rows), seg outside [0, S), bar_stop <= bar_start, or the program row is a padding row (length <= 0): the table lives on the device and
 * the entry point reads nothing back, so such a row cannot be refused here (piano_a2s_amd.hip.event_table refuses it on the host table).  One thread
 * per event, two loads and two stores of the program per event, nothing else of the programs is touched.  Two rows that name the same program row
 * race; event_table refuses them.  One launch.
 * Both: no atomics, nothing allocated, no synchronisation, nothing read back; results do not depend on S, E or the place in a table.  Null pointers
 * (inverse2 excepted), negative counts, n_max outside [1, 4096], path_stride < 1, hop outside [1, 65535]: A2S_ERR_ARG, nothing is launched; S = 0 (or
 * E = 0) returns 0 and launches nothing.  a2s_retime_launches: launches of the two so far (proof of the path). */
int a2s_path_warp(void* stream, const int* paths, long path_stride, const int* steps, const int* table, int S, int n_max, int* warp2, int* inverse2);
int a2s_retime_events(void* stream, const int* warp2, int n_max, const int* table, int S, const int* events, int E, int hop, int* programs, int B,
                      int program_rows);
int a2s_retime_launches(void);
/* Round 6: the two NoteDecoders of a segment (/root/reference/models.py:261-275: decode_notes of the upper and of the lower staff over the same
 * encoder_outputs) issued by ONE host loop on their two streams; while both staves run a step, the step's attention sweep is one launch that reads
 * the encoder outputs once for both (csrc/a2s_seq.hip: attn_fwd_split256_pair).  pair_order / pair_rank: device, n_clips ints -- the clips sorted by
 * the step the last row of EITHER staff finishes at (latest first) and the inverse permutation; pair_n_active: HOST, max(steps) ints.  Training calls
 * with the finished-row bookkeeping only; anything else runs the two calls one after the other (a2s_note_decoder_fwd twice). */
int a2s_note_decoder_fwd_pair(void* stream_upper, void* stream_lower, const a2s_note_dec_args* upper, const a2s_note_dec_args* lower,
                              const int* pair_order, const int* pair_rank, const int* pair_n_active, int* steps_done_upper, int* steps_done_lower);
size_t a2s_note_step_workspace_floats(int H, int E);
/* scratch of the persistent path (0: that many clips are not supported) */
size_t a2s_note_decoder_persist_ws_bytes(int n_clips, int R, int steps);
size_t a2s_note_decoder_bwd_persist_ws_bytes(int n_clips);

/* ---- packed staff-embedding bi-GRU final states (get_staff_token_from_{gt,probs}, models.py:164-189).
 * gru_w: 8 device pointers {w_ih,w_hh,b_ih,b_hh} forward then reverse. */
int a2s_staff_emb_fwd(void* stream, const float* note_emb, const float* const* gru_w, const long long* ids64,
                      const int* ids32, long id_bstride, const long long* lengths, long len_stride, float* out,
                      long ldo, int col0, float* hsave, int R, int maxlen, int E, int S);

/* ======================================================================================= backward
 * Gradients follow torch.autograd on the reference graph.  All "+=" outputs accumulate (beta = 1 semantics). */

/* dx = g - exp(y) * rowsum(g) for y = log_softmax(x).  Row r of g/y at base + (r/inner)*outer_stride + (r%inner)*V;
 * time_major=1 writes dx row (r%inner)*n_outer + r/inner (step-major, to line up with the saved step buffers). */
int a2s_log_softmax_bwd_rows(void* stream, const float* g, const float* y, long outer_stride, int inner, float* dx,
                             int R, int V, int n_outer, int time_major);
/* GRU cell backward from the saved [r|z|n|gh_n]; dh = dh_a + dh_b (dh_b may be NULL); hprev NULL = zeros. */
int a2s_gru_gates_bwd(void* stream, const float* dh_a, long lda, const float* dh_b, long ldb, const float* save,
                      const float* hprev, long ldhp, float* dgi, long ldgi, float* dgh, long ldgh, float* dgh2, long ldgh2,
                      float* dhprev, long lddp, int R, int H);
/* one attention step backward: dq, ds (T per row) and the summed dctx (see csrc/a2s_bwd.hip) */
int a2s_attn_step_bwd(void* stream, const float* keys, const float* enc, const float* q, long ldq, const float* v,
                      const float* attw, const float* ctx, long ldctx, const float* dctx_a, long ldda, const float* dctx_b,
                      long lddb, float* dctx_out, long lddo, float* dq, long lddq, float* ds_out, int B, int T, int H, float* workspace);
int a2s_attn_step_bwd_rows(void* stream, const float* keys, const float* enc, const float* q, long ldq, const float* v, const float* attw,
                           const float* ctx, long ldctx, const float* dctx_a, long ldda, const float* dctx_b, long lddb, float* dctx_out,
                           long lddo, float* dq, long lddq, float* ds_out, int R, int T, int H, float* workspace, int n_clips,
                           const int* clip_order, const int* clip_rank, const int* row_until, int n_active, int step);
/* deferred key gradient of S steps: dK += ..., dv partials [B*ceil(T/16)][H] (reduce with a2s_col_sum) */
int a2s_attn_dk_accum(void* stream, const float* keys, const float* q_all, const float* ds_all, const float* v, float* dK,
                      float* dv_partial, int B, int T, int S, int H, const int* row_until, int groups);
/* q_all / ds_all rows: (step, group, clip) with `groups` fused bars per step (1 = plain); row_until (optional, groups*B ints):
 * the ds rows of (group, clip) are zero from step row_until[group*B + clip] on and are not read */
int a2s_attn_dk_blocks(int B, int T);
/* deferred encoder-output gradient of S steps: dEnc[b] (T x H2) += sum over the live (step, group) pairs of attw[row]^T dctx[row], same row
 * conventions (attw_all rows of T, dctx_all rows of H2 floats, both dense); the rows of finished pairs are not read.  H2 must be 512: the
 * caller takes a2s_gemm_f32 for every other width.  Fixed summation order (ascending pairs), no atomics. */
int a2s_attn_denc_accum(void* stream, const float* attw_all, const float* dctx_all, float* dEnc, int B, int T, int S, int H2,
                        const int* row_until, int groups);
/* out[c] = alpha * sum_r x[r*ld+c] + beta*out[c]; with a workspace (>= 2*C floats, ideally 1024*C) long matrices are reduced in two
 * stages over many workgroups (fixed partition: deterministic). */
int a2s_col_sum(void* stream, const float* x, long ld, float* out, long rows, int C, float alpha, float beta, float* workspace, size_t workspace_floats);
int a2s_embed_scatter_add(void* stream, float* table_grad, const long long* ids64, const int* ids32, long id_stride,
                          int const_id, const float* g, long ldg, int col0, int R, int E, const uint8_t* keep_mask, float inv_keep);
int a2s_ew_act_bwd(void* stream, const float* g, const float* y, float* dx, long n, int act);

typedef struct a2s_note_dec_bwd_args {
    const float* attn_w; const float* attn_v; const float* w_ih; const float* w_hh;
    const float* keys; const float* enc;
    const float* h; const float* x; const float* q; const float* gates; const float* attw;   /* saved by the forward */
    const float* do_all;                 /* (steps, R, 4H): dlogits_all W_out = [dh | dctx] of the output projection */
    float* dgi_all; float* dgh_all; float* dq_all; float* ds_all; float* dctx_all; float* dx;
    float* dh;                           /* (2, R, 2H) carry; dh[0] = gradient wrt the initial hidden on return */
    float* attn_ws;                      /* as in the forward call */
    float* gemm_ws; size_t gemm_ws_bytes;   /* split-K scratch for the per-step skinny GEMMs (NULL: no split-K) */
    const int* clip_order;               /* the forward's fused-bars / finished-rows description (or NULLs): see a2s_note_dec_args */
    const int* clip_rank;
    const int* row_until;
    const int* n_active;                 /* HOST */
    int n_clips;
    const int* m_active;                 /* HOST or NULL: as in the forward call (the call zero-fills dx first) */
    const int* row_list;                 /* device or NULL, and */
    const int* n_rows_active;            /* HOST: as in the forward call */
    int R, T, H, E, steps;
    float* step_ws; size_t step_ws_floats;   /* as in the forward call (holds the transposed weight copies of the fused backward step) */
    float* persist_ws; size_t persist_ws_bytes;   /* round 4: a2s_note_decoder_bwd_persist_ws_bytes(n_clips) bytes (256-byte aligned) or NULL:
                                                     at most 8 clips run the reverse loop as ONE persistent launch (csrc/a2s_dec_persist.hip) */
    const float* w_ih_full;                  /* unused (reserved) */
} a2s_note_dec_bwd_args;
int a2s_note_decoder_bwd(void* stream, const a2s_note_dec_bwd_args* args);
/* Round 6: the reverse loops of a segment's two NoteDecoders from one host loop on their two streams, the attention sweep of a step as ONE launch
 * for both staves while both step (see a2s_note_decoder_fwd_pair; autograd of /root/reference/models.py:261-275). */
int a2s_note_decoder_bwd_pair(void* stream_upper, void* stream_lower, const a2s_note_dec_bwd_args* upper, const a2s_note_dec_bwd_args* lower,
                              const int* pair_order, const int* pair_rank, const int* pair_n_active);

/* BPTT of one encoder GRU direction (reverse of a2s_gru_seq_fwd) */
int a2s_gru_seq_bwd(void* stream, const float* dout, long do_bstride, long do_tstride, const float* out, long out_bstride,
                    long out_tstride, const float* gates, const float* w_hh, const float* dhn, float* dgi_all, float* dgh_shift,
                    float* dgh_first, float* dhbuf, float* dgh_tmp, int B, int T, int H, int reverse, float* workspace, size_t workspace_bytes);
/* ... which also hands out the operand ranges of the deferred weight-gradient products: ranges_out (DEVICE, 2 floats) <- max |dgi_all|,
 * max |dgh_shift|, bit-equal to a2s_absmax of the two tensors, when the call ran as one persistent launch; *ranges_valid (HOST) <- 1 then, 0
 * otherwise (the launch-per-step kernels do not produce them: measure the tensors with a2s_absmax). */
int a2s_gru_seq_bwd_ranged(void* stream, const float* dout, long do_bstride, long do_tstride, const float* out, long out_bstride,
                           long out_tstride, const float* gates, const float* w_hh, const float* dhn, float* dgi_all, float* dgh_shift,
                           float* dgh_first, float* dhbuf, float* dgh_tmp, int B, int T, int H, int reverse, float* workspace, size_t workspace_bytes,
                           float* ranges_out, int* ranges_valid);
/* Bytes of `workspace` (256-byte aligned) with which a2s_gru_seq_fwd and a2s_gru_seq_bwd / _ranged take their fastest path at B clips of width H:
 * the transposed W_hh, the launch-per-step kernel's scratch and, at H = 256, the persistent launches' granule buffers.  With less the calls still
 * compute the same values on slower kernels (a2s_debug_get "gru_persist_*_launches" / "gru_step_*_launches" tell which ran).  0: B < 1 or H < 1. */
size_t a2s_gru_workspace_bytes(int B, int H);
/* BPTT of the packed staff-embedding bi-GRU; grads: DEVICE array of 8 pointers (same order as gru_w) */
int a2s_staff_emb_bwd(void* stream, const float* note_emb, const float* const* gru_w, float* const* grads, float* note_emb_grad,
                      const long long* ids64, const int* ids32, long id_bstride, const long long* lengths, long len_stride,
                      const float* dout, long lddo, int col0, const float* hsave, int R, int maxlen, int E, int S);

/* BatchNorm(+ReLU, + optional dropout on the (rows,C) layout) backward, training statistics (models.py:525-541):
 * dgamma/dbeta +=, dx written (may alias g; NULL = statistics only: c12 is left for a2s_conv3x3_wgrad_bn, which forms dx itself).
 * rows x C x F elements, channel of element i = (i/F)%C.
 * partial: a2s_bn_bwd_partial_floats() floats of scratch; c12: 2*C floats of scratch. */
int a2s_bn_bwd(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
               const float* shift, const uint8_t* keep_mask, float inv_keep, float* dgamma, float* dbeta, float* dx,
               float* partial, float* c12, long rows, int C, int F);
int a2s_bn_bwd_amax(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
                    const float* shift, const uint8_t* keep_mask, float inv_keep, float* dgamma, float* dbeta, float* dx,
                    float* partial, float* c12, long rows, int C, int F, float* dx_absmax);
size_t a2s_bn_bwd_partial_floats(long rows, int C, int F);
/* the same in two halves for synchronised BatchNorm: (1) this rank's per-channel {sum g', sum g' xhat} -> sums[2C];
 * [host: all-reduce];  (2) dgamma/dbeta += LOCAL sums, dx from the GLOBAL sums / global element count. */
int a2s_bn_bwd_stats(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
                     const float* shift, const uint8_t* keep_mask, float inv_keep, float* partial, float* sums, long rows, int C, int F);
int a2s_bn_bwd_apply(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
                     const float* shift, const uint8_t* keep_mask, float inv_keep, const float* sums_local, const float* sums_global,
                     double count_global, float* dgamma, float* dbeta, float* dx, float* c12, long rows, int C, int F);
/* ... and for statistics the producer of g already reduced into per-block partials (a2s_conv3x3_dgrad_bnstats*, a2s_linear_dgrad_bnstats):
 * (1) partial[nblocks][C][2] -> this rank's sums[2C]; [host: all-reduce]; (2) dgamma / dbeta += LOCAL sums, c12 = GLOBAL sums / global element
 * count -- no pass over (g, x); the input gradient is formed by the fused consumer (a2s_conv3x3_wgrad_bn_ranged).  With these the synchronised
 * BatchNorm of torch.nn.SyncBatchNorm (what SpeechBrain's DDP wrapping gives reference pretrain.py:257) keeps every fused path of the per-rank one. */
int a2s_bn_bwd_sums_from_partial(void* stream, const float* partial, int nblocks, int C, float* sums);
int a2s_bn_bwd_c12_from_sums(void* stream, const float* sums_local, const float* sums_global, double count_global, float* dgamma, float* dbeta,
                             float* c12, int C);
/* conv weight gradient dW += dy (*) relu(x*in_scale+in_shift)  (deterministic two-stage reduction) */
int a2s_conv3x3_wgrad(void* stream, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dW,
                      float* workspace, size_t workspace_bytes, int B, int T, int F, int Cin, int Cout);
/* ... with max |dy| (device scalar written by a2s_bn_bwd*_amax) for the two-term fp16 path of the split-operand kernel (NULL: as above) */
int a2s_conv3x3_wgrad_scaled(void* stream, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dW,
                             float* workspace, size_t workspace_bytes, int B, int T, int F, int Cin, int Cout, const float* dy_absmax);
/* ... with the RANGE of the activated operand relu(x * in_scale[c] + in_shift[c]) as well (round 3): act_absmax = device scalar from
 * a2s_act_bound (NULL: operand used unscaled, as a2s_conv3x3_wgrad_scaled).  Reference: autograd of nn.Conv2d, models.py:525-534. */
int a2s_conv3x3_wgrad_ranged(void* stream, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dW, float* workspace,
                             size_t workspace_bytes, int B, int T, int F, int Cin, int Cout, const float* dy_absmax, const float* act_absmax);
/* out[0] = max_c (|scale[c]| * absmax[c] + |shift[c]|): hard bound of relu(x * scale[c] + shift[c]) over a tensor whose producer wrote the
 * per-channel max |x| (a2s_conv3x3_ranged); the operand range handed to the kernels that apply BatchNorm + ReLU while staging
 * (a2s_conv3x3_wgrad_ranged, a2s_gemm_f32_affine_scaled).  Nothing comparable in the reference (fp32 throughout). */
int a2s_act_bound(void* stream, const float* scale, const float* shift, const float* absmax, int C, float* out);
size_t a2s_conv3x3_wgrad_workspace_bytes(int Cin, int Cout);
/* The same with the BatchNorm backward of the layer's output folded into the staging of the dy operand: g = gradient wrt
 * relu(bn(y)), y = the layer's pre-BN output, c12 from a2s_bn_bwd(..., dx = NULL); dy = scale*(g' - c1 - xhat*c2) is formed on the fly
 * and also written to dy_out (may be NULL) for the data-gradient convolution that follows -- the separate apply pass disappears. */
int a2s_conv3x3_wgrad_bn(void* stream, const float* g, const float* y, const float* mean, const float* invstd, const float* scale, const float* shift,
                         const float* c12, float* dy_out, const float* x, const float* in_scale, const float* in_shift, float* dW, float* workspace,
                         size_t workspace_bytes, int B, int T, int F, int Cin, int Cout);
/* Round 4: the same fusion on the row-streaming weight-gradient kernel (csrc/a2s_conv_wrows.hip, two-term fp16 operands), for the shapes
 * a2s_conv3x3_wgrad_bn_ranged_eligible accepts (F % 4 == 0, 20 / 40 channels): its staging waves form dz from (g, y), write it to dy_out
 * (required: the data-gradient convolution reads it) and fold max |dz| into dy_absmax_out (device scalar, zeroed by the call).  The operand
 * scale of dz comes from a BOUND derived on the device from g_absmax[g_absmax_n] (max |g|, one value or one per channel, reduced by the kernel
 * that wrote g: a2s_linear_dgrad_bnstats, a2s_conv3x3_dgrad_bnstats_ranged) and y_absmax[Cout] (max |y_c|, written by the forward
 * convolution: a2s_conv3x3_ranged); act_absmax as in a2s_conv3x3_wgrad_ranged. */
int a2s_conv3x3_wgrad_bn_ranged(void* stream, const float* g, const float* y, const float* mean, const float* invstd, const float* scale, const float* shift,
                                const float* c12, const float* g_absmax, int g_absmax_n, const float* y_absmax, float* dy_out, float* dy_absmax_out, const float* x,
                                const float* in_scale, const float* in_shift, float* dW, float* workspace, size_t workspace_bytes, int B, int T, int F,
                                int Cin, int Cout, const float* act_absmax);
int a2s_conv3x3_wgrad_bn_ranged_eligible(int F, int Cin, int Cout);

/* ---- objective and optimizer of the recipe (pretrain.py:72-88,:125-128; pretrain.yaml:44-54)
 * NLL, mean over targets != ignore_index (pass -1 for "none"): loss_out[0] = loss, loss_out[1] = 1/count;
 * dlogp (zero-filled by the caller, or NULL) receives d(gscale*loss)/dlogp.  partial: 2*nblocks doubles. */
int a2s_nll_loss(void* stream, const float* logp, const long long* target, long rows, int V, long long ignore_index,
                 float* loss_out, float* dlogp, float gscale, double* partial, int nblocks);
/* the gradient alone for `rows` rows, with loss_out[1] = 1/count given by the caller (the count of targets != ignore_index over the WHOLE
 * minibatch is known from the targets): dlogp (zero-filled) receives d(gscale*loss)/dlogp of these rows. */
int a2s_nll_grad(void* stream, float* dlogp, const long long* target, const float* loss_out, float gscale, long rows, int V,
                 long long ignore_index);
/* clip_grad_norm_(max_norm) + Adadelta over one flat buffer; skipped when *loss (NULL: not looked at) or the gradient norm is not finite.
 * ctl[0..2] = {total norm, clip coefficient, applied flag}; partial: nblocks doubles; zero_grad clears the gradients. */
int a2s_clip_adadelta(void* stream, float* params, float* grads, float* square_avg, float* acc_delta, long n, const float* loss,
                      float max_norm, float lr, float rho, float eps, float* ctl, double* partial, int nblocks, int zero_grad);

/* ---- VQT front-end epilogue (utilities.get_VQT, utilities.py:240-254): C (B, rows, 2*bins) = [re | im] of the framed complex GEMM
 * (run with a2s_gemm_f32, A row stride = hop) -> out (B, rows, bins) = dB relative to the clip maximum, floor 1e-5, top_db, /80 + 1.
 * partial: B*64 floats of scratch.  Null pointers, B < 1, rows < 1 or bins < 1: A2S_ERR_ARG, nothing is launched. */
int a2s_vqt_logmag(void* stream, const float* C, float* out, float* partial, int B, long rows, int bins, float top_db);
/* the same over a response laid out octave by octave: C (B, rows, n_oct * 2 * bins_per_octave), octave o (HIGHEST first) = [re | im] of its
 * bins_per_octave bins -- what one framed GEMM per octave against the (n_fft, 2 * bins_per_octave) bank writes.  Null pointers, B < 1, rows < 1,
 * bins < 1, bins_per_octave < 1 or bins no multiple of bins_per_octave: A2S_ERR_ARG, nothing is launched. */
int a2s_vqt_logmag_octaves(void* stream, const float* C, float* out, float* partial, int B, long rows, int bins, int bins_per_octave, float top_db);
/* decimation by 2 between the octaves of librosa.vqt's recursion (librosa.resample(y, orig_sr=2, target_sr=1, scale=True); the filter is this
 * build's stand-in for libsoxr, see piano_a2s_amd/vqt.py): out[b][m] = sum_j ypad[b][2 m + j] taps[j], ntaps even and <= 4096; ypad (B, padded_len),
 * rows padded_len floats apart, with any padded_len >= 1: ypad[b][s] is taken as zero for every s >= padded_len (never read, so a short row does not
 * reach into the next clip's), out (B, n_out).  Null pointers, B < 1, n_out < 1, padded_len < 1, ntaps < 2, odd or > 4096: A2S_ERR_ARG, nothing is
 * launched. */
int a2s_vqt_decimate(void* stream, const float* ypad, long padded_len, const float* taps, int ntaps, float* out, long n_out, int B);

/* ---- scoring of the VALID / TEST stages (pretrain.py:216-249: jiwer.wer per clip on the host): unit-cost Levenshtein distance of n_pairs
 * independent pairs of word sequences, one launch, one wave per pair (csrc/a2s_metrics.hip).  ref / hyp: the pairs' words (any int32 codes;
 * equal code = equal word) one after the other; ref_off / hyp_off: n_pairs + 1 offsets into them; order: n_pairs pair indices in the order the
 * device should take them (longest first keeps the tail of the launch short; NULL: as they come); dist: n_pairs ints.  All of these are device
 * pointers.  No side of a pair may be longer than a2s_edit_distance_max_len() words (>= 2047): checked on max_ref_len / max_hyp_len, the HOST
 * values the caller passes -- the library neither reads device memory back nor synchronises; a pair that is longer all the same is not
 * indexed and gets dist = -1.  Bad arguments (negative counts, over-capacity lengths, a null pointer with n_pairs > 0) are refused before
 * anything is launched; n_pairs == 0 returns 0 and launches nothing.  a2s_debug_get("edit_distance_launches") counts the launches. */
int a2s_edit_distance(void* stream, const int* ref, const long long* ref_off, const int* hyp, const long long* hyp_off, const int* order,
                      int n_pairs, int max_ref_len, int max_hyp_len, int* dist);
int a2s_edit_distance_max_len(void);

/* ---- note-level scoring of decoded bars (csrc/a2s_notes.hip; the definition is piano_a2s_amd/metrics.py: note_events).
 * n_pairs pairs of bar rows (target, prediction), one workgroup each, one launch.  ref / hyp: the rows' token ids one after the other (int32;
 * a row counts up to its first <eos>); ref_off / hyp_off: n_pairs + 1 offsets into them.  Vocabulary tables of V int32 each: dur_ticks (ticks of a
 * duration symbol, 147840 to the whole note; 0: no duration), midi (MIDI number of a pitch symbol, A2S_NOTE_MIDI_REST for the rest, -1: no pitch),
 * cls (A2S_NOTE_CLS_*).  An id outside [0, V) is ignored like <pad> and indexes no table.  out: 8 ints per pair = n_ref, n_hyp, tp_pitch,
 * tp_onset, tp_value, tp_spelled, flags (bit 0 / 1: the target / prediction row has events beyond the eighth spine, which are dropped), 0.
 * A pair with a row of more than a2s_note_match_max_len() (1024) ids is not read and gets -1 in its six counts.  All pointers are device
 * pointers; nothing is read back or synchronised.  Bad arguments (a null pointer, n_pairs < 0, V < 1) are refused before anything is launched;
 * n_pairs == 0 launches nothing.  a2s_note_match_launches: launches so far (proof of the path). */
#define A2S_NOTE_CLS_OTHER 0
#define A2S_NOTE_CLS_TAB 1
#define A2S_NOTE_CLS_NL 2
#define A2S_NOTE_CLS_FERM 3
#define A2S_NOTE_CLS_CLOSE 4
#define A2S_NOTE_CLS_EOS 5
#define A2S_NOTE_CLS_IGNORE 6
#define A2S_NOTE_MIDI_REST (-2)
int a2s_note_match(void* stream, const int* ref, const long long* ref_off, const int* hyp, const long long* hyp_off, int n_pairs,
                   const int* dur_ticks, const int* midi, const int* cls, int V, int* out);
int a2s_note_match_max_len(void);
long a2s_note_match_launches(void);

#ifdef __cplusplus
}
#endif
#endif
