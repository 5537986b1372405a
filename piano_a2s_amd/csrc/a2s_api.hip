// extern "C" surface of liba2s_hip.so (declared in include/a2s.h): thin, exception-free trampolines onto the
// *_impl launchers of the kernel translation units (a2s_internal.h), and the storage of the switch table (a2s_switches.h).
#define A2S_SWITCHES_IMPL
#include "a2s_internal.h"

thread_local char a2s_err_msg[512] = {0};
long long a2s_launch_counter = 0;

#define ST ((hipStream_t)stream)

extern "C" {

const char* a2s_last_error(void) { return a2s_err_msg; }
int a2s_version(void) { return 1; }
long long a2s_launch_count(void) { return __atomic_load_n(&a2s_launch_counter, __ATOMIC_RELAXED); }

int a2s_gemm_f32(void* stream, int M, int N, int K, float alpha, const float* A, long sAm, long sAk, const float* B, long sBk,
                 long sBn, float beta, float* C, long ldc, const float* bias, int act, int batch, long bsA, long bsB, long bsC,
                 int splitk, float* workspace, size_t workspace_bytes) {
    return a2s_gemm_impl(ST, M, N, K, alpha, A, sAm, sAk, B, sBk, sBn, beta, C, ldc, bias, act, batch, bsA, bsB, bsC, splitk,
                         workspace, workspace_bytes);
}
int a2s_gemm_f32_affine(void* stream, int M, int N, int K, float alpha, const float* A, long sAm, long sAk, const float* B, long sBk,
                        long sBn, float beta, float* C, long ldc, const float* bias, int act, int batch, long bsA, long bsB, long bsC,
                        int splitk, float* workspace, size_t workspace_bytes, const float* a_scale, const float* a_shift, int a_period,
                        const float* b_scale, const float* b_shift, int b_period) {
    return a2s_gemm_affine_impl(ST, M, N, K, alpha, A, sAm, sAk, B, sBk, sBn, beta, C, ldc, bias, act, batch, bsA, bsB, bsC, splitk,
                                workspace, workspace_bytes, a_scale, a_shift, a_period, b_scale, b_shift, b_period,
                                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr);
}
int a2s_gemm_f32_affine_scaled(void* stream, int M, int N, int K, float alpha, const float* A, long sAm, long sAk, const float* B, long sBk,
                               long sBn, float beta, float* C, long ldc, const float* bias, int act, int batch, long bsA, long bsB, long bsC,
                               int splitk, float* workspace, size_t workspace_bytes, const float* a_scale, const float* a_shift, int a_period,
                               const float* b_scale, const float* b_shift, int b_period, const float* a_absmax, const float* b_absmax) {
    return a2s_gemm_affine_impl(ST, M, N, K, alpha, A, sAm, sAk, B, sBk, sBn, beta, C, ldc, bias, act, batch, bsA, bsB, bsC, splitk,
                                workspace, workspace_bytes, a_scale, a_shift, a_period, b_scale, b_shift, b_period,
                                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, a_absmax, b_absmax);
}
int a2s_gemm_f32_bnstats_scaled(void* stream, int M, int N, int K, const float* A, long sAm, long sAk, const float* B, long sBk, long sBn, float* C, long ldc,
                                const float* y, const float* mean, const float* invstd, const float* scale, const float* shift, int period, float* partial,
                                const float* a_absmax, const float* b_absmax) {
    return a2s_gemm_affine_impl(ST, M, N, K, 1.f, A, sAm, sAk, B, sBk, sBn, 0.f, C, ldc, nullptr, 0, 1, 0, 0, 0, 1, nullptr, 0,
                                nullptr, nullptr, 0, nullptr, nullptr, 0, y, mean, invstd, scale, shift, partial, period, 1, a_absmax, b_absmax);
}
int a2s_absmax(void* stream, const float* x, long n, float* out) { return a2s_absmax_impl(ST, x, n, out); }
int a2s_linear_dgrad_bnstats(void* stream, int M, int N, int K, const float* dz, long lda, const float* Wt, float* da, long ldc, const float* y,
                             const float* mean, const float* invstd, const float* scale, const float* shift, int period, float* partial,
                             const float* dz_absmax, const float* w_absmax, float* workspace, size_t workspace_bytes, float* da_absmax_out) {
    return a2s_linear_dgrad_bnstats_impl(ST, M, N, K, dz, lda, Wt, 1, K, da, ldc, y, mean, invstd, scale, shift, period, partial, dz_absmax, w_absmax,
                                         workspace, workspace_bytes, da_absmax_out);
}
size_t a2s_linear_dgrad_ws_bytes(int N, int K) { return a2s_linear_dgrad_ws_bytes_impl(N, K); }
int a2s_linear_fwd(void* stream, int M, int N, int K, const float* y, long lda, const float* W, float* z, long ldc, const float* scale, const float* shift,
                   int period, const float* y_absmax, const float* w_absmax, float* workspace, size_t workspace_bytes) {
    return a2s_linear_fwd_impl(ST, M, N, K, y, lda, W, z, ldc, scale, shift, period, y_absmax, w_absmax, workspace, workspace_bytes);
}
int a2s_linear_wgrad(void* stream, int M, int N, int K, const float* dz, long ldz, const float* y, long lda, float* G, long ldg, const float* scale,
                     const float* shift, int period, const float* dz_absmax, const float* y_absmax, float* workspace, size_t workspace_bytes) {
    return a2s_linear_wgrad_impl(ST, M, N, K, dz, ldz, y, lda, G, ldg, scale, shift, period, dz_absmax, y_absmax, workspace, workspace_bytes);
}
size_t a2s_linear_wgrad_ws_bytes(int M, int K) { return a2s_linear_wgrad_ws_bytes_impl(M, K); }
int a2s_linear_wgrad_eligible(int M, int N, int K, int period) { return a2s_linear_wgrad_ok(M, N, K, 256, 4, 4, period, nullptr, nullptr, nullptr) ? 1 : 0; }
int a2s_tallk_wgrad(void* stream, int M, int Np, int K, const float* P, long ldp, const float* A, long lda, float* G, long ldg, int transposed, float* bias,
                    const float* p_absmax, const float* a_absmax, float* workspace, size_t workspace_bytes) {
    return a2s_tallk_wgrad_impl(ST, M, Np, K, P, ldp, A, lda, G, ldg, transposed, bias, p_absmax, a_absmax, workspace, workspace_bytes);
}
size_t a2s_tallk_wgrad_ws_bytes(int M, int Np, int K) { return a2s_tallk_wgrad_ws_bytes_impl(M, Np, K); }
int a2s_tallk_wgrad_eligible(int M, int Np, int K, long ldp, long lda, long ldg, int transposed) {
    return a2s_tallk_wgrad_ok(M, Np, K, ldp, lda, ldg, transposed, nullptr, nullptr, nullptr, nullptr) ? 1 : 0;
}
int a2s_linear_fwd_eligible(int M, int N, int K, int period) { return a2s_linear_fwd_ok(M, N, K, 4, 4, period, nullptr, nullptr, nullptr) ? 1 : 0; }
int a2s_linear_dgrad_blocks(int M) { return a2s_linear_dgrad_blocks_impl(M); }
int a2s_linear_dgrad_eligible(int M, int N, int K, int period) {
    return a2s_linear_dgrad_ok(M, N, K, 4, 1, K, 4, period, nullptr, nullptr, nullptr, nullptr) ? 1 : 0;
}
int a2s_gemm_f32_bnstats(void* stream, int M, int N, int K, const float* A, long sAm, long sAk, const float* B, long sBk, long sBn, float* C, long ldc,
                         const float* y, const float* mean, const float* invstd, const float* scale, const float* shift, int period, float* partial) {
    return a2s_gemm_affine_impl(ST, M, N, K, 1.f, A, sAm, sAk, B, sBk, sBn, 0.f, C, ldc, nullptr, 0, 1, 0, 0, 0, 1, nullptr, 0,
                                nullptr, nullptr, 0, nullptr, nullptr, 0, y, mean, invstd, scale, shift, partial, period, 0, nullptr, nullptr);
}
int a2s_gemm_bnstats_blocks(int M, int period) { return a2s_cdiv(M, 128) * a2s_gemm_bnstats_slots(period); }
size_t a2s_gemm_workspace_bytes(int M, int N, int batch, int splitk) { return a2s_gemm_workspace_bytes_impl(M, N, batch, splitk); }
int a2s_gemm_pick_splitk(int M, int N, int K, int batch) { return a2s_gemm_pick_splitk_impl(M, N, K, batch); }
void a2s_gemm_debug_tile(int cfg) { a2s_gemm_debug_tile_impl(cfg); }
size_t a2s_note_step_workspace_floats(int H, int E) { return a2s_note_step_workspace_floats_impl(H, E); }
int a2s_debug_set(const char* key, int value) {
    if (!key) return A2S_ERR_ARG;
    const int id = a2s_switch_find(key);
    if (id >= 0) { a2s_switch_store(id, value); return A2S_OK; }
    if (!strcmp(key, "attn_deferred_fast")) { a2s_attn_deferred_fast = value ? 1 : 0; return A2S_OK; }
    if (!strcmp(key, "tallk_wgrad")) { a2s_tallk_wgrad_on = value ? 1 : 0; return A2S_OK; }
    if (!strcmp(key, "tallk_wgrad_max_splits")) { a2s_tallk_wgrad_max_splits = value > 0 ? value : 0; return A2S_OK; }
    if (!strcmp(key, "conv_rows_stage")) { a2s_conv_rows_stage = value & 3; return A2S_OK; }
    if (!strcmp(key, "gemm_tile")) { a2s_gemm_debug_tile_impl(value); return A2S_OK; }          // write-only
    snprintf(a2s_err_msg, sizeof(a2s_err_msg), "a2s_debug_set: unknown key %s", key);
    return A2S_ERR_ARG;
}
int a2s_env_check(void) {
    if (const char* e = a2s_switch_env_error()) A2S_FAIL(A2S_ERR_ARG, "%s: expected a decimal number >= 0", e);
    return A2S_OK;
}

int a2s_persist_abort_latch(void* device_word) { a2s_persist_latch_set(device_word); return A2S_OK; }

int a2s_debug_get(const char* key) {
    if (!key) return -1;
    const int id = a2s_switch_find(key);
    if (id == A2S_SW_attn_pair_fused_rows) return a2s_attn_pair_fused_rows();
    if (id >= 0) return a2s_sw((a2s_switch)id);
    // read-only: launch counters (tests: proof of the path taken) and what the runtime reports for the current device
    if (!strcmp(key, "attn_pair_launches")) return (int)a2s_attn_pair_launches();
    if (!strcmp(key, "attn_pair_bwd_launches")) return (int)a2s_attn_pair_bwd_launches();
    if (!strcmp(key, "attn_deferred_fast")) return a2s_attn_deferred_fast;
    if (!strcmp(key, "tallk_wgrad")) return a2s_tallk_wgrad_on;
    if (!strcmp(key, "tallk_wgrad_max_splits")) return a2s_tallk_wgrad_max_splits;
    if (!strcmp(key, "tallk_wgrad_launches")) return (int)a2s_tallk_wgrad_launches();
    if (!strcmp(key, "attn_dk_ahead_launches")) return (int)a2s_attn_dk_ahead_launches();
    if (!strcmp(key, "attn_denc_launches")) return (int)a2s_attn_denc_launches();
    if (!strcmp(key, "dec_mid_launches")) return a2s_dec_mid_launches();
    if (!strcmp(key, "dec_cmb_launches")) return a2s_dec_cmb_launches();
    if (!strcmp(key, "dec_persist_launches")) return a2s_dec_persist_launches();
    if (!strcmp(key, "gru_persist_fwd_launches")) return (int)a2s_gru_persist_fwd_launches();
    if (!strcmp(key, "gru_persist_bwd_launches")) return (int)a2s_gru_persist_bwd_launches();
    if (!strcmp(key, "gru_step_fwd_launches")) return (int)a2s_gru_step_fwd_launches();
    if (!strcmp(key, "gru_step_bwd_launches")) return (int)a2s_gru_step_bwd_launches();
    if (!strcmp(key, "edit_distance_launches")) return (int)a2s_edit_distance_launches();
    if (!strcmp(key, "conv_rows16_c20_launches")) return (int)a2s_conv_rows16_c20_launches();
    if (!strcmp(key, "conv_rows_stage")) return a2s_conv_rows_stage;
    if (!strcmp(key, "conv_rows_stage_launches")) return (int)a2s_conv_rows_stage_launches();
    if (!strcmp(key, "device_cus")) return a2s_device_geometry().cus;
    if (!strcmp(key, "device_xccs")) return a2s_device_geometry().xccs;
    return -1;
}

int a2s_conv3x3(void* stream, const float* x, const float* w, float* y, const float* in_scale, const float* in_shift,
                float* stat_partial, int B, int T, int F, int Cin, int Cout, int flip, float* workspace) {
    return a2s_conv3x3_impl(ST, x, w, y, in_scale, in_shift, stat_partial, B, T, F, Cin, Cout, flip, workspace, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr);
}
int a2s_conv3x3_ranged(void* stream, const float* x, const float* w, float* y, const float* in_scale, const float* in_shift, const float* in_absmax,
                       float* stat_partial, float* out_absmax, int B, int T, int F, int Cin, int Cout, float* workspace) {
    return a2s_conv3x3_impl(ST, x, w, y, in_scale, in_shift, stat_partial, B, T, F, Cin, Cout, 0, workspace, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            in_absmax, out_absmax);
}
int a2s_conv3x3_dgrad_bnstats(void* stream, const float* dy, const float* w, float* g, const float* yl, const float* yl_mean, const float* yl_invstd,
                              const float* yl_scale, const float* yl_shift, float* stat_partial, int B, int T, int F, int Cin, int Cout,
                              float* workspace) {
    if (!yl) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "conv3x3_dgrad_bnstats: yl is required"); return A2S_ERR_ARG; }
    return a2s_conv3x3_impl(ST, dy, w, g, nullptr, nullptr, stat_partial, B, T, F, Cin, Cout, 1, workspace, yl, yl_mean, yl_invstd, yl_scale, yl_shift, nullptr, nullptr, nullptr);
}
int a2s_conv3x3_dgrad_bnstats_scaled(void* stream, const float* dy, const float* w, float* g, const float* yl, const float* yl_mean, const float* yl_invstd,
                                     const float* yl_scale, const float* yl_shift, float* stat_partial, int B, int T, int F, int Cin, int Cout,
                                     float* workspace, const float* dy_absmax) {
    if (!yl) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "conv3x3_dgrad_bnstats_scaled: yl is required"); return A2S_ERR_ARG; }
    return a2s_conv3x3_impl(ST, dy, w, g, nullptr, nullptr, stat_partial, B, T, F, Cin, Cout, 1, workspace, yl, yl_mean, yl_invstd, yl_scale, yl_shift, dy_absmax, nullptr, nullptr);
}
int a2s_conv3x3_dgrad_bnstats_ranged(void* stream, const float* dy, const float* w, float* g, const float* yl, const float* yl_mean, const float* yl_invstd,
                                     const float* yl_scale, const float* yl_shift, float* stat_partial, int B, int T, int F, int Cin, int Cout,
                                     float* workspace, const float* dy_absmax, float* g_absmax_out) {
    if (!yl) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "conv3x3_dgrad_bnstats_ranged: yl is required"); return A2S_ERR_ARG; }
    return a2s_conv3x3_impl(ST, dy, w, g, nullptr, nullptr, stat_partial, B, T, F, Cin, Cout, 1, workspace, yl, yl_mean, yl_invstd, yl_scale, yl_shift, dy_absmax, nullptr, g_absmax_out);
}
int a2s_bn_bwd_from_partial(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale, const float* shift,
                            float* dgamma, float* dbeta, float* dx, const float* partial, int nblocks, float* c12, long rows, int C, int F) {
    return a2s_bn_bwd_from_partial_impl(ST, g, x, mean, invstd, scale, shift, dgamma, dbeta, dx, partial, nblocks, c12, rows, C, F, nullptr);
}
int a2s_bn_bwd_from_partial_amax(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale, const float* shift,
                                 float* dgamma, float* dbeta, float* dx, const float* partial, int nblocks, float* c12, long rows, int C, int F,
                                 float* dx_absmax) {
    return a2s_bn_bwd_from_partial_impl(ST, g, x, mean, invstd, scale, shift, dgamma, dbeta, dx, partial, nblocks, c12, rows, C, F, dx_absmax);
}
size_t a2s_conv3x3_workspace_floats(int Cin) { return a2s_conv3x3_workspace_floats_impl(Cin); }
int a2s_conv3x3_stat_blocks(int B, int T, int F, int Cin) { return a2s_conv3x3_stat_blocks_impl(B, T, F, Cin); }
int a2s_bn_finalize(void* stream, const float* partial, int nblocks, int C, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, long long* nbt, float* mean, float* invstd, float* scale,
                    float* shift, float eps, float momentum, int training) {
    return a2s_bn_finalize_impl(ST, partial, nblocks, C, count, gamma, beta, running_mean, running_var, nbt, mean, invstd, scale,
                                shift, eps, momentum, training);
}
int a2s_bn_relu_apply(void* stream, const float* x, float* y, const float* scale, const float* shift, long n, int C, int F) {
    return a2s_bn_relu_apply_impl(ST, x, y, scale, shift, n, C, F);
}
int a2s_linear_fwd_f64(void* stream, int M, int N, int K, const float* x, const float* W, float* z, const float* scale, const float* shift, int period) {
    return a2s_linear_fwd_f64_impl(ST, M, N, K, x, W, z, scale, shift, period);
}
int a2s_col_stats_split(void* stream, const float* x, float* partial, long rows, int C, int rows_per_block) {
    return a2s_col_stats_split_impl(ST, x, partial, rows, C, rows_per_block);
}
int a2s_col_stats(void* stream, const float* x, float* partial, long rows, int C, int rows_per_block) {
    return a2s_col_stats_impl(ST, x, partial, rows, C, rows_per_block);
}
int a2s_bn1d_relu_dropout(void* stream, const float* x, float* y, const float* scale, const float* shift, const uint8_t* keep_mask,
                          float inv_keep, long n, int C) {
    return a2s_bn1d_relu_dropout_impl(ST, x, y, scale, shift, keep_mask, inv_keep, n, C);
}
int a2s_gru_gates_fwd(void* stream, const float* gi, long ldgi, const float* gh, long ldgh, const float* hprev, long ldhp,
                      float* hout, long ldho, float* hout2, long ldho2, float* save, int R, int H) {
    return a2s_gru_gates_fwd_impl(ST, gi, ldgi, gh, ldgh, hprev, ldhp, hout, ldho, hout2, ldho2, save, R, H);
}
int a2s_gru_seq_fwd(void* stream, const float* gi_all, long gi_bstride, long gi_tstride, const float* w_hh, const float* b_hh,
                    float* out, long out_bstride, long out_tstride, float* hbuf, float* gh, float* save, float* hn, int B, int T,
                    int H, int reverse, float* workspace, size_t workspace_bytes) {
    return a2s_gru_seq_fwd_impl(ST, gi_all, gi_bstride, gi_tstride, w_hh, b_hh, out, out_bstride, out_tstride, hbuf, gh, save, hn,
                                B, T, H, reverse, workspace, workspace_bytes);
}
int a2s_attn_step_fwd(void* stream, const float* keys, const float* enc, const float* q, long ldq, const float* v, float* ctx,
                      long ldctx, float* ctx2, long ldctx2, float* attw, int B, int T, int H, const int* n_done, int n_rows_total, float* workspace) {
    return a2s_attn_step_fwd_impl(ST, keys, enc, q, ldq, v, ctx, ldctx, ctx2, ldctx2, attw, B, T, H, n_done, n_rows_total, workspace, nullptr);
}
int a2s_attn_step_fwd_rows(void* stream, const float* keys, const float* enc, const float* q, long ldq, const float* v, float* ctx,
                           long ldctx, float* ctx2, long ldctx2, float* attw, int R, int T, int H, float* workspace, int n_clips,
                           const int* clip_order, const int* clip_rank, const int* row_until, int n_active, int step) {
    a2s_attn_rows rows = {clip_order, clip_rank, row_until, n_clips, n_active, step};
    return a2s_attn_step_fwd_impl(ST, keys, enc, q, ldq, v, ctx, ldctx, ctx2, ldctx2, attw, R, T, H, nullptr, 0, workspace, &rows);
}
size_t a2s_attn_workspace_floats(int B, int T, int H) { return a2s_attn_workspace_floats_impl(B, T, H, 1); }
size_t a2s_attn_workspace_floats_fused(int n_clips, int T, int H, int groups) { return a2s_attn_workspace_floats_impl(n_clips, T, H, groups); }
int a2s_log_softmax_rows(void* stream, const float* x, long ldx, float* y, long ldy, int* argmax_out, int R, int V) {
    return a2s_log_softmax_rows_impl(ST, x, ldx, y, ldy, argmax_out, R, V);
}
int a2s_embed_rows(void* stream, const float* table, const long long* ids64, const int* ids32, long id_stride, int const_id,
                   float* out, long ldo, int col0, int R, int E, const uint8_t* keep_mask, float inv_keep) {
    return a2s_embed_rows_impl(ST, table, ids64, ids32, id_stride, const_id, out, ldo, col0, R, E, keep_mask, inv_keep);
}
int a2s_note_decoder_fwd(void* stream, const a2s_note_dec_args* args, int* steps_done) {
    if (!args) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "note_decoder_fwd: null args"); return A2S_ERR_ARG; }
    return a2s_note_decoder_fwd_impl(ST, *args, steps_done);
}
int a2s_grammar_argmax_rows(void* stream, const float* x, long ldx, float* y, long ldy, const signed char* next_state, int n_states, int* row_state,
                            int* choice_out, int R, int V) {
    return a2s_grammar_argmax_rows_impl(ST, x, ldx, y, ldy, next_state, n_states, row_state, choice_out, R, V);
}
int a2s_note_decoder_fwd_grammar(void* stream, const a2s_note_dec_args* args, const signed char* next_state, int n_states, int* row_state, int* steps_done) {
    if (!args) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "note_decoder_fwd_grammar: null args"); return A2S_ERR_ARG; }
    const a2s_grammar_ref g = {next_state, n_states, row_state};
    return a2s_note_decoder_fwd_grammar_impl(ST, *args, g, steps_done);
}
int a2s_grammar_launches(void) { return a2s_grammar_launches_impl(); }
int a2s_metre_argmax_rows(void* stream, const float* x, long ldx, float* y, long ldy, const signed char* next_state, int n_states, int* row_state,
                          const int* dur_ticks, const uint8_t* cls, const uint8_t* fillable, int n_fillable, int* row_metre, int* choice_out, int R, int V) {
    const a2s_metre_ref m = {dur_ticks, cls, fillable, n_fillable, row_metre};
    return a2s_metre_argmax_rows_impl(ST, x, ldx, y, ldy, next_state, n_states, row_state, &m, choice_out, R, V);
}
int a2s_note_decoder_fwd_metre(void* stream, const a2s_note_dec_args* args, const signed char* next_state, int n_states, int* row_state,
                               const int* dur_ticks, const uint8_t* cls, const uint8_t* fillable, int n_fillable, int* row_metre, int* steps_done) {
    if (!args) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "note_decoder_fwd_metre: null args"); return A2S_ERR_ARG; }
    const a2s_grammar_ref g = {next_state, n_states, row_state};
    const a2s_metre_ref m = {dur_ticks, cls, fillable, n_fillable, row_metre};
    return a2s_note_decoder_fwd_metre_impl(ST, *args, g, &m, steps_done);
}
int a2s_metre_launches(void) { return a2s_metre_launches_impl(); }
int a2s_note_decoder_fwd_beam(void* stream, const a2s_note_dec_args* args, const a2s_beam_args* beam, int* steps_done) {
    if (!args || !beam) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "note_decoder_fwd_beam: null args"); return A2S_ERR_ARG; }
    return a2s_note_decoder_fwd_beam_impl(ST, *args, *beam, steps_done);
}
int a2s_beam_step(void* stream, const a2s_beam_args* beam, const float* logits, long ldl, const float* emb, float* xnext, long ldx, float* h, int h_cols,
                  float* q, int q_cols, int* n_done, int* steps_exec, int B, int V, int E, int t, int max_steps, int eos_id) {
    if (!beam) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "beam_step: null args"); return A2S_ERR_ARG; }
    const a2s_beam_args& g = *beam;
    const BeamStepArgs a = {logits, ldl, emb, xnext, ldx, h, h_cols, q, q_cols, g.next_state, g.n_states, g.row_state, g.score, g.finished, g.done_count,
                            g.token_hist, g.parent_hist, g.score_hist, g.probs_scratch, n_done, steps_exec, B, g.K, V, E, t, max_steps, eos_id, g.pad_id};
    return a2s_beam_step_finalize_impl(ST, a);
}
int a2s_beam_backtrack(void* stream, const a2s_beam_args* beam, float* probs, long probs_bstride, const int* steps_exec, int B, int V, int max_steps, int eos_id) {
    if (!beam) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "beam_backtrack: null args"); return A2S_ERR_ARG; }
    const a2s_beam_args& g = *beam;
    const BeamBackArgs a = {g.score, g.token_hist, g.parent_hist, g.probs_scratch, probs, probs_bstride, g.ids_out, (long)max_steps, g.lengths_out, g.score_out,
                            steps_exec, g.alpha, B, g.K, V, max_steps, eos_id, g.pad_id};
    return a2s_beam_backtrack_impl(ST, a);
}
int a2s_beam_launches(void) { return a2s_beam_launches_impl(); }
int a2s_attn_align_rows(void* stream, const float* attw, long ldw, int R, int T, int* peak_out, float* weight_out, float* centroid_out, long out_stride) {
    return a2s_attn_align_rows_impl(ST, attw, ldw, R, T, peak_out, weight_out, centroid_out, out_stride);
}
int a2s_note_decoder_fwd_align(void* stream, const a2s_note_dec_args* args, const a2s_align_args* align, int* steps_done) {
    if (!args || !align) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "note_decoder_fwd_align: null args"); return A2S_ERR_ARG; }
    return a2s_note_decoder_fwd_align_impl(ST, *args, *align, steps_done);
}
int a2s_align_launches(void) { return a2s_align_launches_impl(); }
int a2s_render_notes(void* stream, const int* programs, int rows_per_clip, int n_samples, float* wave, long wave_bstride, int B) {
    return a2s_render_notes_impl(ST, programs, rows_per_clip, n_samples, wave, wave_bstride, B);
}
int a2s_render_launches(void) { return a2s_render_launches_impl(); }
int a2s_transpose_targets(void* stream, const int* new_key, const int* interval, const int* token_map, int n_rows, int V, const int* semitones,
                          const float* detune, long long* key, long long* upper, long long* lower, int bars, int U, int L, int bins_per_semitone,
                          float* eff_bins, int* counters, int B) {
    return a2s_transpose_targets_impl(ST, new_key, interval, token_map, n_rows, V, semitones, detune, key, upper, lower, bars, U, L, bins_per_semitone, eff_bins,
                                      counters, B);
}
int a2s_shift_bins(void* stream, const float* x, float* y, const float* eff_bins, int B, int rows, int F) {
    return a2s_shift_bins_impl(ST, x, y, eff_bins, B, rows, F);
}
int a2s_augment_launches(void) { return a2s_augment_launches_impl(); }
int a2s_tempo_plan(void* stream, const float* x, int B, int rows, int F, const float* u, float R, int min_frames, int* content, int* step,
                   int* counters) {
    return a2s_tempo_plan_impl(ST, x, B, rows, F, u, R, min_frames, content, step, counters);
}
int a2s_stretch_frames(void* stream, const float* x, float* y, const int* step, int B, int rows, int F) {
    return a2s_stretch_frames_impl(ST, x, y, step, B, rows, F);
}
int a2s_tempo_launches(void) { return a2s_tempo_launches_impl(); }
int a2s_specaug_plan(void* stream, const float* x, int B, int rows, int F, const float* table, const unsigned* draws, int Wt, int Wf, int m,
                     int* content, int* plan, float* stats, int* counters) {
    return a2s_specaug_plan_impl(ST, x, B, rows, F, table, draws, Wt, Wf, m, content, plan, stats, counters);
}
int a2s_specaug_apply(void* stream, const float* x, float* y, const float* table, const int* content, const int* plan, const float* stats, int B,
                      int rows, int F) {
    return a2s_specaug_apply_impl(ST, x, y, table, content, plan, stats, B, rows, F);
}
int a2s_specaug_launches(void) { return a2s_specaug_launches_impl(); }
int a2s_room_ir(void* stream, const unsigned* room_seed, const int* params, int B, float* ir, long ir_bstride, int L_max) {
    return a2s_room_ir_impl(ST, room_seed, params, B, ir, ir_bstride, L_max);
}
int a2s_fir_rows(void* stream, const float* x, long x_bstride, const float* ir, long ir_bstride, const int* params, float* y, long y_bstride, int B,
                 int n_samples, int L_max) {
    return a2s_fir_rows_impl(ST, x, x_bstride, ir, ir_bstride, params, y, y_bstride, B, n_samples, L_max);
}
int a2s_fir_tile_samples(void) { return a2s_fir_tile_samples_impl(); }
int a2s_fir_tap_chunk(void) { return a2s_fir_tap_chunk_impl(); }
int a2s_room_launches(void) { return a2s_room_launches_impl(); }
int a2s_resample_rows(void* stream, const float* x, long x_bstride, const int* n_in, int n_in_max, int C, const float* table, int L, int M, int K, int Hh,
                      float* y, long y_bstride, int n_out_max, int B) {
    return a2s_resample_rows_impl(ST, x, x_bstride, n_in, n_in_max, C, table, L, M, K, Hh, y, y_bstride, n_out_max, B);
}
int a2s_resample_tile_samples(void) { return a2s_resample_tile_samples_impl(); }
int a2s_resample_launches(void) { return a2s_resample_launches_impl(); }

int a2s_onset_strength(void* stream, const float* x, long x_bstride, long x_rstride, const int* n_rows, int B, int rows, int F, int lag, int f_split,
                       float* env_full, float* env_low, long env_bstride) {
    return a2s_onset_strength_impl(ST, x, x_bstride, x_rstride, n_rows, B, rows, F, lag, f_split, env_full, env_low, env_bstride);
}
int a2s_tempogram(void* stream, const float* env, long stride, const int* n, int R, int J, int win, int hop_b, int lag_min, int lag_max, float* out) {
    return a2s_tempogram_impl(ST, env, stride, n, R, J, win, hop_b, lag_min, lag_max, out);
}
int a2s_beat_dp(void* stream, const float* ls, long stride, const int* period, int J, int hop_b, const float* pen, int lag_min, int lag_max, const int* n,
                int R, float* S, int* back, int* beats, int max_beats, int* count) {
    return a2s_beat_dp_impl(ST, ls, stride, period, J, hop_b, pen, lag_min, lag_max, n, R, S, back, beats, max_beats, count);
}
int a2s_beat_launches(void) { return a2s_beat_launches_impl(); }
int a2s_segment_agreement(void* stream, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* seg, int S, double* out) {
    return a2s_segment_agreement_impl(ST, x, y, clip_stride, B, T, F, seg, S, out);
}
int a2s_agreement_launches(void) { return a2s_agreement_launches_impl(); }
int a2s_agreement_partial_cells(void) { return a2s_agreement_partial_cells_impl(); }
size_t a2s_dtw_cost_bytes(int S, int n_max, int r_max) { return a2s_dtw_cost_bytes_impl(S, n_max, r_max); }
size_t a2s_dtw_workspace_bytes(int S, int n_max, int r_max) { return a2s_dtw_workspace_bytes_impl(S, n_max, r_max); }
int a2s_dtw_cost(void* stream, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* seg, int S, const float* off, int n_max,
                 int r_max, float* cost, size_t cost_bytes) {
    return a2s_dtw_cost_impl(ST, x, y, clip_stride, B, T, F, seg, S, off, n_max, r_max, cost, cost_bytes);
}
int a2s_dtw_path(void* stream, const int* seg, int S, int B, int T, int n_max, int r_max, const float* cost, size_t cost_bytes, uint8_t* ws,
                 size_t ws_bytes, int* path, int* steps, float* total) {
    return a2s_dtw_path_impl(ST, seg, S, B, T, n_max, r_max, cost, cost_bytes, ws, ws_bytes, path, steps, total);
}
int a2s_dtw_launches(void) { return a2s_dtw_launches_impl(); }
int a2s_note_levels(void* stream, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* rows, int S, double* out) {
    return a2s_note_levels_impl(ST, x, y, clip_stride, B, T, F, rows, S, out);
}
int a2s_note_amp_update(void* stream, const double* sums, const int* rows, const int* first, int B, float* cum, int* programs, int program_stride,
                        float base_amp) {
    return a2s_note_amp_update_impl(ST, sums, rows, first, B, cum, programs, program_stride, base_amp);
}
int a2s_dynamics_launches(void) { return a2s_dynamics_launches_impl(); }
int a2s_tuning_profile(void* stream, const float* x, long x_bstride, long x_rstride, const int* n_rows, int B, int rows, int F, int bins_per_semitone,
                       float thr, long long* hist) {
    return a2s_tuning_profile_impl(ST, x, x_bstride, x_rstride, n_rows, B, rows, F, bins_per_semitone, thr, hist);
}
int a2s_tuning_estimate(void* stream, const long long* hist, const int* first, int G, int B, int bins_per_semitone, double min_conf, int min_peaks,
                        double* est, float* eff_bins) {
    return a2s_tuning_estimate_impl(ST, hist, first, G, B, bins_per_semitone, min_conf, min_peaks, est, eff_bins);
}
int a2s_tuning_launches(void) { return a2s_tuning_launches_impl(); }
int a2s_path_warp(void* stream, const int* paths, long path_stride, const int* steps, const int* table, int S, int n_max, int* warp2, int* inverse2) {
    return a2s_path_warp_impl(ST, paths, path_stride, steps, table, S, n_max, warp2, inverse2);
}
int a2s_retime_events(void* stream, const int* warp2, int n_max, const int* table, int S, const int* events, int E, int hop, int* programs, int B,
                      int program_rows) {
    return a2s_retime_events_impl(ST, warp2, n_max, table, S, events, E, hop, programs, B, program_rows);
}
int a2s_retime_launches(void) { return a2s_retime_launches_impl(); }
int a2s_note_decoder_fwd_pair(void* stream_upper, void* stream_lower, const a2s_note_dec_args* upper, const a2s_note_dec_args* lower,
                              const int* pair_order, const int* pair_rank, const int* pair_n_active, int* steps_done_upper, int* steps_done_lower) {
    if (!upper || !lower) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "note_decoder_fwd_pair: null args"); return A2S_ERR_ARG; }
    return a2s_note_decoder_fwd_pair_impl((hipStream_t)stream_upper, (hipStream_t)stream_lower, *upper, *lower, pair_order, pair_rank, pair_n_active,
                                          steps_done_upper, steps_done_lower);
}
int a2s_staff_emb_fwd(void* stream, const float* note_emb, const float* const* gru_w, const long long* ids64, const int* ids32,
                      long id_bstride, const long long* lengths, long len_stride, float* out, long ldo, int col0, float* hsave,
                      int R, int maxlen, int E, int S) {
    if (!gru_w) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "staff_emb_fwd: null weight table"); return A2S_ERR_ARG; }
    return a2s_staff_emb_fwd_impl(ST, note_emb, gru_w, ids64, ids32, id_bstride, lengths, len_stride, out, ldo, col0, hsave, R,
                                  maxlen, E, S);
}

int a2s_log_softmax_bwd_rows(void* stream, const float* g, const float* y, long outer_stride, int inner, float* dx, int R, int V,
                             int n_outer, int time_major) {
    return a2s_log_softmax_bwd_rows_impl(ST, g, y, outer_stride, inner, dx, R, V, n_outer, time_major);
}
int a2s_gru_gates_bwd(void* stream, const float* dh_a, long lda, const float* dh_b, long ldb, const float* save, const float* hprev,
                      long ldhp, float* dgi, long ldgi, float* dgh, long ldgh, float* dgh2, long ldgh2, float* dhprev, long lddp, int R, int H) {
    return a2s_gru_gates_bwd_impl(ST, dh_a, lda, dh_b, ldb, save, hprev, ldhp, dgi, ldgi, dgh, ldgh, dgh2, ldgh2, dhprev, lddp, R, H);
}
int a2s_attn_step_bwd(void* stream, const float* keys, const float* enc, const float* q, long ldq, const float* v, const float* attw,
                      const float* ctx, long ldctx, const float* dctx_a, long ldda, const float* dctx_b, long lddb, float* dctx_out,
                      long lddo, float* dq, long lddq, float* ds_out, int B, int T, int H, float* workspace) {
    return a2s_attn_step_bwd_impl(ST, keys, enc, q, ldq, v, attw, ctx, ldctx, dctx_a, ldda, dctx_b, lddb, dctx_out, lddo, dq, lddq, ds_out, B, T, H, workspace, nullptr);
}
int a2s_attn_step_bwd_rows(void* stream, const float* keys, const float* enc, const float* q, long ldq, const float* v, const float* attw,
                           const float* ctx, long ldctx, const float* dctx_a, long ldda, const float* dctx_b, long lddb, float* dctx_out,
                           long lddo, float* dq, long lddq, float* ds_out, int R, int T, int H, float* workspace, int n_clips,
                           const int* clip_order, const int* clip_rank, const int* row_until, int n_active, int step) {
    a2s_attn_rows rows = {clip_order, clip_rank, row_until, n_clips, n_active, step};
    return a2s_attn_step_bwd_impl(ST, keys, enc, q, ldq, v, attw, ctx, ldctx, dctx_a, ldda, dctx_b, lddb, dctx_out, lddo, dq, lddq, ds_out, R, T, H, workspace, &rows);
}
int a2s_attn_dk_accum(void* stream, const float* keys, const float* q_all, const float* ds_all, const float* v, float* dK,
                      float* dv_partial, int B, int T, int S, int H, const int* row_until, int groups) {
    return a2s_attn_dk_accum_impl(ST, keys, q_all, ds_all, v, dK, dv_partial, B, T, S, H, row_until, groups);
}
int a2s_attn_dk_blocks(int B, int T) { return B * ((T + 15) / 16); }
int a2s_attn_denc_accum(void* stream, const float* attw_all, const float* dctx_all, float* dEnc, int B, int T, int S, int H2,
                        const int* row_until, int groups) {
    return a2s_attn_denc_accum_impl(ST, attw_all, dctx_all, dEnc, B, T, S, H2, row_until, groups);
}
int a2s_col_sum(void* stream, const float* x, long ld, float* out, long rows, int C, float alpha, float beta, float* workspace, size_t workspace_floats) {
    return a2s_col_sum_impl(ST, x, ld, out, rows, C, alpha, beta, workspace, workspace_floats);
}
int a2s_embed_scatter_add(void* stream, float* table_grad, const long long* ids64, const int* ids32, long id_stride, int const_id,
                          const float* g, long ldg, int col0, int R, int E, const uint8_t* keep_mask, float inv_keep) {
    return a2s_embed_scatter_add_impl(ST, table_grad, ids64, ids32, id_stride, const_id, g, ldg, col0, R, E, keep_mask, inv_keep);
}
int a2s_ew_act_bwd(void* stream, const float* g, const float* y, float* dx, long n, int act) { return a2s_ew_act_bwd_impl(ST, g, y, dx, n, act); }
int a2s_note_decoder_bwd(void* stream, const a2s_note_dec_bwd_args* args) {
    if (!args) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "note_decoder_bwd: null args"); return A2S_ERR_ARG; }
    return a2s_note_decoder_bwd_impl(ST, *args);
}
int a2s_note_decoder_bwd_pair(void* stream_upper, void* stream_lower, const a2s_note_dec_bwd_args* upper, const a2s_note_dec_bwd_args* lower,
                              const int* pair_order, const int* pair_rank, const int* pair_n_active) {
    if (!upper || !lower) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "note_decoder_bwd_pair: null args"); return A2S_ERR_ARG; }
    return a2s_note_decoder_bwd_pair_impl((hipStream_t)stream_upper, (hipStream_t)stream_lower, *upper, *lower, pair_order, pair_rank, pair_n_active);
}
int a2s_gru_seq_bwd(void* stream, const float* dout, long do_bstride, long do_tstride, const float* out, long out_bstride, long out_tstride,
                    const float* gates, const float* w_hh, const float* dhn, float* dgi_all, float* dgh_shift, float* dgh_first,
                    float* dhbuf, float* dgh_tmp, int B, int T, int H, int reverse, float* workspace, size_t workspace_bytes) {
    return a2s_gru_seq_bwd_impl(ST, dout, do_bstride, do_tstride, out, out_bstride, out_tstride, gates, w_hh, dhn, dgi_all, dgh_shift,
                                dgh_first, dhbuf, dgh_tmp, B, T, H, reverse, workspace, workspace_bytes, nullptr, nullptr);
}
size_t a2s_gru_workspace_bytes(int B, int H) { return a2s_gru_workspace_bytes_impl(B, H); }
int a2s_gru_seq_bwd_ranged(void* stream, const float* dout, long do_bstride, long do_tstride, const float* out, long out_bstride, long out_tstride,
                           const float* gates, const float* w_hh, const float* dhn, float* dgi_all, float* dgh_shift, float* dgh_first,
                           float* dhbuf, float* dgh_tmp, int B, int T, int H, int reverse, float* workspace, size_t workspace_bytes,
                           float* ranges_out, int* ranges_valid) {
    if (!ranges_out || !ranges_valid) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "gru_seq_bwd_ranged: null ranges_out / ranges_valid"); return A2S_ERR_ARG; }
    return a2s_gru_seq_bwd_impl(ST, dout, do_bstride, do_tstride, out, out_bstride, out_tstride, gates, w_hh, dhn, dgi_all, dgh_shift,
                                dgh_first, dhbuf, dgh_tmp, B, T, H, reverse, workspace, workspace_bytes, ranges_out, ranges_valid);
}
int a2s_staff_emb_bwd(void* stream, const float* note_emb, const float* const* gru_w, float* const* grads, float* note_emb_grad,
                      const long long* ids64, const int* ids32, long id_bstride, const long long* lengths, long len_stride,
                      const float* dout, long lddo, int col0, const float* hsave, int R, int maxlen, int E, int S) {
    if (!gru_w) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "staff_emb_bwd: null weight table"); return A2S_ERR_ARG; }
    return a2s_staff_emb_bwd_impl(ST, note_emb, gru_w, grads, note_emb_grad, ids64, ids32, id_bstride, lengths, len_stride, dout, lddo,
                                  col0, hsave, R, maxlen, E, S);
}

int a2s_bn_bwd(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale, const float* shift,
               const uint8_t* keep_mask, float inv_keep, float* dgamma, float* dbeta, float* dx, float* partial, float* c12, long rows, int C, int F) {
    return a2s_bn_bwd_impl(ST, g, x, mean, invstd, scale, shift, keep_mask, inv_keep, dgamma, dbeta, dx, partial, c12, rows, C, F, nullptr);
}
int a2s_bn_bwd_amax(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale, const float* shift,
                    const uint8_t* keep_mask, float inv_keep, float* dgamma, float* dbeta, float* dx, float* partial, float* c12, long rows, int C, int F,
                    float* dx_absmax) {
    return a2s_bn_bwd_impl(ST, g, x, mean, invstd, scale, shift, keep_mask, inv_keep, dgamma, dbeta, dx, partial, c12, rows, C, F, dx_absmax);
}
size_t a2s_bn_bwd_partial_floats(long rows, int C, int F) { return a2s_bn_bwd_partial_floats_impl(rows, C, F); }
int a2s_conv3x3_wgrad(void* stream, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dW, float* workspace,
                      size_t workspace_bytes, int B, int T, int F, int Cin, int Cout) {
    return a2s_conv3x3_wgrad_impl(ST, dy, x, in_scale, in_shift, dW, workspace, workspace_bytes, B, T, F, Cin, Cout, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr);
}
int a2s_conv3x3_wgrad_ranged(void* stream, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dW, float* workspace,
                             size_t workspace_bytes, int B, int T, int F, int Cin, int Cout, const float* dy_absmax, const float* act_absmax) {
    return a2s_conv3x3_wgrad_impl(ST, dy, x, in_scale, in_shift, dW, workspace, workspace_bytes, B, T, F, Cin, Cout, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, dy_absmax, act_absmax);
}
int a2s_act_bound(void* stream, const float* scale, const float* shift, const float* absmax, int C, float* out) {
    return a2s_act_bound_impl(ST, scale, shift, absmax, C, out);
}
int a2s_conv3x3_wgrad_scaled(void* stream, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dW, float* workspace,
                             size_t workspace_bytes, int B, int T, int F, int Cin, int Cout, const float* dy_absmax) {
    return a2s_conv3x3_wgrad_impl(ST, dy, x, in_scale, in_shift, dW, workspace, workspace_bytes, B, T, F, Cin, Cout, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, dy_absmax, nullptr);
}
int a2s_conv3x3_wgrad_bn(void* stream, const float* g, const float* y, const float* mean, const float* invstd, const float* scale, const float* shift,
                         const float* c12, float* dy_out, const float* x, const float* in_scale, const float* in_shift, float* dW, float* workspace,
                         size_t workspace_bytes, int B, int T, int F, int Cin, int Cout) {
    if (!y) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "conv3x3_wgrad_bn: y is required"); return A2S_ERR_ARG; }
    return a2s_conv3x3_wgrad_impl(ST, g, x, in_scale, in_shift, dW, workspace, workspace_bytes, B, T, F, Cin, Cout, y, mean, invstd, scale, shift, c12, dy_out, nullptr, nullptr);
}
size_t a2s_conv3x3_wgrad_workspace_bytes(int Cin, int Cout) { return a2s_conv3x3_wgrad_workspace_bytes_impl(Cin, Cout); }
int a2s_conv3x3_wgrad_bn_ranged_eligible(int F, int Cin, int Cout) { return (a2s_wgrad_rows_eligible(F, Cin, Cout) && !(Cin == 40 && Cout == 20)) ? 1 : 0; }
int a2s_conv3x3_wgrad_bn_ranged(void* stream, const float* g, const float* y, const float* mean, const float* invstd, const float* scale, const float* shift,
                                const float* c12, const float* g_absmax, int g_absmax_n, const float* y_absmax, float* dy_out, float* dy_absmax_out, const float* x,
                                const float* in_scale, const float* in_shift, float* dW, float* workspace, size_t workspace_bytes, int B, int T, int F,
                                int Cin, int Cout, const float* act_absmax) {
    if (!a2s_conv3x3_wgrad_bn_ranged_eligible(F, Cin, Cout)) { snprintf(a2s_err_msg, sizeof(a2s_err_msg), "conv3x3_wgrad_bn_ranged: shape not eligible"); return A2S_ERR_ARG; }
    return a2s_conv3x3_wgrad_rows_bn_impl(ST, g, y, mean, invstd, scale, shift, c12, g_absmax, g_absmax_n, y_absmax, dy_out, dy_absmax_out, x, in_scale, in_shift, dW,
                                          workspace, workspace_bytes, B, T, F, Cin, Cout, act_absmax);
}

int a2s_nll_grad(void* stream, float* dlogp, const long long* target, const float* loss_out, float gscale, long rows, int V, long long ignore_index) {
    return a2s_nll_grad_impl(ST, dlogp, target, loss_out, gscale, rows, V, ignore_index);
}
int a2s_nll_loss(void* stream, const float* logp, const long long* target, long rows, int V, long long ignore_index, float* loss_out,
                 float* dlogp, float gscale, double* partial, int nblocks) {
    return a2s_nll_loss_impl(ST, logp, target, rows, V, ignore_index, loss_out, dlogp, gscale, partial, nblocks);
}
int a2s_clip_adadelta(void* stream, float* params, float* grads, float* square_avg, float* acc_delta, long n, const float* loss, float max_norm,
                      float lr, float rho, float eps, float* ctl, double* partial, int nblocks, int zero_grad) {
    return a2s_clip_adadelta_impl(ST, params, grads, square_avg, acc_delta, n, loss, max_norm, lr, rho, eps, ctl, partial, nblocks, zero_grad);
}

int a2s_vqt_logmag(void* stream, const float* C, float* out, float* partial, int B, long rows, int bins, float top_db) {
    return a2s_vqt_logmag_impl(ST, C, out, partial, B, rows, bins, top_db);
}

int a2s_edit_distance(void* stream, const int* ref, const long long* ref_off, const int* hyp, const long long* hyp_off, const int* order,
                      int n_pairs, int max_ref_len, int max_hyp_len, int* dist) {
    return a2s_edit_distance_impl(ST, ref, ref_off, hyp, hyp_off, order, n_pairs, max_ref_len, max_hyp_len, dist);
}
int a2s_edit_distance_max_len(void) { return a2s_edit_distance_max_len_impl(); }

int a2s_note_match(void* stream, const int* ref, const long long* ref_off, const int* hyp, const long long* hyp_off, int n_pairs,
                   const int* dur_ticks, const int* midi, const int* cls, int V, int* out) {
    return a2s_note_match_impl(ST, ref, ref_off, hyp, hyp_off, n_pairs, dur_ticks, midi, cls, V, out);
}
int a2s_note_match_max_len(void) { return a2s_note_match_max_len_impl(); }
long a2s_note_match_launches(void) { return a2s_note_match_launches_impl(); }

int a2s_bn_bwd_stats(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale, const float* shift,
                     const uint8_t* keep_mask, float inv_keep, float* partial, float* sums, long rows, int C, int F) {
    return a2s_bn_bwd_stats_impl(ST, g, x, mean, invstd, scale, shift, keep_mask, inv_keep, partial, sums, rows, C, F);
}
int a2s_bn_bwd_apply(void* stream, const float* g, const float* x, const float* mean, const float* invstd, const float* scale, const float* shift,
                     const uint8_t* keep_mask, float inv_keep, const float* sums_local, const float* sums_global, double count_global,
                     float* dgamma, float* dbeta, float* dx, float* c12, long rows, int C, int F) {
    return a2s_bn_bwd_apply_impl(ST, g, x, mean, invstd, scale, shift, keep_mask, inv_keep, sums_local, sums_global, count_global, dgamma, dbeta,
                                 dx, c12, rows, C, F);
}
int a2s_vqt_logmag_octaves(void* stream, const float* C, float* out, float* partial, int B, long rows, int bins, int bins_per_octave, float top_db) {
    return a2s_vqt_logmag_octaves_impl(ST, C, out, partial, B, rows, bins, bins_per_octave, top_db);
}
int a2s_vqt_decimate(void* stream, const float* ypad, long padded_len, const float* taps, int ntaps, float* out, long n_out, int B) {
    return a2s_vqt_decimate_impl(ST, ypad, padded_len, taps, ntaps, out, n_out, B);
}
int a2s_bn_bwd_sums_from_partial(void* stream, const float* partial, int nblocks, int C, float* sums) {
    return a2s_bn_bwd_sums_from_partial_impl(ST, partial, nblocks, C, sums);
}
int a2s_bn_bwd_c12_from_sums(void* stream, const float* sums_local, const float* sums_global, double count_global, float* dgamma, float* dbeta,
                             float* c12, int C) {
    return a2s_bn_bwd_c12_from_sums_impl(ST, sums_local, sums_global, count_global, dgamma, dbeta, c12, C);
}

}  // extern "C"
