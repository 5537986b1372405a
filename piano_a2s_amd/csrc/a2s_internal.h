// What crosses translation units inside liba2s_hip.so: every function that one .hip file defines and another calls is declared here, once.
// Every .hip file includes this header (and through it a2s_common.h, the public include/a2s.h and the switch table a2s_switches.h).
#pragma once
#include "a2s_common.h"
#include "../../include/a2s.h"
#include "a2s_switches.h"

// ---- switches that are not a plain read of the table
// the pair loop hands over to the few-row kernels at "attn_pair_fused_rows" rows, but never above the few-row path's own limit
static inline int a2s_attn_pair_fused_rows(void) {
    const int cap = a2s_sw(A2S_SW_dec_fused_max_rows), v = a2s_sw(A2S_SW_attn_pair_fused_rows);
    return v < cap ? v : cap;
}
// the test-hook word handed to the persistent kernels (PERSIST_DBG_* bits, a2s_common.h)
static inline unsigned a2s_persist_dbg(void) {
    return (a2s_sw(A2S_SW_persist_force_agent) ? PERSIST_DBG_FORCE_AGENT : 0u) | (a2s_sw(A2S_SW_persist_inject_abort) ? PERSIST_DBG_INJECT_ABORT : 0u);
}

// ---- a2s_gemm.hip
int a2s_absmax_impl(hipStream_t st, const float* x, long n, float* out);
size_t a2s_gemm_workspace_bytes_impl(int M, int N, int batch, int splitk);
int a2s_gemm_pick_splitk_impl(int M, int N, int K, int batch);
int a2s_gemm_bnstats_slots(int period);
void a2s_gemm_debug_tile_impl(int cfg);
int a2s_gemm_affine_impl(hipStream_t st, int M, int N, int K, float alpha, const float* A, long sAm, long sAk,
    const float* B, long sBk, long sBn, float beta, float* C, long ldc, const float* bias, int act,
    int batch, long bsA, long bsB, long bsC, int splitk, float* ws, size_t ws_bytes,
    const float* a_scale, const float* a_shift, int a_period, const float* b_scale, const float* b_shift, int b_period,
    const float* ep_y, const float* ep_mean, const float* ep_invstd, const float* ep_scale, const float* ep_shift,
    float* ep_partial, int ep_period, int two_term, const float* a_absmax, const float* b_absmax);
int a2s_gemm_impl(hipStream_t st, int M, int N, int K, float alpha, const float* A, long sAm, long sAk,
    const float* B, long sBk, long sBn, float beta, float* C, long ldc, const float* bias, int act,
    int batch, long bsA, long bsB, long bsC, int splitk, float* ws, size_t ws_bytes);

// ---- a2s_linear.hip
size_t a2s_linear_dgrad_ws_bytes_impl(int N, int K);
int a2s_linear_dgrad_blocks_impl(int M);
bool a2s_linear_dgrad_ok(int M, int N, int K, long lda, long sBk, long sBn, long ldc, int period, const void* A, const void* B, const void* C, const void* y);
int a2s_linear_dgrad_bnstats_impl(hipStream_t st, int M, int N, int K, const float* A, long lda, const float* Wt, long sBk, long sBn, float* C, long ldc,
    const float* ep_y, const float* mean, const float* invstd, const float* scale, const float* shift, int period,
    float* partial, const float* a_absmax, const float* b_absmax, float* ws, size_t ws_bytes, float* c_absmax_out);
bool a2s_linear_fwd_ok(int M, int N, int K, long lda, long ldc, int period, const void* A, const void* W, const void* C);
int a2s_linear_fwd_impl(hipStream_t st, int M, int N, int K, const float* A, long lda, const float* W, float* C, long ldc, const float* a_scale,
    const float* a_shift, int period, const float* a_absmax, const float* w_absmax, float* ws, size_t ws_bytes);
int a2s_linear_fwd_f64_impl(hipStream_t st, int M, int N, int K, const float* x, const float* W, float* z, const float* scale, const float* shift, int period);
size_t a2s_linear_wgrad_ws_bytes_impl(int M, int K);
bool a2s_linear_wgrad_ok(int M, int N, int K, long ldz, long lda, long ldg, int period, const void* dz, const void* A, const void* G);
int a2s_linear_wgrad_impl(hipStream_t st, int M, int N, int K, const float* dz, long ldz, const float* A, long lda, float* G, long ldg, const float* a_scale,
    const float* a_shift, int period, const float* dz_absmax, const float* a_absmax, float* ws, size_t ws_bytes);
extern int a2s_tallk_wgrad_on;                      // the key "tallk_wgrad" beside the switch list (a2s_switches.h)
extern int a2s_tallk_wgrad_max_splits;              // "tallk_wgrad_max_splits" (test aid)
long a2s_tallk_wgrad_launches(void);
size_t a2s_tallk_wgrad_ws_bytes_impl(int M, int Np, int K);
bool a2s_tallk_wgrad_ok(int M, int Np, int K, long ldp, long lda, long ldg, int transposed, const void* P, const void* A, const void* G, const void* bias);
int a2s_tallk_wgrad_impl(hipStream_t st, int M, int Np, int K, const float* P, long ldp, const float* A, long lda, float* G, long ldg, int transposed,
    float* bias, const float* p_absmax, const float* a_absmax, float* ws, size_t ws_bytes);

// ---- a2s_conv.hip
// tile of the fp32-input kernels (forward / data gradient and weight gradient): rows x columns per workgroup, input channels per LDS chunk
#define CV_TR 4
#define CV_FT 32
#define CV_CK 20
// trace builds (-DC4_TRACE, tools/conv_trace.py): workgroups x stages of 8 stamps each, in a buffer per file (a2s_conv_trace_read, a2s_conv_wgrad_trace_read)
#define C4_TRACE_WGS 8
#define C4_TRACE_STAGES 24
int a2s_act_bound_impl(hipStream_t st, const float* scale, const float* shift, const float* absmax, int C, float* out);
size_t a2s_conv3x3_workspace_floats_impl(int Cin);
int a2s_conv3x3_impl(hipStream_t st, const float* x, const float* w, float* y, const float* in_scale,
    const float* in_shift, float* stat_partial, int B, int T, int F, int Cin, int Cout, int flip, float* ws,
    const float* yl, const float* yl_mean, const float* yl_invstd, const float* yl_scale, const float* yl_shift,
    const float* x_absmax, const float* in_absmax, float* out_absmax);
int a2s_conv3x3_stat_blocks_impl(int B, int T, int F, int Cin);

// ---- a2s_conv_wgrad.hip
size_t a2s_conv3x3_wgrad_workspace_bytes_impl(int Cin, int Cout);
int a2s_conv3x3_wgrad_impl(hipStream_t st, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dW,
    float* ws, size_t ws_bytes, int B, int T, int F, int Cin, int Cout, const float* bn_y, const float* bn_mean,
    const float* bn_invstd, const float* bn_scale, const float* bn_shift, const float* bn_c12, float* dy_out,
    const float* dy_absmax, const float* act_absmax);

// ---- a2s_bn.hip
int a2s_bn_finalize_impl(hipStream_t st, const float* partial, int nblocks, int C, double count, const float* gamma,
    const float* beta, float* running_mean, float* running_var, long long* nbt, float* mean,
    float* invstd, float* scale, float* shift, float eps, float momentum, int training);
int a2s_bn_relu_apply_impl(hipStream_t st, const float* x, float* y, const float* scale, const float* shift, long n, int C, int F);
int a2s_col_stats_impl(hipStream_t st, const float* x, float* partial, long rows, int C, int rows_per_block);
int a2s_col_stats_split_impl(hipStream_t st, const float* x, float* partial, long rows, int C, int rows_per_block);
int a2s_bn1d_relu_dropout_impl(hipStream_t st, const float* x, float* y, const float* scale, const float* shift,
    const uint8_t* mask, float inv_keep, long n, int C);
int a2s_bn_bwd_impl(hipStream_t st, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
    const float* shift, const uint8_t* mask, float inv_keep, float* dgamma, float* dbeta, float* dx, float* partial,
    float* c12, long rows, int C, int F, float* dx_absmax);
int a2s_bn_bwd_from_partial_impl(hipStream_t st, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
    const float* shift, float* dgamma, float* dbeta, float* dx, const float* partial, int nblocks, float* c12,
    long rows, int C, int F, float* dx_absmax);
int a2s_bn_bwd_stats_impl(hipStream_t st, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
    const float* shift, const uint8_t* mask, float inv_keep, float* partial, float* sums, long rows, int C, int F);
int a2s_bn_bwd_apply_impl(hipStream_t st, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
    const float* shift, const uint8_t* mask, float inv_keep, const float* sums_local, const float* sums_global,
    double count_global, float* dgamma, float* dbeta, float* dx, float* c12, long rows, int C, int F);
int a2s_bn_bwd_sums_from_partial_impl(hipStream_t st, const float* partial, int nblocks, int C, float* sums);
int a2s_bn_bwd_c12_from_sums_impl(hipStream_t st, const float* sums_local, const float* sums_global, double count_global, float* dgamma, float* dbeta,
    float* c12, int C);
size_t a2s_bn_bwd_partial_floats_impl(long rows, int C, int F);
void a2s_absmax_small_launch(hipStream_t st, const float* w, int n, float* out);     // one workgroup; for a2s_conv3x3_impl, see the note at the kernel

// ---- a2s_conv_rows.hip
int a2s_channel_absmax_impl(hipStream_t st, const float* x, long rows, int C, int F, float* out);
bool a2s_conv_rows_eligible(int F, int Cin);
int a2s_conv_rows_blocks(int B, int T, int F);
size_t a2s_conv_rows_workspace_floats(int Cin);
long a2s_conv_rows16_c20_launches(void);
extern int a2s_conv_rows_stage;                     // the key "conv_rows_stage" beside the switch list (a2s_switches.h)
long a2s_conv_rows_stage_launches(void);
int a2s_conv3x3_rows_impl(hipStream_t st, const float* x, const float* w, float* y, const float* in_scale, const float* in_shift,
    const float* in_absmax, float* stat_partial, float* out_absmax, int B, int T, int F, int Cin, int Cout, int flip,
    float* ws, const float* yl, const float* yl_mean, const float* yl_invstd, const float* yl_scale, const float* yl_shift,
    const float* x_absmax);

// ---- a2s_conv_wrows.hip
bool a2s_wgrad_rows_eligible(int F, int Cin, int Cout);
int a2s_conv3x3_wgrad_rows_bn_impl(hipStream_t st, const float* g, const float* y, const float* mean, const float* invstd, const float* scale,
    const float* shift, const float* c12, const float* g_absmax, int g_absmax_n, const float* y_absmax, float* dz_out,
    float* dz_absmax_out, const float* x, const float* in_scale, const float* in_shift, float* dW, float* ws, size_t ws_bytes,
    int B, int T, int F, int Cin, int Cout, const float* act_absmax);
int a2s_conv3x3_wgrad_rows_impl(hipStream_t st, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dW, float* ws,
    size_t ws_bytes, int B, int T, int F, int Cin, int Cout, const float* dy_absmax, const float* act_absmax);

// ---- a2s_seq.hip
// argument block of the step epilogue (note_step_finalize; grammar_step_finalize of a2s_grammar.hip)
struct StepFinArgs {
    const float* logits; long ldl;        // (R, V)
    float* probs; long probs_bstride;     // row b, step t at probs + b*probs_bstride + t*V
    const long long* gt; long gt_bstride; // ground-truth ids (row b at gt + b*gt_bstride), null in inference
    const float* emb;                     // (V, E) embedding table
    float* xnext; long ldx;               // next GRU input rows; token embedding -> columns [0, E)
    const uint8_t* drop; float inv_keep;  // (R, E) keep mask for the NEXT token or null
    int* argmax_out; long am_bstride;     // ids[b*am_bstride + t] (int32) or null
    int* eos_seen; long long* lengths; int* n_done; int* steps_exec;
    const int* t_base;                    // graph replay: step index = t + *t_base (null: t)
    const int* row_until;                 // training: rows finished at this step (t >= row_until[row]) keep their outputs untouched
    int n_clips;                          // rows per group (fused bars); teacher_force bit g applies to the rows of group g
    int R, V, E, t, teacher_force, eos_id, max_t;
};
// a token grammar for the greedy decoder: next[s * V + v] = state after token v in state s, negative where v is illegal; one state per row
struct a2s_grammar_ref { const signed char* next; int n_states; int* row_state; };
// the metre on top of it (members as include/a2s.h documents them): tables per token id, and 16 ints per row
struct a2s_metre_ref { const int* dur_ticks; const uint8_t* cls; const uint8_t* fillable; int n_fillable; int* row_metre; };
int a2s_gru_gates_fwd_impl(hipStream_t st, const float* gi, long ldgi, const float* gh, long ldgh, const float* hprev,
    long ldhp, float* hout, long ldho, float* hout2, long ldho2, float* save, int R, int H);
int a2s_gru_bptt_step_impl(hipStream_t st, const float* dgh, const float* w_hh_t, const float* dhz_in, const float* dout, long ld_dout,
    const float* save, const float* hprev, long ld_hprev, float* dgi, long ld_dgi, float* dgh_out, float* dgh2,
    long ld_dgh2, float* dhz_out, int R, int H);
int a2s_skinny_gemm_acc_impl(hipStream_t st, const float* A, long lda, const float* Bt, long ldb, float* Cm, long ldc, int R, int N, int K);
long a2s_gru_step_fwd_launches(void);
long a2s_gru_step_bwd_launches(void);
int a2s_gru_seq_fwd_impl(hipStream_t st, const float* gi_all, long gi_bstride, long gi_tstride, const float* w_hh,
    const float* b_hh, float* out, long out_bstride, long out_tstride, float* hbuf, float* gh,
    float* save, float* hn, int B, int T, int H, int reverse, float* ws, size_t ws_bytes);
int a2s_attn_step_fwd_impl(hipStream_t st, const float* Kmat, const float* enc, const float* q, long ldq, const float* v,
    float* ctx, long ldctx, float* ctx2, long ldctx2, float* attw, int B, int T, int H,
    const int* n_done, int n_rows_total, float* ws, const a2s_attn_rows* rows = nullptr, a2s_attn_deferred* defer = nullptr);
int a2s_log_softmax_rows_impl(hipStream_t st, const float* x, long ldx, float* y, long ldy, int* argmax_out, int R, int V);
int a2s_embed_rows_impl(hipStream_t st, const float* table, const long long* ids64, const int* ids32, long id_stride,
    int const_id, float* out, long ldo, int col0, int R, int E, const uint8_t* drop, float inv_keep);
int a2s_note_decoder_fwd_impl(hipStream_t st, const a2s_note_dec_args& a, int* steps_done);
int a2s_note_decoder_fwd_grammar_impl(hipStream_t st, const a2s_note_dec_args& a, const a2s_grammar_ref& g, int* steps_done);
int a2s_note_decoder_fwd_metre_impl(hipStream_t st, const a2s_note_dec_args& a, const a2s_grammar_ref& g, const a2s_metre_ref* mt, int* steps_done);
int a2s_note_decoder_fwd_pair_impl(hipStream_t su, hipStream_t sl, const a2s_note_dec_args& au, const a2s_note_dec_args& al, const int* pair_order,
    const int* pair_rank, const int* pair_n_active, int* done_u, int* done_l);
int a2s_staff_emb_fwd_impl(hipStream_t st, const float* note_emb, const float* const* w /* 8 GRU tensors f then r */,
    const long long* ids64, const int* ids32, long id_bstride, const long long* lengths,
    long len_stride, float* out, long ldo, int col0, float* hsave, int R, int maxlen, int E, int S);
int a2s_note_decoder_zero_unwritten(hipStream_t st, const a2s_note_dec_args& a, const char* who /* in the error message */);
size_t a2s_attn_workspace_floats_impl(int B, int T, int H, int groups);
size_t a2s_attn_bulk_lds(size_t shm, int n_active, int backward);
long a2s_attn_pair_launches(void);
// the pair loops (forward here, reverse in a2s_bwd.hip) launch both staves' sweeps of a step at once.  AttnPairStep: the pair's clip bookkeeping at
// one step and the geometry its partials use (the sweep sets G and chunk, the staves' combines read them)
struct AttnPairStep { const int* clip_order; const int* clip_rank; int n_clips; int n_active; int step; int G; int chunk; };
int a2s_pair_events(const char* who, hipEvent_t** ev_out);       // -> the issuing thread's two events on the current device
// what stream `from` has been given so far, stream `to` waits for
static inline int a2s_record_wait(hipEvent_t ev, hipStream_t from, hipStream_t to, const char* who) {
    hipError_t e = hipEventRecord(ev, from);
    if (e == hipSuccess) e = hipStreamWaitEvent(to, ev, 0);
    if (e != hipSuccess) A2S_FAIL(A2S_ERR_HIP, "%s: event: %s", who, hipGetErrorString(e));
    return A2S_OK;
}

// ---- a2s_bwd.hip
int a2s_log_softmax_bwd_rows_impl(hipStream_t st, const float* g, const float* y, long outer_stride, int inner, float* dx,
    int R, int V, int n_outer, int time_major);
int a2s_gru_gates_bwd_impl(hipStream_t st, const float* dh_a, long lda, const float* dh_b, long ldb, const float* save,
    const float* hprev, long ldhp, float* dgi, long ldgi, float* dgh, long ldgh, float* dgh2, long ldgh2,
    float* dhprev, long lddp, int R, int H);
int a2s_attn_step_bwd_impl(hipStream_t st, const float* Kmat, const float* enc, const float* q, long ldq, const float* v,
    const float* attw, const float* ctx, long ldctx, const float* dctx_a, long ldda, const float* dctx_b,
    long lddb, float* dctx_out, long lddo, float* dq, long lddq, float* ds_out, int B, int T, int H, float* ws,
    const a2s_attn_rows* rows = nullptr);
int a2s_attn_dk_accum_impl(hipStream_t st, const float* Kmat, const float* q_all, const float* ds_all, const float* v,
    float* dK, float* dv_partial, int B, int T, int S, int H, const int* row_until, int groups);
int a2s_attn_denc_accum_impl(hipStream_t st, const float* attw_all, const float* dctx_all, float* dEnc, int B, int T, int S, int H2,
    const int* row_until, int groups);
long a2s_attn_dk_ahead_launches(void);
long a2s_attn_denc_launches(void);
int a2s_col_sum_impl(hipStream_t st, const float* x, long ld, float* out, long rows, int C, float alpha, float beta, float* ws, size_t ws_floats);
int a2s_embed_scatter_add_impl(hipStream_t st, float* table_grad, const long long* ids64, const int* ids32, long id_stride,
    int const_id, const float* g, long ldg, int col0, int R, int E, const uint8_t* drop, float inv_keep);
int a2s_ew_act_bwd_impl(hipStream_t st, const float* g, const float* y, float* dx, long n, int act);
int a2s_note_decoder_bwd_impl(hipStream_t st, const a2s_note_dec_bwd_args& a);
int a2s_note_decoder_bwd_pair_impl(hipStream_t su, hipStream_t sl, const a2s_note_dec_bwd_args& au, const a2s_note_dec_bwd_args& al, const int* pair_order,
    const int* pair_rank, const int* pair_n_active);
int a2s_gru_seq_bwd_impl(hipStream_t st, const float* dout, long do_bstride, long do_tstride, const float* out, long out_bstride,
    long out_tstride, const float* gates, const float* w_hh, const float* dhn, float* dgi_all, float* dgh_shift,
    float* dgh_first, float* dhbuf, float* dgh_tmp, int B, int T, int H, int reverse, float* ws, size_t ws_bytes,
    float* ranges_out, int* ranges_valid);
int a2s_staff_emb_bwd_impl(hipStream_t st, const float* note_emb, const float* const* w, float* const* grads_dev, float* note_emb_grad,
    const long long* ids64, const int* ids32, long id_bstride, const long long* lengths, long len_stride,
    const float* dout, long lddo, int col0, const float* hsave, int R, int maxlen, int E, int S);
size_t a2s_gru_workspace_bytes_impl(int B, int H);
long a2s_attn_pair_bwd_launches(void);

// ---- a2s_step.hip
size_t a2s_note_step_fused_head_floats(void);
size_t a2s_note_step_workspace_floats_impl(int H, int E);
int a2s_dec_mid_launches(void);
int a2s_dec_cmb_launches(void);
bool a2s_dec_step_fusable(int R, int H, int E, int V, const void* const* ptrs, int nptrs, const float* ws, size_t ws_floats, bool greedy = false);
int a2s_note_step_fused_fwd(hipStream_t st, const a2s_note_dec_args& a, int si, int so, int sv, int sv_next, int t, const int* t_base, int tf, bool last,
    int nrows, const int* rowmap, const a2s_attn_deferred* defer = nullptr);
int a2s_note_step_fused_bwd_prepare(hipStream_t st, const a2s_note_dec_bwd_args& a);
int a2s_note_step_fused_bwd(hipStream_t st, const a2s_note_dec_bwd_args& a, int s, const float* dh_in, float* dh_out, const a2s_attn_rows* rows,
    int nrows, const int* rowmap);
bool a2s_note_step_mid_ok(int H, int E, const void* const* ptrs, int nptrs);
int a2s_note_step_mid_gru(hipStream_t st, const a2s_note_dec_args& a, int si, int so, int sv, int sv_next, int nrows, const int* rowmap);
bool a2s_note_step_mid_bwd_ok(const a2s_note_dec_bwd_args& a);
int a2s_note_step_mid_bwd(hipStream_t st, const a2s_note_dec_bwd_args& a, int s, float* dh_out, int nrows, const int* rowmap);
int a2s_note_step_mid_bwd_query(hipStream_t st, const a2s_note_dec_bwd_args& a, int s, float* dh_out, int nrows, const int* rowmap);

// ---- a2s_grammar.hip
bool a2s_grammar_ref_ok(const a2s_grammar_ref& g, int R, int V);
int a2s_grammar_argmax_rows_impl(hipStream_t st, const float* x, long ldx, float* y, long ldy, const signed char* next, int n_states, int* row_state,
    int* choice_out, int R, int V);
int a2s_grammar_step_finalize_impl(hipStream_t st, const StepFinArgs& a, const a2s_grammar_ref& g);
int a2s_grammar_launches_impl(void);
bool a2s_metre_ref_ok(const a2s_metre_ref& m);
int a2s_metre_argmax_rows_impl(hipStream_t st, const float* x, long ldx, float* y, long ldy, const signed char* next, int n_states, int* row_state,
    const a2s_metre_ref* mt, int* choice_out, int R, int V);
int a2s_metre_step_finalize_impl(hipStream_t st, const StepFinArgs& a, const a2s_grammar_ref& g, const a2s_metre_ref& mt);
int a2s_metre_launches_impl(void);

// ---- a2s_align.hip
// n_done / n_rows_total (the decode loop's greedy calls, else null / 0): the launch is a no-op once every row has shown <eos>, as the step's attention
int a2s_attn_align_rows_impl(hipStream_t st, const float* attw, long ldw, int R, int T, int* peak_out, float* weight_out, float* centroid_out,
    long out_stride, const int* n_done = nullptr, int n_rows_total = 0);
int a2s_align_launches_impl(void);
int a2s_note_decoder_fwd_align_impl(hipStream_t st, const a2s_note_dec_args& a, const a2s_align_args& g, int* steps_done);

// ---- a2s_render.hip
int a2s_render_notes_impl(hipStream_t st, const int* programs, int rows_per_clip, int n_samples, float* wave, long wave_bstride, int B);
int a2s_render_launches_impl(void);

// ---- a2s_augment.hip
int a2s_transpose_targets_impl(hipStream_t st, const int* new_key, const int* interval, const int* token_map, int n_rows, int V, const int* semitones,
    const float* detune, long long* key, long long* upper, long long* lower, int bars, int U, int L, int bins_per_semitone, float* eff_bins, int* counters,
    int B);
int a2s_shift_bins_impl(hipStream_t st, const float* x, float* y, const float* eff_bins, int B, int rows, int F);
int a2s_augment_launches_impl(void);

// ---- the tile frame of the row-streaming augmentation kernels (shift_bins, stretch_frames, specaug_apply): a workgroup of (A2S_ROW_TX, A2S_ROW_TY)
// threads works on A2S_ROW_TILE consecutive rows of one clip, threadIdx.y on A2S_ROW_NR of them; a thread moves VEC floats at once, four where
// F % 4 == 0 and y is 16-byte aligned, else one.
#define A2S_ROW_TX 128
#define A2S_ROW_TY 2
#define A2S_ROW_TILE 16
#define A2S_ROW_NR (A2S_ROW_TILE / A2S_ROW_TY)
#ifdef __HIPCC__
template <int VEC> struct a2s_row_vec { typedef float type; };
template <> struct a2s_row_vec<4> { typedef f32x4 type; };
static inline int a2s_row_vec_width(int F, const void* y) { return (F % 4 == 0 && ((uintptr_t)y & 15) == 0) ? 4 : 1; }
// the grid (row tiles, B, column tiles) of a kernel whose threads each own `vec` columns and do not loop over them; false where F has more column tiles
// than a grid's z extent
static inline bool a2s_row_grid(int B, int rows, int F, int vec, dim3* grid) {
    *grid = dim3(a2s_cdiv(rows, A2S_ROW_TILE), B, a2s_cdiv(F, A2S_ROW_TX * vec));
    return grid->z <= 65535;
}
// kernel<4> or kernel<1>, as `vec` says, on the frame's block
#define A2S_ROW_LAUNCH(kernel, vec, grid, st, ...)                                                                   \
    do {                                                                                                             \
        if ((vec) == 4) hipLaunchKernelGGL(kernel<4>, grid, dim3(A2S_ROW_TX, A2S_ROW_TY), 0, st, __VA_ARGS__);       \
        else hipLaunchKernelGGL(kernel<1>, grid, dim3(A2S_ROW_TX, A2S_ROW_TY), 0, st, __VA_ARGS__);                  \
    } while (0)
#endif

// ---- a2s_tempo.hip
int a2s_tempo_plan_impl(hipStream_t st, const float* x, int B, int rows, int F, const float* u, float R, int min_frames, int* content, int* step,
    int* counters);
int a2s_stretch_frames_impl(hipStream_t st, const float* x, float* y, const int* step, int B, int rows, int F);
int a2s_tempo_launches_impl(void);

// the backward content scan of tempo_plan and specaug_plan, one workgroup of THREADS threads per clip xb (rows, F): 1 + the last row that holds a value
// != 0 (true for a NaN, false for -0.0), 0 for an all-zero clip, the same in every thread.  Chunks of A2S_CONTENT_CHUNK rows from the last row backwards,
// up to the first chunk with content.  Loads at [0, rows * F) of xb only; s_last is one int of the caller's LDS.
#define A2S_CONTENT_CHUNK 16
#ifdef __HIPCC__
template <int THREADS>
__device__ __forceinline__ int a2s_content_rows(const float* __restrict__ xb, int rows, int F, int* s_last) {
    const int tid = threadIdx.x;
    for (int r1 = rows; r1 > 0; r1 -= A2S_CONTENT_CHUNK) {
        const int r0 = r1 > A2S_CONTENT_CHUNK ? r1 - A2S_CONTENT_CHUNK : 0;
        const float* xc = xb + (long)r0 * F;
        const long len = (long)(r1 - r0) * F;
        long last = -1;
#pragma unroll 4
        for (long i = tid; i < len; i += THREADS)
            if (xc[i] != 0.0f) last = i;          // (true for a NaN, false for -0.0)
        if (tid == 0) *s_last = -1;
        __syncthreads();
        if (last >= 0) atomicMax(s_last, (int)(last / F));
        __syncthreads();
        const int got = *s_last;
        __syncthreads();                          // (thread 0 resets s_last in the next chunk)
        if (got >= 0) return r0 + got + 1;
    }
    return 0;
}
#endif

// ---- a2s_specaug.hip
int a2s_specaug_plan_impl(hipStream_t st, const float* x, int B, int rows, int F, const float* table, const unsigned* draws, int Wt, int Wf, int m,
    int* content, int* plan, float* stats, int* counters);
int a2s_specaug_apply_impl(hipStream_t st, const float* x, float* y, const float* table, const int* content, const int* plan, const float* stats, int B,
    int rows, int F);
int a2s_specaug_launches_impl(void);

// ---- a2s_room.hip
int a2s_room_ir_impl(hipStream_t st, const unsigned* room_seed, const int* params, int B, float* ir, long ir_bstride, int L_max);
int a2s_fir_rows_impl(hipStream_t st, const float* x, long x_bstride, const float* ir, long ir_bstride, const int* params, float* y, long y_bstride, int B,
                      int n_samples, int L_max);
int a2s_fir_tile_samples_impl(void);
int a2s_fir_tap_chunk_impl(void);
int a2s_room_launches_impl(void);

// ---- a2s_resample.hip
int a2s_resample_rows_impl(hipStream_t st, const float* x, long x_bstride, const int* n_in, int n_in_max, int C, const float* table, int L, int M, int K,
                           int Hh, float* y, long y_bstride, int n_out_max, int B);
int a2s_resample_tile_samples_impl(void);
int a2s_resample_launches_impl(void);

// ---- a2s_beat.hip
int a2s_onset_strength_impl(hipStream_t st, const float* x, long x_bstride, long x_rstride, const int* n_rows, int B, int rows, int F, int lag, int f_split,
                            float* env_full, float* env_low, long env_bstride);
int a2s_tempogram_impl(hipStream_t st, const float* env, long stride, const int* n, int R, int J, int win, int hop_b, int lag_min, int lag_max, float* out);
int a2s_beat_dp_impl(hipStream_t st, const float* ls, long stride, const int* period, int J, int hop_b, const float* pen, int lag_min, int lag_max,
                     const int* n, int R, float* S, int* back, int* beats, int max_beats, int* count);
int a2s_beat_launches_impl(void);

// ---- a2s_agree.hip
int a2s_segment_agreement_impl(hipStream_t st, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* seg, int S, double* out);
int a2s_agreement_launches_impl(void);
int a2s_agreement_partial_cells_impl(void);

// ---- a2s_dtw.hip
size_t a2s_dtw_cost_bytes_impl(int S, int n_max, int r_max);
size_t a2s_dtw_workspace_bytes_impl(int S, int n_max, int r_max);
int a2s_dtw_cost_impl(hipStream_t st, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* seg, int S, const float* off,
                      int n_max, int r_max, float* cost, size_t cost_bytes);
int a2s_dtw_path_impl(hipStream_t st, const int* seg, int S, int B, int T, int n_max, int r_max, const float* cost, size_t cost_bytes, unsigned char* ws,
                      size_t ws_bytes, int* path, int* steps, float* total);
int a2s_dtw_launches_impl(void);

// ---- a2s_dynamics.hip
int a2s_note_levels_impl(hipStream_t st, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* rows, int S, double* out);
int a2s_note_amp_update_impl(hipStream_t st, const double* sums, const int* rows, const int* first, int B, float* cum, int* programs, int rows_per_clip,
                             float base_amp);
int a2s_dynamics_launches_impl(void);

// ---- a2s_tuning.hip
int a2s_tuning_profile_impl(hipStream_t st, const float* x, long x_bstride, long x_rstride, const int* n_rows, int B, int rows, int F,
                            int bins_per_semitone, float thr, long long* hist);
int a2s_tuning_estimate_impl(hipStream_t st, const long long* hist, const int* first, int G, int B, int bins_per_semitone, double min_conf, int min_peaks,
                             double* est, float* eff_bins);
int a2s_tuning_launches_impl(void);

// ---- a2s_retime.hip
int a2s_path_warp_impl(hipStream_t st, const int* paths, long path_stride, const int* steps, const int* table, int S, int n_max, int* warp2, int* inverse2);
int a2s_retime_events_impl(hipStream_t st, const int* warp2, int n_max, const int* table, int S, const int* events, int E, int hop, int* programs, int B,
                           int program_rows);
int a2s_retime_launches_impl(void);

// ---- a2s_beam.hip
// argument block of the beam step epilogue (beam_step_finalize): rows = K slots x B clips, row = slot * B + clip
struct BeamStepArgs {
    const float* logits; long ldl;        // (K * B, V)
    const float* emb;                     // (V, E) embedding table
    float* xnext; long ldx;               // next GRU input rows; token embedding -> columns [0, E)
    float* h; int h_cols;                 // what the next step reads of this one per row, permuted in place: the state rows ...
    float* q; int q_cols;                 // ... and the next step's query rows where the step kernels have left them behind (or null)
    const signed char* next; int n_states; int* row_state;     // the grammar (a2s_grammar_ref), next null: none
    float* score; int* finished; int* done_count;
    int* token_hist; int* parent_hist; float* score_hist;      // (max_t, K * B)
    float* probs_scratch;                 // (K * B, max_t, V)
    int* n_done; int* steps_exec;
    int B, K, V, E, t, max_t, eos_id, pad_id;
};
struct BeamBackArgs {
    const float* score; const int* token_hist; const int* parent_hist; const float* probs_scratch;
    float* probs; long probs_bstride;     // clip b, step t at probs + b * probs_bstride + t * V
    int* ids_out; long ids_bstride; long long* lengths_out; float* score_out;
    const int* steps_exec;                // device: steps executed (null: max_t)
    float alpha;
    int B, K, V, max_t, eos_id, pad_id;
};
bool a2s_beam_args_ok(const a2s_beam_args& g, int R, int n_clips, int V);
int a2s_beam_init_impl(hipStream_t st, const a2s_beam_args& g, int* n_done, int B, int steps);
int a2s_beam_step_finalize_impl(hipStream_t st, const BeamStepArgs& a);
int a2s_beam_backtrack_impl(hipStream_t st, const BeamBackArgs& a);
int a2s_beam_launches_impl(void);
int a2s_note_decoder_fwd_beam_impl(hipStream_t st, const a2s_note_dec_args& a, const a2s_beam_args& g, int* steps_done);

// ---- a2s_persist.hip
unsigned* a2s_persist_latch_ptr(void);
void a2s_persist_latch_set(void* p);
a2s_device_geom a2s_device_geometry(void);
size_t a2s_gru_persist_ws_bytes_impl(int B, int H, int bwd);       // granule buffers + header of one persistent launch; 0: shape not supported
long a2s_gru_persist_fwd_launches(void);
long a2s_gru_persist_bwd_launches(void);
bool a2s_gru_seq_fwd_persist_ok(const float* w_hh, const float* gi, int B, int T, int H, float* ws, size_t ws_bytes);
int a2s_gru_seq_fwd_persist_impl(hipStream_t st, const float* gi_all, long gi_bstride, long gi_tstride, const float* w_hh, const float* b_hh, float* out,
    long out_bstride, long out_tstride, float* save, float* hn, int B, int T, int H, int reverse, float* ws, size_t ws_bytes);
bool a2s_gru_seq_bwd_persist_ok(int B, int T, int H, float* ws, size_t ws_bytes, size_t ws_used);
int a2s_gru_seq_bwd_persist_impl(hipStream_t st, const float* dout, long do_bstride, long do_tstride, const float* out, long out_bstride, long out_tstride,
    const float* gates, const float* w_hh_t, const float* dhn, float* dgi_all, float* dgh_shift, float* dgh_first, int B, int T,
    int H, int reverse, float* ws, size_t ws_off, size_t ws_bytes, float* ranges_out);

// ---- a2s_dec_persist.hip
int a2s_dec_persist_launches(void);
bool a2s_note_decoder_fwd_persist_ok(const a2s_note_dec_args& a);
int a2s_note_decoder_fwd_persist(hipStream_t st, const a2s_note_dec_args& a, int* steps_done);
bool a2s_note_decoder_bwd_persist_ok(const a2s_note_dec_bwd_args& a);
int a2s_note_decoder_bwd_persist(hipStream_t st, const a2s_note_dec_bwd_args& a);

// ---- a2s_opt.hip
int a2s_nll_loss_impl(hipStream_t st, const float* logp, const long long* target, long rows, int V, long long ignore_index,
    float* loss_out /* 2 floats */, float* dlogp /* zero-filled or null */, float gscale, double* partial, int nblocks);
int a2s_nll_grad_impl(hipStream_t st, float* dlogp, const long long* target, const float* loss_out, float gscale, long rows, int V, long long ignore_index);
int a2s_clip_adadelta_impl(hipStream_t st, float* params, float* grads, float* square_avg, float* acc_delta, long n, const float* loss,
    float max_norm, float lr, float rho, float eps, float* ctl /* 3 floats */, double* partial, int nblocks, int zero_grad);

// ---- a2s_metrics.hip
int a2s_edit_distance_max_len_impl(void);
long a2s_edit_distance_launches(void);
int a2s_edit_distance_impl(hipStream_t st, const int* ref, const long long* ref_off, const int* hyp, const long long* hyp_off, const int* order,
    int n_pairs, int max_ref_len, int max_hyp_len, int* dist);

// ---- a2s_notes.hip
int a2s_note_match_max_len_impl(void);
long a2s_note_match_launches_impl(void);
int a2s_note_match_impl(hipStream_t st, const int* ref, const long long* ref_off, const int* hyp, const long long* hyp_off, int n_pairs,
    const int* dur_ticks, const int* midi, const int* cls, int V, int* out);

// ---- a2s_vqt.hip
int a2s_vqt_logmag_impl(hipStream_t st, const float* C, float* out, float* partial, int B, long rows, int bins, float top_db);
int a2s_vqt_decimate_impl(hipStream_t st, const float* ypad, long plen, const float* taps, int ntaps, float* out, long n_out, int B);
int a2s_vqt_logmag_octaves_impl(hipStream_t st, const float* C, float* out, float* partial, int B, long rows, int bins, int bpo, float top_db);
