// The run-time switches of liba2s_hip.so: ONE list.  From it come the ids, the storage (one int array), a2s_debug_set / a2s_debug_get for these
// keys and the environment overlay; the kernels' launchers read a switch with a2s_sw(A2S_SW_<key>).  INTEGRATION.md ("Process-wide switches")
// documents the same keys in the same order (tests/test_switches_cpu.py keeps the two in step).
//
//   X(key, default, how a written value is stored, environment variable that overrides the default or 0)
//     ONOFF   0 stays 0, everything else is 1.   Environment: off exactly when the text starts with '0'.
//     COUNT   a number or bit mask >= 0; a negative value is stored as 0 (these keys once kept -1 for "not read yet").   Environment: decimal.
//     RAW     stored as written.
// The switches are plain ints, written by the host thread that drives the step and read by the threads that enqueue: no locks, no atomics.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define A2S_SWITCHES(X)                                                                                                                              \
    /* ConvStack: bit 0 the row-streaming kernels of a2s_conv_rows.hip, bit 1 their second generation (conv3x3_rows16) where it exists              \
       (Cout 20, 40), bits 2 / 3 its form with two accumulator sets for the forward / data-gradient launches; 0 = the tiled kernels of a2s_conv.hip */ \
    X(conv_rows, 7, COUNT, "A2S_CONV_ROWS")                                                                                                          \
    /* the weight gradient on the row-streaming kernels of a2s_conv_wrows.hip (0: the tiled ones of a2s_conv_wgrad.hip) */                           \
    X(wgrad_rows, 1, COUNT, "A2S_WGRAD_ROWS")                                                                                                        \
    /* the first layer's compile-time-shaped kernels (conv3x3_c1_fixed, conv3x3_wgrad_c1_stream); 0 = the generic ones (tests: bit-equal) */         \
    X(conv_c1_fast, 1, RAW, 0)                                                                                                                       \
    /* convolutions on the bf16 matrix pipes with 3-term split operands (conv3x3_split<.., 3>): bit 0 forward, bit 1 data-gradient launches */       \
    X(conv_bf16x3, 3, RAW, 0)                                                                                                                        \
    /* ... and of those, which use the TWO-term fp16 split instead (conv3x3_split<.., 2>: three products instead of six) */                          \
    X(conv_f16x2, 3, COUNT, 0)                                                                                                                       \
    /* conv3x3_wgrad_split for the plain weight-gradient launches: 1 = where it is faster, 2 = every eligible launch */                              \
    X(wgrad_bf16x3, 1, RAW, 0)                                                                                                                       \
    /* ... with two fp16 terms (needs the max |dy| scalar) instead of three bf16 terms */                                                            \
    X(wgrad_f16x2, 1, COUNT, 0)                                                                                                                      \
    /* GEMM: 128x128 launches with two k-contiguous operands on the bf16 matrix pipes with 3-term split operands */                                  \
    X(gemm_bf16x3, 1, RAW, 0)                                                                                                                        \
    /* ... two fp16 terms instead where the caller vouches for the operands' ranges (a2s_gemm_f32_affine_scaled) */                                  \
    X(gemm_f16x2, 1, COUNT, 0)                                                                                                                       \
    /* encoder GRU: one launch per step (0: the three-launch step, A/B measurements) */                                                              \
    X(gru_fused, 1, ONOFF, 0)                                                                                                                        \
    /* encoder GRU: the persistent recurrences of a2s_persist.hip (0: the launch-per-step kernels) */                                                \
    X(gru_persist, 1, ONOFF, "A2S_GRU_PERSIST")                                                                                                      \
    /* the host runs the two directions of a layer one after the other: a persistent launch may then fill the chip alone */                          \
    X(gru_persist_alone, 0, ONOFF, 0)                                                                                                                \
    /* staff embedding: the E = 16, S = 32 kernels (0: the generic ones) */                                                                          \
    X(staff_emb_fast, 1, ONOFF, 0)                                                                                                                   \
    /* note decoder: the few-row fused step of a2s_step.hip ... */                                                                                   \
    X(dec_fused, 1, ONOFF, "A2S_DEC_FUSED")                                                                                                          \
    /* ... for training calls of at most this many rows ... */                                                                                       \
    X(dec_fused_max_rows, 192, COUNT, 0)                                                                                                             \
    /* ... and inside the pair loop from this many rows on; READS BACK as min(stored, dec_fused_max_rows) (a2s_attn_pair_fused_rows) */              \
    X(attn_pair_fused_rows, 32, RAW, 0)                                                                                                              \
    /* note decoder: the mid-size kernels (dec_gru_mid, dec_bwd_mid) for launches over more than 160 rows */                                         \
    X(dec_mid, 1, ONOFF, 0)                                                                                                                          \
    /* note decoder: the persistent few-clip decoder of a2s_dec_persist.hip (0: the launch-per-step kernels) */                                      \
    X(dec_persist, 1, ONOFF, "A2S_DEC_PERSIST")                                                                                                      \
    /* attention: both staves' sweeps of a decode step in one launch (0: every staff sweeps on its own) */                                           \
    X(attn_pair, 1, ONOFF, 0)                                                                                                                        \
    /* attention: training launches over at most this many active clips use the one-round-trip forward sweep */                                      \
    X(attn_deep, 24, COUNT, 0)                                                                                                                       \
    /* attention: the combine of the few-clip training launches folded into the GRU step */                                                          \
    X(attn_defer_combine, 1, ONOFF, 0)                                                                                                               \
    /* attention: the last-arriving workgroup merges the partials: 0 never, 1 always, n >= 2 launches over at most n clips (slower: a2s_seq.hip) */  \
    X(attn_fused_combine, 0, COUNT, 0)                                                                                                               \
    /* attention: launches covering at least this many clips stream K / enc with non-temporal loads (0: off) */                                      \
    X(attn_nt, 64, COUNT, 0)                                                                                                                         \
    /* attention: occupancy cap of the bulk launches (a2s_attn_bulk_lds); the host switches it on while another clip group decodes beside */         \
    X(attn_bulk_cap, 0, ONOFF, 0)                                                                                                                    \
    /* persistent kernels, test hooks (bits of a2s_persist_dbg()): never take the plain-store (one-XCD) hand-off ... */                              \
    X(persist_force_agent, 0, ONOFF, 0)                                                                                                              \
    /* ... every persistent launch behaves as if a wait had timed out */                                                                             \
    X(persist_inject_abort, 0, ONOFF, 0)
// Not in the list, because they are not stored integers (a2s_debug_set / a2s_debug_get, a2s_api.hip): "gemm_tile" is write-only
// (a2s_gemm_debug_tile); the "*_launches" counters and "device_cus" / "device_xccs" are read-only.
// Three keys are kept beside the list, because the list is a recorded contract (tests/test_switches_cpu.py spells its keys out):
// "attn_deferred_fast" (default 1; a2s_attn_deferred_fast, a2s_bwd.hip) -- the deferred attention gradients on attn_dk_accum_ahead and
// attn_denc_accum; 0 = attn_dk_accum and the batched GEMM.  No environment variable.
// "tallk_wgrad" (default 1; a2s_tallk_wgrad_on, a2s_linear.hip) -- the encoder GRU's weight gradients and the attention key products on
// a2s_tallk_wgrad (a2s_tallk_wgrad_eligible answers 0 while it is off); 0 = the generic split-K GEMM and the column-sum passes.  No environment variable.
// Its test aid "tallk_wgrad_max_splits" (default 0 = no cap) bounds the kernel's split over the rows, so that a small shape runs long row ranges.
// "conv_rows_stage" (bits, default 3; a2s_conv_rows_stage, a2s_conv_rows.hip) -- bit 0: conv3x3_rows16 stages its input rows with the narrow-group waves
// alone (the instances of rows16_stage_narrow; bit-identical results); 0 = every thread stages.  Bit 1 (with bit 0): the 40 -> 40 data gradient with two
// accumulator sets.  "conv_rows_stage_launches" counts the narrow-staging launches (read-only).  No environment variable.

enum a2s_switch {
#define X(key, def, rule, env) A2S_SW_##key,
    A2S_SWITCHES(X)
#undef X
    A2S_SW_COUNT
};
extern int a2s_switch_value[A2S_SW_COUNT];          // constant-initialised with the defaults; the environment is applied before main()
static inline int a2s_sw(a2s_switch id) { return a2s_switch_value[id]; }

extern int a2s_attn_deferred_fast;                  // the key beside the list (above)

int a2s_switch_find(const char* key);               // id, or -1
void a2s_switch_store(int id, int value);           // applies the key's storage rule
const char* a2s_switch_env_error(void);             // "NAME=text" of the first variable of the list whose text was not a decimal number, or NULL

#ifdef A2S_SWITCHES_IMPL                            // defined by exactly one translation unit (a2s_api.hip)
enum { A2S_RULE_ONOFF, A2S_RULE_COUNT, A2S_RULE_RAW };
struct a2s_switch_desc { const char* key; int rule; const char* env; };
static const a2s_switch_desc a2s_switch_table[A2S_SW_COUNT] = {
#define X(key, def, rule, env) {#key, A2S_RULE_##rule, env},
    A2S_SWITCHES(X)
#undef X
};
int a2s_switch_value[A2S_SW_COUNT] = {
#define X(key, def, rule, env) def,
    A2S_SWITCHES(X)
#undef X
};
static char a2s_switch_bad_env[96] = {0};

int a2s_switch_find(const char* key) {
    for (int i = 0; key && i < A2S_SW_COUNT; ++i)
        if (!strcmp(key, a2s_switch_table[i].key)) return i;
    return -1;
}
void a2s_switch_store(int id, int value) {
    const int rule = a2s_switch_table[id].rule;
    a2s_switch_value[id] = rule == A2S_RULE_ONOFF ? (value ? 1 : 0) : (rule == A2S_RULE_COUNT && value < 0) ? 0 : value;
}
const char* a2s_switch_env_error(void) { return a2s_switch_bad_env[0] ? a2s_switch_bad_env : nullptr; }

// Read once per process, when the library is loaded and before the static initialisers of the other files: a later a2s_debug_set wins.
__attribute__((constructor(101))) static void a2s_switch_read_env(void) {
    for (int i = 0; i < A2S_SW_COUNT; ++i) {
        const char* e = a2s_switch_table[i].env ? getenv(a2s_switch_table[i].env) : nullptr;
        if (!e || !*e) continue;
        if (a2s_switch_table[i].rule == A2S_RULE_ONOFF) { a2s_switch_value[i] = e[0] == '0' ? 0 : 1; continue; }
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (*end || v < 0 || v > 0x7fffffff) {
            if (!a2s_switch_bad_env[0]) snprintf(a2s_switch_bad_env, sizeof(a2s_switch_bad_env), "%s=%s", a2s_switch_table[i].env, e);
            continue;
        }
        a2s_switch_value[i] = (int)v;
    }
}
#endif
