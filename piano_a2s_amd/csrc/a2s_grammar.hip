// Grammar-constrained greedy choice: the step epilogue of the note decoder when every decoded bar has to be a
// well-formed **kern token sequence, and its stand-alone sibling for one batch of logits rows.
//
// The language is regular: a row carries ONE automaton state s, and the host table next[s][v] (n_states x V signed bytes,
// piano_a2s_amd/kern_grammar.py) gives the state after token v, or a negative value where v is illegal in s.  The step emits
//     argmax { x[v] : next[s][v] >= 0 }      (lowest index on ties, as the unconstrained epilogue)
// and moves the row to next[s][v].  The log-probabilities it writes stay the model's UNCONSTRAINED log_softmax(x): the meaning of the
// output tensors does not depend on the mode; the emitted ids go to argmax_out.  Nothing here knows a token class or the <eos> state:
// "after <eos> only <pad>" is a row of the table, and with a table of one all-legal state the kernel is note_step_finalize bit for bit
// (same per-lane order of the maximum, the exp sum and the wave reductions).
//
// One wave per row, four rows per 256-thread workgroup, no LDS: lane l holds logits l, l + 64, ... (NK = ceil(V / 64) of them) and the
// matching bytes of next[s] in registers; both arg-maxima are one butterfly each.
//
// The metre is a per-token predicate on top of the table: grammar_row takes it as a parameter, the syntax kernels pass the
// predicate that allows everything, metre_argmax_rows / metre_step_finalize one built from the row's 16 metre ints.
#include "a2s_internal.h"

#define GR_NONE 0x7fffffff        // "no candidate yet" index of the arg-maxima
#define GR_MAX_V 256              // NK <= 4

static long long gr_launches = 0;       // step epilogues launched (a2s_grammar_launches: the tests' proof of the path)

struct GrChoice { int id; int state; bool legal; };    // legal: a legal token existed (else id is the unconstrained argmax, the state kept)

// the predicate of the syntax kernels: the table alone decides.  fetch(j): what the predicate reads per token, loaded beside the logit and the table
// byte (not behind them); operator()(j, fetched): may token j be emitted
struct GrAny {
    struct Tok {};
    __device__ __forceinline__ Tok fetch(int) const { return {}; }
    __device__ __forceinline__ bool operator()(int, Tok) const { return true; }
};

// lg: the row's V logits.  y: where its log-probabilities go, or null.  Returns (every lane) the emitted token and the row's new state.
// A row whose state has no legal token -- no table made by kern_grammar.py has one -- emits the unconstrained argmax and keeps its state;
// a state outside [0, n_states) is read as the nearest valid one: nothing is ever indexed out of bounds.
// pred: may token j be emitted beyond what the table says?  (fetch sees an index below V; the answer counts only where the table allows j)
template <int NK, class Pred = GrAny>
__device__ __forceinline__ GrChoice grammar_row(const float* __restrict__ lg, int V, const signed char* __restrict__ next, int n_states, int state,
                                                float* __restrict__ y, int lane, const Pred& pred = Pred()) {
    const int s = min(max(state, 0), n_states - 1);
    const signed char* nrow = next + (long)s * V;
    float v[NK];
    float m = -INFINITY, gm = -INFINITY;
    int mi = GR_NONE, gi = GR_NONE;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int j = lane + 64 * k;
        const bool in = j < V;
        v[k] = in ? lg[j] : -INFINITY;
        const auto tok = pred.fetch(in ? j : 0);
        const bool legal = in && nrow[j] >= 0 && pred(j, tok);
        if (v[k] > m) { m = v[k]; mi = j; }
        if (legal && (gi == GR_NONE || v[k] > gm)) { gm = v[k]; gi = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64); const int oi = __shfl_xor(mi, o, 64);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
        const float ogm = __shfl_xor(gm, o, 64); const int ogi = __shfl_xor(gi, o, 64);
        if (ogi != GR_NONE && (gi == GR_NONE || ogm > gm || (ogm == gm && ogi < gi))) { gm = ogm; gi = ogi; }
    }
    if (y) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) if (lane + 64 * k < V) sum += expf(v[k] - m);
        sum = wave_sum(sum);
        const float lse = m + logf(sum);
#pragma unroll
        for (int k = 0; k < NK; ++k) if (lane + 64 * k < V) y[lane + 64 * k] = v[k] - lse;
    }
    GrChoice c;
    if (gi != GR_NONE) { c.id = gi; c.state = nrow[gi]; c.legal = true; }
    else { c.id = mi != GR_NONE ? mi : 0; c.state = s; c.legal = false; }
    return c;
}

// ---- the constrained sibling of log_softmax_rows
template <int NK>
__global__ __launch_bounds__(256) void grammar_argmax_rows(const float* __restrict__ x, long ldx, float* __restrict__ y, long ldy,
                                                           const signed char* __restrict__ next, int n_states, int* __restrict__ row_state,
                                                           int* __restrict__ choice_out, int R, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const GrChoice c = grammar_row<NK>(x + (long)row * ldx, V, next, n_states, row_state[row], y ? y + (long)row * ldy : nullptr, lane);
    if (lane == 0) {
        row_state[row] = c.state;
        if (choice_out) choice_out[row] = c.id;
    }
}

// ---- the step epilogue: note_step_finalize (a2s_seq.hip) with the constrained choice in the place of its argmax
template <int NK>
__global__ __launch_bounds__(256) void grammar_step_finalize(StepFinArgs a, a2s_grammar_ref g) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.R) return;
    if (*a.n_done >= a.R) return;                               // every row has shown <eos>: the step is a no-op
    const int t = a.t + (a.t_base ? *a.t_base : 0);
    if (t >= a.max_t) return;                                   // a replayed chunk may overshoot the step budget
    const bool finished = a.row_until && t >= a.row_until[row];
    float* pr = a.probs + (long)row * a.probs_bstride + (long)t * a.V;
    const GrChoice c = grammar_row<NK>(a.logits + (long)row * a.ldl, a.V, g.next, g.n_states, g.row_state[row], finished ? nullptr : pr, lane);
    for (int j = lane; j < a.E; j += 64) a.xnext[(long)row * a.ldx + j] = a.emb[(long)c.id * a.E + j];
    if (lane == 0 && !finished) {
        if (row == 0 && a.steps_exec) *a.steps_exec = t + 1;      // steps run in order on one stream
        if (a.argmax_out) a.argmax_out[(long)row * a.am_bstride + t] = c.id;
        g.row_state[row] = c.state;
        if (c.id == a.eos_id) {
            if (!a.eos_seen[row]) { a.eos_seen[row] = 1; atomicAdd(a.n_done, 1); }
            a.lengths[row] = t + 1;
        }
    }
}


// ---- the metre.  A row's 16 ints (layout: include/a2s.h, a2s_metre_ref) are wave-uniform: every lane loads them once and
// derives the same few flags; only a lane that holds a DUR token in a row where a note may start reads `fillable`, at an index checked against its
// length.  No value read from memory is an index without a clamp: field -> 0 .. 7, the spine count -> 1 .. 8, a token id is below V.
static long long mt_launches = 0;       // metre step epilogues launched (a2s_metre_launches)

struct MetreRow {
    const int* dur; const unsigned char* cls; const unsigned char* fillable; int n_fillable;
    bool on, need_note, in_chord, tab_ok, nl_ok, eos_ok, first_line;
    int L, t, n_fields, field, field_dur, rem, m;

    __device__ __forceinline__ MetreRow(const a2s_metre_ref& g, const int* __restrict__ st)
        : dur(g.dur_ticks), cls(g.cls), fillable(g.fillable), n_fillable(g.n_fillable) {
        L = st[A2S_METRE_L]; t = st[A2S_METRE_T]; first_line = st[A2S_METRE_FIRST] != 0; n_fields = st[A2S_METRE_NFIELDS];
        field = min(max(st[A2S_METRE_FIELD], 0), A2S_METRE_FIELDS - 1); in_chord = st[A2S_METRE_CHORD] != 0; field_dur = st[A2S_METRE_FDUR];
        on = L > 0;
        const int n = min(max(first_line ? field + 1 : n_fields, 1), A2S_METRE_FIELDS);
        int end_f = 0, end_0 = 0;
        m = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < A2S_METRE_FIELDS; ++j) {
            const int e = st[A2S_METRE_END + j];
            if (j < n) m = min(m, e);
            if (j == field) end_f = e;
            if (j == 0) end_0 = e;
        }
        need_note = end_f == t;
        rem = L - t;
        const bool complete = first_line || field == n_fields - 1;
        tab_ok = first_line ? field < A2S_METRE_FIELDS - 1 : field < n_fields - 1;
        nl_ok = complete && m < L;
        eos_ok = (first_line && field == 0 && end_0 == 0) || (complete && m == L);       // the empty bar, or every spine at L
    }
    // class and ticks of token j: their addresses depend on nothing the row holds, so the loads go out with the logit's; only the `fillable`
    // byte of a duration that may start here waits for the row's state
    struct Tok { int cls, dur; };
    __device__ __forceinline__ Tok fetch(int j) const { return {cls[j], dur[j]}; }
    __device__ __forceinline__ bool operator()(int, Tok k) const {
        if (!on) return true;
        switch (k.cls) {
            case A2S_METRE_CLS_NULL: return !need_note;
            case A2S_METRE_CLS_OPEN: return in_chord || need_note;
            case A2S_METRE_CLS_DUR: {
                if (in_chord) return k.dur == field_dur;
                const int r = rem - k.dur;
                return need_note && r >= 0 && r < n_fillable && fillable[r] != 0;
            }
            case A2S_METRE_CLS_TAB: return tab_ok;
            case A2S_METRE_CLS_NL: return nl_ok;
            case A2S_METRE_CLS_EOS: return eos_ok;
            default: return true;
        }
    }
    // one lane: the row's metre ints after it has emitted the legal token `id` (< V)
    __device__ __forceinline__ void advance(int* __restrict__ st, int id) const {
        if (!on) return;
        switch (cls[id]) {
            case A2S_METRE_CLS_DUR: if (!in_chord) { const int d = dur[id]; st[A2S_METRE_END + field] = t + d; st[A2S_METRE_FDUR] = d; } break;
            case A2S_METRE_CLS_SP: st[A2S_METRE_CHORD] = 1; break;
            case A2S_METRE_CLS_TAB: st[A2S_METRE_FIELD] = min(field + 1, A2S_METRE_FIELDS - 1); st[A2S_METRE_CHORD] = 0; break;
            case A2S_METRE_CLS_NL:
                st[A2S_METRE_T] = m;
                if (first_line) { st[A2S_METRE_NFIELDS] = field + 1; st[A2S_METRE_FIRST] = 0; }
                st[A2S_METRE_FIELD] = 0; st[A2S_METRE_CHORD] = 0;
                break;
            default: break;
        }
    }
};

template <int NK>
__global__ __launch_bounds__(256) void metre_argmax_rows(const float* __restrict__ x, long ldx, float* __restrict__ y, long ldy,
                                                         const signed char* __restrict__ next, int n_states, int* __restrict__ row_state, a2s_metre_ref mt,
                                                         int* __restrict__ choice_out, int R, int V) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    int* ms = mt.row_metre + (long)row * A2S_METRE_INTS;
    const MetreRow pred(mt, ms);
    const GrChoice c = grammar_row<NK>(x + (long)row * ldx, V, next, n_states, row_state[row], y ? y + (long)row * ldy : nullptr, lane, pred);
    if (lane == 0) {
        row_state[row] = c.state;
        if (c.legal) pred.advance(ms, c.id);
        if (choice_out) choice_out[row] = c.id;
    }
}

// ---- grammar_step_finalize with the metre predicate
template <int NK>
__global__ __launch_bounds__(256) void metre_step_finalize(StepFinArgs a, a2s_grammar_ref g, a2s_metre_ref mt) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= a.R) return;
    if (*a.n_done >= a.R) return;
    const int t = a.t + (a.t_base ? *a.t_base : 0);
    if (t >= a.max_t) return;
    const bool finished = a.row_until && t >= a.row_until[row];
    float* pr = a.probs + (long)row * a.probs_bstride + (long)t * a.V;
    int* ms = mt.row_metre + (long)row * A2S_METRE_INTS;
    const MetreRow pred(mt, ms);
    const GrChoice c = grammar_row<NK>(a.logits + (long)row * a.ldl, a.V, g.next, g.n_states, g.row_state[row], finished ? nullptr : pr, lane, pred);
    for (int j = lane; j < a.E; j += 64) a.xnext[(long)row * a.ldx + j] = a.emb[(long)c.id * a.E + j];
    if (lane == 0 && !finished) {
        if (row == 0 && a.steps_exec) *a.steps_exec = t + 1;
        if (a.argmax_out) a.argmax_out[(long)row * a.am_bstride + t] = c.id;
        g.row_state[row] = c.state;
        if (c.legal) pred.advance(ms, c.id);
        if (c.id == a.eos_id) {
            if (!a.eos_seen[row]) { a.eos_seen[row] = 1; atomicAdd(a.n_done, 1); }
            a.lengths[row] = t + 1;
        }
    }
}

static bool grammar_shape_ok(const signed char* next, int n_states, const int* row_state, int R, int V) {
    return next && row_state && n_states >= 1 && n_states <= 127 && R >= 0 && V >= 1 && V <= GR_MAX_V;
}

int a2s_grammar_argmax_rows_impl(hipStream_t st, const float* x, long ldx, float* y, long ldy, const signed char* next, int n_states, int* row_state,
                                 int* choice_out, int R, int V) {
    A2S_REQUIRE(grammar_shape_ok(next, n_states, row_state, R, V), "grammar_argmax_rows: needs a table of 1..127 states, row states, 1 <= V <= %d (got %d states, V = %d, R = %d)",
                GR_MAX_V, n_states, V, R);
    A2S_REQUIRE(x && ldx >= V && (!y || ldy >= V), "grammar_argmax_rows: null logits or a row stride below V");
    if (R == 0) return A2S_OK;
#define A2S_GR_ROWS(NK) hipLaunchKernelGGL(grammar_argmax_rows<NK>, dim3(a2s_cdiv(R, 4)), dim3(256), 0, st, x, ldx, y, ldy, next, n_states, row_state, choice_out, R, V)
    switch ((V + 63) / 64) {
        case 1: A2S_GR_ROWS(1); break;
        case 2: A2S_GR_ROWS(2); break;
        case 3: A2S_GR_ROWS(3); break;
        default: A2S_GR_ROWS(4); break;
    }
#undef A2S_GR_ROWS
    A2S_CHECK_LAUNCH("grammar_argmax_rows");
    return A2S_OK;
}

bool a2s_grammar_ref_ok(const a2s_grammar_ref& g, int R, int V) { return grammar_shape_ok(g.next, g.n_states, g.row_state, R, V); }

int a2s_grammar_step_finalize_impl(hipStream_t st, const StepFinArgs& a, const a2s_grammar_ref& g) {
#define A2S_GR_STEP(NK) hipLaunchKernelGGL(grammar_step_finalize<NK>, dim3(a2s_cdiv(a.R, 4)), dim3(256), 0, st, a, g)
    switch ((a.V + 63) / 64) {
        case 1: A2S_GR_STEP(1); break;
        case 2: A2S_GR_STEP(2); break;
        case 3: A2S_GR_STEP(3); break;
        default: A2S_GR_STEP(4); break;
    }
#undef A2S_GR_STEP
    A2S_CHECK_LAUNCH("grammar_step_finalize");
    __atomic_fetch_add(&gr_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_grammar_launches_impl(void) { return (int)__atomic_load_n(&gr_launches, __ATOMIC_RELAXED); }

bool a2s_metre_ref_ok(const a2s_metre_ref& m) { return m.dur_ticks && m.cls && m.fillable && m.n_fillable >= 1 && m.row_metre; }

int a2s_metre_argmax_rows_impl(hipStream_t st, const float* x, long ldx, float* y, long ldy, const signed char* next, int n_states, int* row_state,
                               const a2s_metre_ref* mt, int* choice_out, int R, int V) {
    A2S_REQUIRE(grammar_shape_ok(next, n_states, row_state, R, V), "metre_argmax_rows: needs a table of 1..127 states, row states, 1 <= V <= %d (got %d states, V = %d, R = %d)",
                GR_MAX_V, n_states, V, R);
    A2S_REQUIRE(mt && a2s_metre_ref_ok(*mt), "metre_argmax_rows: needs the duration, class and fillable tables and the rows' metre states");
    A2S_REQUIRE(x && ldx >= V && (!y || ldy >= V), "metre_argmax_rows: null logits or a row stride below V");
    if (R == 0) return A2S_OK;
#define A2S_MT_ROWS(NK) hipLaunchKernelGGL(metre_argmax_rows<NK>, dim3(a2s_cdiv(R, 4)), dim3(256), 0, st, x, ldx, y, ldy, next, n_states, row_state, *mt, choice_out, R, V)
    switch ((V + 63) / 64) {
        case 1: A2S_MT_ROWS(1); break;
        case 2: A2S_MT_ROWS(2); break;
        case 3: A2S_MT_ROWS(3); break;
        default: A2S_MT_ROWS(4); break;
    }
#undef A2S_MT_ROWS
    A2S_CHECK_LAUNCH("metre_argmax_rows");
    return A2S_OK;
}

int a2s_metre_step_finalize_impl(hipStream_t st, const StepFinArgs& a, const a2s_grammar_ref& g, const a2s_metre_ref& mt) {
#define A2S_MT_STEP(NK) hipLaunchKernelGGL(metre_step_finalize<NK>, dim3(a2s_cdiv(a.R, 4)), dim3(256), 0, st, a, g, mt)
    switch ((a.V + 63) / 64) {
        case 1: A2S_MT_STEP(1); break;
        case 2: A2S_MT_STEP(2); break;
        case 3: A2S_MT_STEP(3); break;
        default: A2S_MT_STEP(4); break;
    }
#undef A2S_MT_STEP
    A2S_CHECK_LAUNCH("metre_step_finalize");
    __atomic_fetch_add(&mt_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_metre_launches_impl(void) { return (int)__atomic_load_n(&mt_launches, __ATOMIC_RELAXED); }
