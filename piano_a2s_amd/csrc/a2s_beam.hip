// Beam search over the note sequences of one (bar, staff) call: the step epilogue of the note decoder when a clip
// carries K <= 4 hypotheses, and the kernel that picks and unrolls the winner behind the loop.
//
// Rows are the fused-bars layout: row = slot * B + clip, so the K rows of a clip share one pass over its key image and encoder rows in the
// attention kernels.  beam_step_finalize is note_step_finalize for such a call: per row the unconstrained log_softmax (same per-lane order of
// the maximum, the exp sum and m + logf(s)); a candidate (slot k, token v) scores score[k] + lp[v] (one fp32 add), -inf where the grammar's
// table forbids v in the slot's state; a finished slot has the single candidate (k, <pad>) at its own score.  The new beam is the K best
// candidates of the clip, ties to the lowest flat index k * V + v, stored best first.  The slot then takes over its parent's recurrent state:
// the h rows (and the next step's query rows, where the step kernels have left them behind) of a clip are permuted in place.
//
// One 256-thread workgroup per clip, wave k = slot k.  Lane l holds logits l, l + 64, ... (NK = ceil(V / 64)).  A wave extracts its own K best
// by K (value, index) butterflies and publishes them to LDS; behind one barrier wave 0 merges the <= K * K candidates.
#include "a2s_internal.h"

#define BM_NONE 0x7fffffff        // "no candidate" index
#define BM_MAX_V 256              // NK <= 4
#define BM_MAX_K A2S_BEAM_MAX

static long long bm_launches = 0;       // step epilogues launched (a2s_beam_launches: the tests' proof of the path)

// (value, index) order of the selection: larger value first, lower index on ties; BM_NONE never wins
__device__ __forceinline__ bool bm_better(float v, int i, float bv, int bi) { return i != BM_NONE && (bi == BM_NONE || v > bv || (v == bv && i < bi)); }

__device__ __forceinline__ void bm_wave_best(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(i, o, 64);
        if (bm_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

template <int NK>
__global__ __launch_bounds__(256) void beam_step_finalize(BeamStepArgs a) {
    __shared__ float c_val[BM_MAX_K][BM_MAX_K];
    __shared__ int c_idx[BM_MAX_K][BM_MAX_K];
    __shared__ float s_score[BM_MAX_K];
    __shared__ int s_tok[BM_MAX_K], s_par[BM_MAX_K], s_state[BM_MAX_K], s_fin[BM_MAX_K];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int B = a.B, K = a.K, R = K * B, V = a.V, t = a.t;
    if (b >= B) return;
    // every workgroup of the launch reads the count the PREVIOUS step left behind: the step is a no-op for all of them or for none
    if (t < 0 || t >= a.max_t) return;
    if (a.done_count[t] >= R) {                                 // every slot of every clip is finished: so they are before the next step
        if (tid == 0) atomicAdd(a.done_count + t + 1, K);
        return;
    }
    if (wave < K) {
        const int row = wave * B + b;
        const float score = a.score[row];
        const bool fin = a.finished[row] != 0;
        const float* lg = a.logits + (long)row * a.ldl;
        const signed char* nrow = a.next ? a.next + (long)min(max(a.row_state[row], 0), a.n_states - 1) * V : nullptr;
        float v[NK];
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int j = lane + 64 * k;
            v[k] = j < V ? lg[j] : -INFINITY;
            if (v[k] > m) m = v[k];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const float om = __shfl_xor(m, o, 64); if (om > m) m = om; }
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) if (lane + 64 * k < V) sum += expf(v[k] - m);
        sum = wave_sum(sum);
        const float lse = m + logf(sum);
        float* pr = a.probs_scratch + ((long)row * a.max_t + t) * V;
        bool open[NK];                                          // candidate (wave, j) exists and has not been extracted yet
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int j = lane + 64 * k;
            const float lp = v[k] - lse;
            if (j < V) pr[j] = lp;                              // the model's UNCONSTRAINED log-probabilities
            open[k] = j < V && (fin ? j == a.pad_id : true);
            const bool legal = !nrow || (j < V && nrow[j] >= 0);
            v[k] = fin ? score : (legal ? score + lp : -INFINITY);
        }
        for (int r = 0; r < K; ++r) {
            float bv = -INFINITY; int bi = BM_NONE;
#pragma unroll
            for (int k = 0; k < NK; ++k) if (open[k] && bm_better(v[k], lane + 64 * k, bv, bi)) { bv = v[k]; bi = lane + 64 * k; }
            bm_wave_best(bv, bi);
#pragma unroll
            for (int k = 0; k < NK; ++k) if (bi == lane + 64 * k) open[k] = false;
            if (lane == 0) { c_val[wave][r] = bv; c_idx[wave][r] = bi; }
        }
    }
    __syncthreads();
    if (wave == 0) {
        // lane l < 16: candidate r = l & 3 of slot l >> 2
        const int ck = lane >> 2, cr = lane & 3;
        const bool have = lane < BM_MAX_K * BM_MAX_K && ck < K && cr < K && c_idx[ck][cr] != BM_NONE;
        const float cv = have ? c_val[ck][cr] : -INFINITY;
        const int cf = have ? ck * V + c_idx[ck][cr] : BM_NONE;
        bool open = have;
        int old_cnt = 0, new_cnt = 0;
        for (int k = 0; k < K; ++k) old_cnt += a.finished[k * B + b] != 0;
        for (int j = 0; j < K; ++j) {
            float bv = open ? cv : -INFINITY; int bi = open ? cf : BM_NONE;
            bm_wave_best(bv, bi);
            if (bi == cf) open = false;
            // (every slot has at least one candidate, so K of them always exist; the guard only keeps a corrupt call inside its buffers)
            const int par = bi != BM_NONE ? bi / V : j, tok = bi != BM_NONE ? bi % V : a.pad_id;
            const int prow = par * B + b;
            const bool pfin = a.finished[prow] != 0;
            int st = a.row_state[prow];
            if (a.next && !pfin) {
                const int nx = a.next[(long)min(max(st, 0), a.n_states - 1) * V + tok];
                if (nx >= 0) st = nx;                           // (an illegal token only ever enters the beam at -inf: a dead slot)
            }
            const int fin = (pfin || tok == a.eos_id || !(bv > -INFINITY)) ? 1 : 0;
            new_cnt += fin;
            if (lane == 0) { s_score[j] = bv; s_tok[j] = tok; s_par[j] = par; s_state[j] = st; s_fin[j] = fin; }
        }
        if (lane == 0) {
            // a finished hypothesis can be pushed out of the beam: the clip adds the CHANGE of its finished count
            if (new_cnt != old_cnt) atomicAdd(a.n_done, new_cnt - old_cnt);
            atomicAdd(a.done_count + t + 1, new_cnt);
            if (b == 0 && a.steps_exec) *a.steps_exec = t + 1;    // steps run in order on one stream
        }
    }
    __syncthreads();
    if (tid < K) {
        const int row = tid * B + b;
        a.score[row] = s_score[tid]; a.finished[row] = s_fin[tid]; a.row_state[row] = s_state[tid];
        const long hi = (long)t * R + row;
        a.token_hist[hi] = s_tok[tid]; a.parent_hist[hi] = s_par[tid]; a.score_hist[hi] = s_score[tid];
    }
    int par[BM_MAX_K];
#pragma unroll
    for (int j = 0; j < BM_MAX_K; ++j) par[j] = j < K ? s_par[j] : 0;
    // new slot j takes the state row of its parent.  The rows of the clip are permuted in place: a thread owns one column, reads it in
    // all K rows and only then writes it
#pragma unroll 1
    for (int w = 0; w < 2; ++w) {
        float* base = w == 0 ? a.h : a.q;
        const int cols = w == 0 ? a.h_cols : a.q_cols;
        if (!base) continue;
        for (int c = tid; c < cols; c += 256) {
            float x[BM_MAX_K];
#pragma unroll
            for (int k = 0; k < BM_MAX_K; ++k) x[k] = k < K ? base[(long)(k * B + b) * cols + c] : 0.f;
#pragma unroll
            for (int j = 0; j < BM_MAX_K; ++j) {
                if (j >= K) break;
                const int p = par[j];
                const float y = p == 0 ? x[0] : (p == 1 ? x[1] : (p == 2 ? x[2] : x[3]));
                if (p != j) base[(long)(j * B + b) * cols + c] = y;
            }
        }
    }
    // the chosen tokens' embeddings -> the next GRU input rows
    for (int i = tid; i < K * a.E; i += 256) {
        const int j = i / a.E, e = i - j * a.E;
        a.xnext[(long)(j * B + b) * a.ldx + e] = a.emb[(long)s_tok[j] * a.E + e];
    }
}

// One wave per clip: the pick (score / len^alpha, ties to the lowest slot), the walk back over the parents, ids / lengths, and the winning
// lineage's log-probability rows gathered from the scratch.
__global__ __launch_bounds__(64) void beam_backtrack(BeamBackArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int B = a.B, K = a.K, R = K * B, V = a.V;
    if (b >= B) return;
    int T = a.steps_exec ? *a.steps_exec : a.max_t;
    T = min(max(T, 0), a.max_t);
    // lane k < K walks slot k back to find its <eos>
    float norm = -INFINITY; int slot = BM_NONE;
    if (lane < K) {
        int cur = lane, eos = -1;
        for (int t = T - 1; t >= 0; --t) {
            const long hi = (long)t * R + cur * B + b;
            if (a.token_hist[hi] == a.eos_id) eos = t;
            cur = min(max(a.parent_hist[hi], 0), K - 1);
        }
        const float sc = a.score[lane * B + b];
        const int len = eos >= 0 ? eos + 1 : T;
        norm = (a.alpha == 0.f || len <= 0) ? sc : sc / powf((float)len, a.alpha);
        slot = lane;
    }
    bm_wave_best(norm, slot);
    if (slot == BM_NONE) slot = 0;
    if (lane == 0 && a.score_out) a.score_out[b] = a.score[slot * B + b];
    int cur = slot, eos = -1;
    float* pb = a.probs + (long)b * a.probs_bstride;
    for (int t = T - 1; t >= 0; --t) {
        const long hi = (long)t * R + cur * B + b;
        const int tok = a.token_hist[hi];
        const int p = min(max(a.parent_hist[hi], 0), K - 1);
        if (tok == a.eos_id) eos = t;
        if (lane == 0) a.ids_out[(long)b * a.ids_bstride + t] = tok;
        // the row that computed step t's logits is the PARENT's
        const float* src = a.probs_scratch + ((long)(p * B + b) * a.max_t + t) * V;
        for (int j = lane; j < V; j += 64) pb[(long)t * V + j] = src[j];
        cur = p;
    }
    for (int t = T + lane; t < a.max_t; t += 64) a.ids_out[(long)b * a.ids_bstride + t] = a.pad_id;
    if (lane == 0 && a.lengths_out) a.lengths_out[b] = eos >= 0 ? eos + 1 : a.max_t;
}

// slot 0 alive at score 0, the others dead (-inf, finished); the counters start at the (K - 1) * B dead slots
__global__ void beam_init(float* score, int* finished, int* n_done, int* done_count, int B, int K, int steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < K * B) { score[i] = i < B ? 0.f : -INFINITY; finished[i] = i < B ? 0 : 1; }
    if (i <= steps) done_count[i] = i == 0 ? (K - 1) * B : 0;
    if (i == 0) *n_done = (K - 1) * B;
}

bool a2s_beam_args_ok(const a2s_beam_args& g, int R, int n_clips, int V) {
    if (g.K < 1 || g.K > BM_MAX_K || n_clips < 1 || R != g.K * n_clips || V < 1 || V > BM_MAX_V) return false;
    if ((g.next_state != nullptr) != (g.n_states > 0) || g.n_states < 0 || g.n_states > 127) return false;
    if (g.pad_id < 0 || g.pad_id >= V || !(g.alpha == g.alpha)) return false;
    return g.row_state && g.score && g.finished && g.done_count && g.token_hist && g.parent_hist && g.score_hist && g.probs_scratch;
}

int a2s_beam_init_impl(hipStream_t st, const a2s_beam_args& g, int* n_done, int B, int steps) {
    const int n = g.K * B > steps + 1 ? g.K * B : steps + 1;
    hipLaunchKernelGGL(beam_init, dim3(a2s_cdiv(n, 256)), dim3(256), 0, st, g.score, g.finished, n_done, g.done_count, B, g.K, steps);
    A2S_CHECK_LAUNCH("beam_init");
    return A2S_OK;
}

int a2s_beam_step_finalize_impl(hipStream_t st, const BeamStepArgs& a) {
    A2S_REQUIRE(a.K >= 1 && a.K <= BM_MAX_K && a.B >= 1 && a.V >= 1 && a.V <= BM_MAX_V && a.E >= 0 && a.t >= 0 && a.t < a.max_t,
                "beam_step_finalize: needs 1 <= K <= %d, 1 <= V <= %d and a step below max_steps (got K = %d, V = %d, step %d of %d)", BM_MAX_K, BM_MAX_V, a.K, a.V, a.t, a.max_t);
    A2S_REQUIRE(a.logits && a.ldl >= a.V && a.emb && a.xnext && a.ldx >= a.E && a.n_done && a.done_count && a.row_state && a.score && a.finished && a.token_hist &&
                a.parent_hist && a.score_hist && a.probs_scratch, "beam_step_finalize: null buffer or a row stride below its width");
    A2S_REQUIRE((a.next != nullptr) == (a.n_states > 0) && a.n_states <= 127 && a.pad_id >= 0 && a.pad_id < a.V && a.h_cols >= 0 && a.q_cols >= 0,
                "beam_step_finalize: bad grammar table, <pad> id or state width");
#define A2S_BM_STEP(NK) hipLaunchKernelGGL(beam_step_finalize<NK>, dim3(a.B), dim3(256), 0, st, a)
    switch ((a.V + 63) / 64) {
        case 1: A2S_BM_STEP(1); break;
        case 2: A2S_BM_STEP(2); break;
        case 3: A2S_BM_STEP(3); break;
        default: A2S_BM_STEP(4); break;
    }
#undef A2S_BM_STEP
    A2S_CHECK_LAUNCH("beam_step_finalize");
    __atomic_fetch_add(&bm_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_beam_backtrack_impl(hipStream_t st, const BeamBackArgs& a) {
    A2S_REQUIRE(a.K >= 1 && a.K <= BM_MAX_K && a.B >= 1 && a.V >= 1 && a.max_t >= 0 && a.pad_id >= 0, "beam_backtrack: needs 1 <= K <= %d (got %d)", BM_MAX_K, a.K);
    A2S_REQUIRE(a.score && a.token_hist && a.parent_hist && a.probs_scratch && a.probs && a.ids_out && a.ids_bstride >= a.max_t && a.alpha == a.alpha,
                "beam_backtrack: null buffer, an id row stride below max_steps or a NaN length penalty");
    hipLaunchKernelGGL(beam_backtrack, dim3(a.B), dim3(64), 0, st, a);
    A2S_CHECK_LAUNCH("beam_backtrack");
    return A2S_OK;
}

int a2s_beam_launches_impl(void) { return (int)__atomic_load_n(&bm_launches, __ATOMIC_RELAXED); }
