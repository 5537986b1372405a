// Tempo augmentation of a training batch on the device: every clip's feature rows are resampled along time, the targets stay.
//
// All positions are integers in Q16 (TP_ONE = 65536 = one source row), so that the host oracle (tests/tempo_oracle.py) and the kernels agree exactly.
// step[b] = rint(65536 / c) is the source advance per output row of clip b, c the factor on durations (c > 1: slower, longer).  Output row t:
//     pos = t * step,  h = max(65536, step),  w_k = h - |k * 65536 - pos| (kept where > 0),  W = sum of w_k over ALL integer k,
//     y[b][t][f] = sum_k (w_k / W) x[b][k][f],  x = 0 for k outside [0, rows).
// step <= 65536: linear interpolation between rows pos >> 16 and the next, W = 65536, the weights w / 65536 exact.  step > 65536: a tent widened to
// the source advance, so that no source row is skipped; for step <= TP_MAX_STEP (c >= 0.75) at most three taps, the rows klo, klo + 1, klo + 2 with
// klo = floor((pos - h + 65536) / 65536), whose first weight is always > 0.  A tap of weight 0 is not read and not added: step == 65536 writes x bit
// for bit.  step outside [TP_MIN_STEP, TP_MAX_STEP]: zeros for that clip.  rows <= 16384 keeps pos below 2^31.
//
// tempo_plan: one workgroup of 256 threads per clip.  content[b] = 1 + the last row that holds a value != 0 (a NaN is content, -0.0 is not; 0 for an
//     all-zero clip), found by scanning BACKWARDS from the last row in chunks of TP_CHUNK rows and stopping at the first chunk with content: a clip
//     that fills its window costs one chunk, a padded clip its padding.  Thread 0 then plans, in fp32 and in exactly this form (n = content[b]):
//         lo = max(1 - R, (float)min_frames / n),  hi = min(1 + R, (float)rows / n);
//         n == 0 or lo > hi: step = 65536, the clip counts as kept;  else c = fmaf(u[b], hi - lo, lo), step = clamp((int)rintf(65536.0f / c)).
//     counters[0 .. 2] += clips seen, clips with step != 65536, clips kept for want of a feasible interval.
//     Bounds: loads at [0, rows * F) of clip b only; content[b], step[b] and the three counters are the only stores.
// stretch_frames: grid (ceil(rows / 16), B, column tiles), block (128, 2).  threadIdx.x and blockIdx.z pick the columns (four floats per thread when
//     F % 4 == 0 and y is 16-byte aligned: F = 480 is one tile, 120 of 128 lanes; no loop over columns, so that nothing per row is hoisted out of
//     one and held in registers), threadIdx.y picks 8 CONSECUTIVE output rows of the workgroup's 16.  Those 8 rows read at most 13
//     consecutive source rows (10 = ceil(7 * 87381 / 65536) advances + 3 taps): tap rows, weights and 1 / W are uniform per output row and computed
//     once per row on the scalar unit (threadIdx.y goes through readfirstlane); the source rows are fetched once each, all loads issued together into
//     v[0 .. 12], and every output row then picks its three out of them by a uniform branch on its offset d = klo(row) - klo(first row), so that no
//     register array is indexed dynamically.  Every load is column-aligned with its store; only rows outside [0, rows) (klo = -1 at t = 0, the rows
//     behind the last) are masked, and a masked or zero-weight row is never loaded.
//     Bounds: loads at columns [0, F) of rows [0, rows) of clip b only; stores at columns [0, F) of rows t < rows of clip b.
#include "a2s_internal.h"

#define TP_ONE 65536
#define TP_MIN_STEP 52429      // rint(65536 / 1.25)
#define TP_MAX_STEP 87381      // rint(65536 / 0.75)
#define TP_THREADS 256
#define TP_CHUNK A2S_CONTENT_CHUNK          // (the scan itself: a2s_content_rows, a2s_internal.h)
#define SF_SRC 13

static long long tempo_launches = 0;

__global__ __launch_bounds__(TP_THREADS) void tempo_plan(const float* __restrict__ x, int rows, int F, const float* __restrict__ u, float R, int min_frames,
                                                         int* __restrict__ content, int* __restrict__ step, int* __restrict__ counters) {
    __shared__ int s_last;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* xb = x + (long)b * rows * F;
    const int n = a2s_content_rows<TP_THREADS>(xb, rows, F, &s_last);
    if (tid != 0) return;
    int st = TP_ONE, kept = 1;
    if (n > 0) {
        const float lo = fmaxf(1.0f - R, (float)min_frames / (float)n);
        const float hi = fminf(1.0f + R, (float)rows / (float)n);
        if (!(lo > hi)) {
            const float c = fmaf(u[b], hi - lo, lo);
            const float q = rintf(65536.0f / c);
            st = (int)fminf(fmaxf(q, (float)TP_MIN_STEP), (float)TP_MAX_STEP);          // (a NaN clamps to TP_MIN_STEP)
            kept = 0;
        }
    }
    content[b] = n;
    step[b] = st;
    atomicAdd(&counters[0], 1);
    if (st != TP_ONE) atomicAdd(&counters[1], 1);
    if (kept) atomicAdd(&counters[2], 1);
}

template <int VEC>
__device__ __forceinline__ typename a2s_row_vec<VEC>::type sf_load(const float* p) {
    typename a2s_row_vec<VEC>::type v;
    __builtin_memcpy(&v, p, 4 * VEC);            // 4-byte aligned: x need not be aligned as y is
    return v;
}

// the output of one row from its three candidate source rows: w[i] == 0 (no weight, or a row outside the clip) is neither multiplied nor added
template <typename V>
__device__ __forceinline__ V sf_taps(const V& a, const V& b, const V& c, const int* w, float inv) {
    V acc = V(0.f);
    bool have = false;
    if (w[0] > 0) { acc = ((float)w[0] * inv) * a; have = true; }
    if (w[1] > 0) { acc = have ? acc + ((float)w[1] * inv) * b : ((float)w[1] * inv) * b; have = true; }
    if (w[2] > 0) { acc = have ? acc + ((float)w[2] * inv) * c : ((float)w[2] * inv) * c; }
    return acc;
}

template <int VEC>
__global__ __launch_bounds__(A2S_ROW_TX * A2S_ROW_TY) void stretch_frames(const float* __restrict__ x, float* __restrict__ y, const int* __restrict__ step_of, int rows,
                                                                int F) {
    typedef typename a2s_row_vec<VEC>::type V;
    const int b = blockIdx.y, j = (blockIdx.z * A2S_ROW_TX + threadIdx.x) * VEC;          // this thread's columns j .. j + VEC - 1, in every row
    const int ty = __builtin_amdgcn_readfirstlane(threadIdx.y);          // (a wave has one threadIdx.y: everything per row below is scalar)
    const int step = step_of[b];
    const int t0 = blockIdx.x * A2S_ROW_TILE + ty * A2S_ROW_NR;
    if (t0 >= rows || j >= F) return;
    const int nr = rows - t0 < A2S_ROW_NR ? rows - t0 : A2S_ROW_NR;                // output rows of this thread that exist
    const float* xb = x + (long)b * rows * F;
    float* y0 = y + (long)b * rows * F + (long)t0 * F;
    if (step < TP_MIN_STEP || step > TP_MAX_STEP) {
        for (int r = 0; r < nr; ++r) *reinterpret_cast<V*>(y0 + (long)r * F + j) = V(0.f);
        return;
    }
    const int h = step > TP_ONE ? step : TP_ONE;
    const int kfirst = (t0 * step - h + TP_ONE) >> 16;                   // first tap of the first row (floor: -1 at t = 0 when step > 65536)
    int klast = ((t0 + nr - 1) * step + h - 1) >> 16;                    // last tap of positive weight of the last row
    if (klast > rows - 1) klast = rows - 1;
    const int need = klast - kfirst;                                     // <= 12: source rows kfirst .. kfirst + need are read, those >= 0
    V v[SF_SRC];
#pragma unroll
    for (int i = 0; i < SF_SRC; ++i) {
        v[i] = V(0.f);
        if (i <= need && kfirst + i >= 0) v[i] = sf_load<VEC>(xb + (long)(kfirst + i) * F + j);
    }
#pragma unroll
    for (int r = 0; r < A2S_ROW_NR; ++r) {
        if (r >= nr) break;
        const int pos = (t0 + r) * step;
        const int klo = (pos - h + TP_ONE) >> 16;
        const int c0 = klo * TP_ONE - pos;                               // in (-h, 0]: the first weight h + c0 is > 0
        int w[3], W = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int c = c0 + i * TP_ONE;
            const int wi = h - (c < 0 ? -c : c);
            W += wi > 0 ? wi : 0;                                        // over all k, in range or not
            w[i] = (wi > 0 && klo + i >= 0 && klo + i < rows) ? wi : 0;
        }
        const float inv = 1.0f / (float)W;                               // 65536 -> 2^-16: the weights w / 65536 are exact
        const int d = klo - kfirst;
        V out = V(0.f);
#pragma unroll
        for (int dd = 0; dd <= SF_SRC - 3; ++dd) {
            // d lies in [floor(r * step / 65536), ceil(r * step / 65536)]: only those offsets are compiled for row r
            if (dd < ((r * TP_MIN_STEP) >> 16) || dd > ((r * TP_MAX_STEP + TP_ONE - 1) >> 16)) continue;
            if (dd == d) out = sf_taps<V>(v[dd], v[dd + 1], v[dd + 2], w, inv);
        }
        *reinterpret_cast<V*>(y0 + (long)r * F + j) = out;
    }
}

int a2s_tempo_plan_impl(hipStream_t st, const float* x, int B, int rows, int F, const float* u, float R, int min_frames, int* content, int* step,
                        int* counters) {
    A2S_REQUIRE(x && u && content && step && counters, "tempo_plan: null x, u, content, step or counter pointer");
    A2S_REQUIRE(B >= 0 && B <= 65535, "tempo_plan: needs 0 <= B <= 65535 (got %d)", B);
    A2S_REQUIRE(rows >= 1 && rows <= 16384 && F >= 1, "tempo_plan: needs 1 <= rows <= 16384 and F >= 1 (got rows = %d, F = %d)", rows, F);
    A2S_REQUIRE(R >= 0.0f && R <= 0.25f, "tempo_plan: the tempo range R must be in 0 .. 0.25 (got %g)", (double)R);
    A2S_REQUIRE(min_frames >= 1, "tempo_plan: needs min_frames >= 1 (got %d)", min_frames);
    if (B == 0) return A2S_OK;
    hipLaunchKernelGGL(tempo_plan, dim3(B), dim3(TP_THREADS), 0, st, x, rows, F, u, R, min_frames, content, step, counters);
    A2S_CHECK_LAUNCH("tempo_plan");
    __atomic_fetch_add(&tempo_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_stretch_frames_impl(hipStream_t st, const float* x, float* y, const int* step, int B, int rows, int F) {
    A2S_REQUIRE(x && y && step, "stretch_frames: null x, y or step");
    A2S_REQUIRE(x != y, "stretch_frames: works out of place (x == y)");
    A2S_REQUIRE(B >= 0 && B <= 65535, "stretch_frames: needs 0 <= B <= 65535 (got %d)", B);
    A2S_REQUIRE(rows >= 1 && rows <= 16384 && F >= 1, "stretch_frames: needs 1 <= rows <= 16384 and F >= 1 (got rows = %d, F = %d)", rows, F);
    if (B == 0) return A2S_OK;
    const int vec = a2s_row_vec_width(F, y);
    dim3 grid;
    A2S_REQUIRE(a2s_row_grid(B, rows, F, vec, &grid), "stretch_frames: %d columns are too many", F);
    A2S_ROW_LAUNCH(stretch_frames, vec, grid, st, x, y, step, rows, F);
    A2S_CHECK_LAUNCH("stretch_frames");
    __atomic_fetch_add(&tempo_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_tempo_launches_impl(void) { return (int)__atomic_load_n(&tempo_launches, __ATOMIC_RELAXED); }
