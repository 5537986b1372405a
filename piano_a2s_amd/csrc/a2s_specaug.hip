// Spectrogram augmentation of a training batch on the device: per clip a per-bin gain that respects the front end's floor, an
// additive noise floor, the front end's re-normalisation, and SpecAugment masks along time and frequency.  The targets stay.
//
// Features x (B, rows, F) are dB / 80 + 1 relative to the clip's peak, so P(x) = 10^(8 (x - 1)) is a cell's power relative to that peak.  Per clip b
// (tests/specaug_oracle.py states the same in float64):
//     n      = 1 + the last row that holds a value != 0 (a NaN is content, -0.0 is not; 0 for an all-zero clip): rows >= n are padding;
//     x_min  = min of x over rows < n;  a cell is AT THE FLOOR iff x - x_min <= 2^-18 (one fp32 subtraction, one compare);  p_min = P(x_min);
//     y      = max(p_min, q + v_k),  q = 0 for a floor cell, else G_k * P(x);   table (B, 2, F): row 0 the power gains G_k > 0, row 1 the noise v_k >= 0;
//     M      = max of y over rows < n;
//     out    = clamp(1 + log10(y / M) / 8, 0, 1),  then 0 in padding rows, in the rows [t0_i, t0_i + w_i) and, in rows < n, in the bins [k0_i, k0_i + wk_i).
// What lies under the front end's clamp is unknown: a floor cell keeps its place (it does not follow the gain), and no cell falls below the floor.
// sa_cell forms y, for the peak sweep and for the apply alike, out of __f*_rn operations that the compiler cannot contract: the cell that attains M
// has y / M == 1 exactly and comes out as 1.0.
// The mask plan is integer arithmetic on the host's 32-bit draws d[b][4 i .. 4 i + 3] = [u, u', u'', u'''] (64-bit products):
//     wmax_t = min(Wt, n / 5),  w  = (u   * (wmax_t + 1)) >> 32,  t0 = (u'   * (n - w  + 1)) >> 32;
//     wmax_f = min(Wf, F / 5),  wk = (u'' * (wmax_f + 1)) >> 32,  k0 = (u''' * (F - wk + 1)) >> 32;     masks i >= m: [0, 0].
//
// specaug_plan: one workgroup of 1024 threads per clip, which sweeps its clip twice after the content scan (a2s_content_rows, a2s_internal.h): once
//     for x_min, once for M (M needs p_min, so the sweeps cannot be one): 2.3 MB per sweep at 1201 x 480, more than the clips in flight leave of the L2.
//     No workgroup waits for another, nothing spins, no partial results cross launches: the batch costs this launch and the apply.  Thread 0 plans
//     the masks and adds to the counters: [clips, clips with a time mask of width > 0, clips with a frequency mask of width > 0].
//     Bounds: loads at [0, n * F) of clip b, [0, 2 F) of its table rows and its 16 draws; stores: content[b], plan[16 b .. 16 b + 15],
//     stats[2 b .. 2 b + 1] = [x_min, M] ([0, 0] for an all-zero clip), atomic adds on counters[0 .. 2].
// specaug_apply: one streaming launch, grid (ceil(rows / 16), B, column tiles), block (128, 2) as stretch_frames: threadIdx.x and blockIdx.z pick the
//     columns (four floats per thread when F % 4 == 0 and y is 16-byte aligned), threadIdx.y eight consecutive rows.  Gains, noise and the frequency
//     masks of a thread's columns are formed once; whether a row is padding or under a time mask is uniform per row, and such a row is not loaded.
//     content[b] is clamped to [0, rows] before it bounds a load.
//     Bounds: loads at columns [0, F) of rows [0, n) of clip b and of its two table rows; stores at columns [0, F) of rows t < rows of clip b.
#include "a2s_internal.h"

#define SA_PLAN_THREADS 1024
#define SA_MAX_MASKS 4
#define SA_FLOOR_EPS 0x1p-18f
#define SA_8_LOG2_10 26.575424759098897f          // P(x) = 2^(8 log2(10) (x - 1))
#define SA_LOG10_2_8TH 0.037628749457997640f      // log10(r) / 8 = log2(r) * log10(2) / 8

static long long specaug_launches = 0;

__device__ __forceinline__ float sa_power(float x) { return exp2f(__fmul_rn(__fsub_rn(x, 1.0f), SA_8_LOG2_10)); }

// y of one cell: the peak sweep of the plan and the apply both call this and nothing else
__device__ __forceinline__ float sa_cell(float x, float x_min, float p_min, float G, float v) {
    const float q = __fsub_rn(x, x_min) <= SA_FLOOR_EPS ? 0.0f : __fmul_rn(G, sa_power(x));
    return fmaxf(p_min, __fadd_rn(q, v));
}

__device__ __forceinline__ float sa_out(float y, float M) {
    const float r = __fadd_rn(1.0f, __fmul_rn(log2f(__fdiv_rn(y, M)), SA_LOG10_2_8TH));          // y == M: log2f(1) = 0, r = 1 exactly
    return fminf(fmaxf(r, 0.0f), 1.0f);
}

// min or max over the workgroup, the same value in every thread (exact whatever the order)
template <bool MAX>
__device__ __forceinline__ float sa_block_reduce(float v, float* s_part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o);
        v = MAX ? fmaxf(v, w) : fminf(v, w);
    }
    __syncthreads();                              // (s_part may still be read from the reduction before)
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = s_part[0];
#pragma unroll
    for (int i = 1; i < SA_PLAN_THREADS / 64; ++i) r = MAX ? fmaxf(r, s_part[i]) : fminf(r, s_part[i]);
    return r;
}

__global__ __launch_bounds__(SA_PLAN_THREADS) void specaug_plan(const float* __restrict__ x, int rows, int F, const float* __restrict__ table,
                                                                const unsigned* __restrict__ draws, int Wt, int Wf, int m, int* __restrict__ content,
                                                                int* __restrict__ plan, float* __restrict__ stats, int* __restrict__ counters) {
    __shared__ int s_last;
    __shared__ float s_part[SA_PLAN_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* xb = x + (long)b * rows * F;
    const int n = a2s_content_rows<SA_PLAN_THREADS>(xb, rows, F, &s_last);
    float x_min = 0.0f, M = 0.0f;
    if (n > 0) {                                  // (uniform: the reductions' barriers are met by every thread)
        const float* G = table + (long)b * 2 * F;
        const float* V = G + F;
        const long len = (long)n * F;
        float lo = INFINITY, hi = 0.0f;
        if (F % 4 == 0) {
#pragma unroll 4
            for (long i = (long)tid * 4; i < len; i += SA_PLAN_THREADS * 4) {
                float c[4];
                __builtin_memcpy(c, xb + i, 16);          // 4-byte aligned: x need not be 16-byte aligned
                lo = fminf(fminf(lo, fminf(c[0], c[1])), fminf(c[2], c[3]));
            }
        } else {
#pragma unroll 4
            for (long i = tid; i < len; i += SA_PLAN_THREADS) lo = fminf(lo, xb[i]);
        }
        x_min = sa_block_reduce<false>(lo, s_part);
        const float p_min = sa_power(x_min);
        if (F % 4 == 0) {
#pragma unroll 2
            for (long i = (long)tid * 4; i < len; i += SA_PLAN_THREADS * 4) {
                const int k = (int)(i % F);               // (F % 4 == 0: the four cells lie in one row)
                float c[4], g[4], v[4];
                __builtin_memcpy(c, xb + i, 16);
                __builtin_memcpy(g, G + k, 16);
                __builtin_memcpy(v, V + k, 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) hi = fmaxf(hi, sa_cell(c[e], x_min, p_min, g[e], v[e]));
            }
        } else {
#pragma unroll 2
            for (long i = tid; i < len; i += SA_PLAN_THREADS) {
                const int k = (int)(i % F);
                hi = fmaxf(hi, sa_cell(xb[i], x_min, p_min, G[k], V[k]));
            }
        }
        M = sa_block_reduce<true>(hi, s_part);
    }
    if (tid != 0) return;
    const unsigned* d = draws + (long)b * 4 * SA_MAX_MASKS;
    int* p = plan + (long)b * 4 * SA_MAX_MASKS;
    const int wmax_t = Wt < n / 5 ? Wt : n / 5, wmax_f = Wf < F / 5 ? Wf : F / 5;
    int any_t = 0, any_f = 0;
    for (int i = 0; i < SA_MAX_MASKS; ++i) {
        int t0 = 0, w = 0, k0 = 0, wk = 0;
        if (i < m) {
            w = (int)(((unsigned long long)d[4 * i] * (unsigned long long)(wmax_t + 1)) >> 32);
            t0 = (int)(((unsigned long long)d[4 * i + 1] * (unsigned long long)(n - w + 1)) >> 32);
            wk = (int)(((unsigned long long)d[4 * i + 2] * (unsigned long long)(wmax_f + 1)) >> 32);
            k0 = (int)(((unsigned long long)d[4 * i + 3] * (unsigned long long)(F - wk + 1)) >> 32);
        }
        p[2 * i] = t0;
        p[2 * i + 1] = w;
        p[2 * SA_MAX_MASKS + 2 * i] = k0;
        p[2 * SA_MAX_MASKS + 2 * i + 1] = wk;
        any_t |= w > 0;
        any_f |= wk > 0;
    }
    content[b] = n;
    stats[2 * b] = x_min;
    stats[2 * b + 1] = M;
    atomicAdd(&counters[0], 1);
    if (any_t) atomicAdd(&counters[1], 1);
    if (any_f) atomicAdd(&counters[2], 1);
}

template <int VEC>
__global__ __launch_bounds__(A2S_ROW_TX * A2S_ROW_TY) void specaug_apply(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ table,
                                                               const int* __restrict__ content, const int* __restrict__ plan,
                                                               const float* __restrict__ stats, int rows, int F) {
    typedef typename a2s_row_vec<VEC>::type V;
    const int b = blockIdx.y, j = (blockIdx.z * A2S_ROW_TX + threadIdx.x) * VEC;          // this thread's columns j .. j + VEC - 1, in every row
    const int ty = __builtin_amdgcn_readfirstlane(threadIdx.y);          // (a wave has one threadIdx.y: everything per row below is scalar)
    const int t0 = blockIdx.x * A2S_ROW_TILE + ty * A2S_ROW_NR;
    if (t0 >= rows || j >= F) return;
    const int nr = rows - t0 < A2S_ROW_NR ? rows - t0 : A2S_ROW_NR;                // output rows of this thread that exist
    int n = content[b];
    n = n < 0 ? 0 : (n > rows ? rows : n);                               // (it bounds the loads below)
    const float x_min = stats[2 * b], M = stats[2 * b + 1];
    const float p_min = sa_power(x_min);
    const int* pl = plan + (long)b * 4 * SA_MAX_MASKS;
    const float* xb = x + (long)b * rows * F;
    float* y0 = y + (long)b * rows * F + (long)t0 * F;
    float g[VEC], v[VEC];
    bool masked[VEC];
    __builtin_memcpy(g, table + (long)b * 2 * F + j, 4 * VEC);
    __builtin_memcpy(v, table + (long)b * 2 * F + F + j, 4 * VEC);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        masked[e] = false;
#pragma unroll
        for (int i = 0; i < SA_MAX_MASKS; ++i) {
            const int k0 = pl[2 * SA_MAX_MASKS + 2 * i], wk = pl[2 * SA_MAX_MASKS + 2 * i + 1];
            masked[e] = masked[e] || (j + e >= k0 && j + e - k0 < wk);
        }
    }
    float c[A2S_ROW_NR][VEC];
    bool live[A2S_ROW_NR];
#pragma unroll
    for (int r = 0; r < A2S_ROW_NR; ++r) {                                    // all loads are issued together
        const int t = t0 + r;
        live[r] = r < nr && t < n;
#pragma unroll
        for (int i = 0; i < SA_MAX_MASKS; ++i) {
            const int m0 = pl[2 * i], w = pl[2 * i + 1];
            live[r] = live[r] && !(t >= m0 && t - m0 < w);
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) c[r][e] = 0.0f;
        if (live[r]) __builtin_memcpy(c[r], xb + (long)t * F + j, 4 * VEC);          // 4-byte aligned: x need not be aligned as y is
    }
#pragma unroll
    for (int r = 0; r < A2S_ROW_NR; ++r) {
        if (r >= nr) break;
        float o[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = (live[r] && !masked[e]) ? sa_out(sa_cell(c[r][e], x_min, p_min, g[e], v[e]), M) : 0.0f;
        V out;
        __builtin_memcpy(&out, o, 4 * VEC);
        *reinterpret_cast<V*>(y0 + (long)r * F + j) = out;
    }
}

int a2s_specaug_plan_impl(hipStream_t st, const float* x, int B, int rows, int F, const float* table, const unsigned* draws, int Wt, int Wf, int m,
                          int* content, int* plan, float* stats, int* counters) {
    A2S_REQUIRE(x && table && draws && content && plan && stats && counters, "specaug_plan: null x, table, draws, content, plan, stats or counter pointer");
    A2S_REQUIRE(B >= 0 && B <= 65535, "specaug_plan: needs 0 <= B <= 65535 (got %d)", B);
    A2S_REQUIRE(rows >= 1 && F >= 1, "specaug_plan: needs rows >= 1 and F >= 1 (got rows = %d, F = %d)", rows, F);
    A2S_REQUIRE(Wt >= 0 && Wf >= 0, "specaug_plan: the mask widths Wt and Wf must be >= 0 (got %d, %d)", Wt, Wf);
    A2S_REQUIRE(m >= 0 && m <= SA_MAX_MASKS, "specaug_plan: the mask count m must be in 0 .. %d (got %d)", SA_MAX_MASKS, m);
    if (B == 0) return A2S_OK;
    hipLaunchKernelGGL(specaug_plan, dim3(B), dim3(SA_PLAN_THREADS), 0, st, x, rows, F, table, draws, Wt, Wf, m, content, plan, stats, counters);
    A2S_CHECK_LAUNCH("specaug_plan");
    __atomic_fetch_add(&specaug_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_specaug_apply_impl(hipStream_t st, const float* x, float* y, const float* table, const int* content, const int* plan, const float* stats, int B,
                           int rows, int F) {
    A2S_REQUIRE(x && y && table && content && plan && stats, "specaug_apply: null x, y, table, content, plan or stats");
    A2S_REQUIRE(x != y, "specaug_apply: works out of place (x == y)");
    A2S_REQUIRE(B >= 0 && B <= 65535, "specaug_apply: needs 0 <= B <= 65535 (got %d)", B);
    A2S_REQUIRE(rows >= 1 && F >= 1, "specaug_apply: needs rows >= 1 and F >= 1 (got rows = %d, F = %d)", rows, F);
    if (B == 0) return A2S_OK;
    const int vec = a2s_row_vec_width(F, y);
    dim3 grid;
    A2S_REQUIRE(a2s_row_grid(B, rows, F, vec, &grid), "specaug_apply: %d columns are too many", F);
    A2S_ROW_LAUNCH(specaug_apply, vec, grid, st, x, y, table, content, plan, stats, rows, F);
    A2S_CHECK_LAUNCH("specaug_apply");
    __atomic_fetch_add(&specaug_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_specaug_launches_impl(void) { return (int)__atomic_load_n(&specaug_launches, __ATOMIC_RELAXED); }
