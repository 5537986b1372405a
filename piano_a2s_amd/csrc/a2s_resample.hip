// Sample-rate conversion of recordings: a rational polyphase resampler with the mono mix in front of it, between an audio file
// and the VQT.  The float64 definition is tests/resample_oracle.py.
//
// resample_rows: y[b][n] = sum_{i = 0 .. K-1} table[p][i] * mono_b[m0 + Hh - i],  n in [0, n_out[b]);  q = n * M (64-bit), p = q mod L, m0 = q div L;
//     mono_b[m] = (sum_{c < C, ascending} x[b][m * C + c]) * (1.0f / C) for m in [0, n_in[b]), 0 elsewhere;  n_out[b] = ceil(n_in[b] * L / M) (64-bit);
//     y[b][n] = 0 for n in [n_out[b], n_out_max).  n_in[b] is clamped to [0, n_in_max].  fp32 FMAs, i ascending, one thread per output's whole sum.
//     Grid (ceil(n_out_max / RS_TILE), B), RS_THREADS threads, tiles anchored at output 0.  A tile at t0 first stages the window of mono that its
//     outputs need in LDS: xs[g] = mono_b[wbase + g], g in [0, wcap), wbase = (m0(t0) + Hh - (K - 1)) rounded DOWN to a multiple of 4 and
//     wcap = ((RS_TILE - 1) * M / L + 1 + K + 3) rounded up to a multiple of 4 (the host's figure: it sizes the dynamic LDS).  Four frames per thread
//     and step: where x's rows are 16-byte aligned and the four frames lie inside [0, n_in[b]), C 16-byte loads (a group starts at a frame that is a
//     multiple of 4, so at a multiple of 16 bytes); otherwise frame by frame and channel by channel under m in [0, n_in[b]), so that nothing at or
//     behind n_in[b] frames is read at all.  The mix is the ascending sum of the channels, times 1.0f / C (a host constant), both in fp32.
//     Outputs n and n + L have the same phase p, so a thread owns RS_R outputs S apart, S = L * max(1, RS_THREADS / L) a multiple of L: it loads
//     each tap once for RS_R FMAs.  The tile is cut into superblocks of S * RS_R outputs; item (sb, j) owns the outputs sb * S * RS_R + j + r * S,
//     j in [0, S), r in [0, RS_R), as far as they lie inside the tile, and the threads walk the items with stride RS_THREADS.  Every output of the tile
//     belongs to exactly one (item, r).  The inputs of the RS_R outputs are (S / L) * M samples apart.  With L = 1 every thread is on phase 0: the
//     taps are read through the scalar unit (UNIFORM).  Otherwise every lane walks its own row of the table, 16 bytes at a time between the row's
//     first and last 16-byte boundary where the table is 16-byte aligned, 4 bytes at a time before, behind and otherwise.  The sum of an output is the
//     same chain either way.  An (item, r) beyond the tile repeats the item's first output and drops it, so that no LDS index leaves the window.
//     The results go through LDS (ys, RS_TILE floats behind the window) so that y is written 16 bytes at a time where its rows allow it: four outputs
//     per thread and step, zero where n >= n_out[b]; the tile's last, partial group and unaligned rows are written 4 bytes at a time under
//     n < n_out_max.  A tile at or behind n_out[b] stages and computes nothing and writes zeros.
//     A sample's bits depend on its own chain alone: not on B, on the other clips, on n_out_max, on the tiling or on alignment.  No atomics, nothing
//     persistent, no waits between workgroups, plain loads and vector stores only.
//     Bounds: x is read at [0, n_in[b] * C) of clip b's row (n_in[b] <= n_in_max, x_bstride >= n_in_max * C), table at [p * K, p * K + K), p < L, y
//     is written at [t0, min(t0 + RS_TILE, n_out_max)) of clip b's row.  LDS: the window is read at m0(n) + Hh - i - wbase for n in
//     [t0, t0 + RS_TILE), i in [0, K): at least (m0(t0) + Hh - (K - 1)) - wbase >= 0, at most m0(t0) + (RS_TILE - 1) * M / L + 1 + Hh - wbase
//     <= (RS_TILE - 1) * M / L + 1 + K + 2 < wcap;  ys at [0, RS_TILE).
#include "a2s_internal.h"

#define RS_THREADS 320
#define RS_R 4
#define RS_TILE (RS_THREADS * RS_R)
#define RS_WINDOW_MAX 15104          // floats: window + RS_TILE results = 64 KiB of LDS

static long long resample_launches = 0;

// xs[g] = mono_b[wbase + g], g in [0, wcap): four frames per thread and step; wbase and wcap are multiples of 4
template <int C>
__device__ __forceinline__ void rs_stage(float* __restrict__ xs, const float* __restrict__ xb, long long wbase, int wcap, int nin, float inv_c, int x_vec,
                                         int tid) {
    for (int g = tid * 4; g < wcap; g += RS_THREADS * 4) {
        const long long m = wbase + g;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (x_vec && m >= 0 && m + 4 <= (long long)nin) {
            f32x4 q[C];
#pragma unroll
            for (int k = 0; k < C; ++k) q[k] = *reinterpret_cast<const f32x4*>(xb + m * C + 4 * k);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s = q[(e * C) / 4][(e * C) % 4];
#pragma unroll
                for (int c = 1; c < C; ++c) s += q[(e * C + c) / 4][(e * C + c) % 4];
                v[e] = s * inv_c;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (m + e >= 0 && m + e < (long long)nin) {
                    const float* f = xb + (m + e) * C;
                    float s = f[0];
#pragma unroll
                    for (int c = 1; c < C; ++c) s += f[c];
                    v[e] = s * inv_c;
                }
            }
        }
        *reinterpret_cast<f32x4*>(xs + g) = v;
    }
}

// one tap on a thread's RS_R outputs: xs[w[r] - i] = mono[m0_r + Hh - i]
__device__ __forceinline__ void rs_tap(float (&acc)[RS_R], float h, const float* __restrict__ xs, const int (&w)[RS_R], int i) {
#pragma unroll
    for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(h, xs[w[r] - i], acc[r]);
}

template <bool UNIFORM>
__global__ __launch_bounds__(RS_THREADS) void resample_rows(const float* __restrict__ x, long x_bstride, const int* __restrict__ n_in, int n_in_max, int C,
                                                            float inv_c, const float* __restrict__ table, int L, int M, int K, int Hh,
                                                            float* __restrict__ y, long y_bstride, int n_out_max, int wcap, int x_vec, int t_vec,
                                                            int y_vec) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    float* ys = xs + wcap;
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long t0 = (long long)blockIdx.x * RS_TILE;
    const int nin = min(max(n_in[b], 0), n_in_max);
    const long long nout = min(((long long)nin * L + M - 1) / M, (long long)n_out_max);
    const int tile_n = (int)min((long long)RS_TILE, (long long)n_out_max - t0);
    const bool live = t0 < nout;

    if (live) {
        const long long m00 = (t0 * M) / L;
        const long long wbase = (m00 + Hh - (K - 1)) & ~3LL;          // (rounds down for negative values too)
        const float* __restrict__ xb = x + (long)b * x_bstride;
        switch (C) {
            case 1: rs_stage<1>(xs, xb, wbase, wcap, nin, inv_c, x_vec, tid); break;
            case 2: rs_stage<2>(xs, xb, wbase, wcap, nin, inv_c, x_vec, tid); break;
            case 3: rs_stage<3>(xs, xb, wbase, wcap, nin, inv_c, x_vec, tid); break;
            case 4: rs_stage<4>(xs, xb, wbase, wcap, nin, inv_c, x_vec, tid); break;
            case 5: rs_stage<5>(xs, xb, wbase, wcap, nin, inv_c, x_vec, tid); break;
            case 6: rs_stage<6>(xs, xb, wbase, wcap, nin, inv_c, x_vec, tid); break;
            case 7: rs_stage<7>(xs, xb, wbase, wcap, nin, inv_c, x_vec, tid); break;
            default: rs_stage<8>(xs, xb, wbase, wcap, nin, inv_c, x_vec, tid); break;
        }
        __syncthreads();

        const int S = UNIFORM ? RS_THREADS : L * max(1, RS_THREADS / L);
        const int dm = (S / L) * M;                                    // between the inputs of a thread's outputs
        const int items = ((RS_TILE + S * RS_R - 1) / (S * RS_R)) * S;
        for (int item = tid; item < items; item += RS_THREADS) {
            const int j0 = (item / S) * (S * RS_R) + item % S;
            if (j0 >= RS_TILE) continue;
            const long long q = (t0 + j0) * M;
            const int p = UNIFORM ? 0 : (int)(q % L);
            const int w0 = (int)(q / L + Hh - wbase);
            int w[RS_R];
            float acc[RS_R];
#pragma unroll
            for (int r = 0; r < RS_R; ++r) {
                w[r] = w0 + (j0 + r * S < RS_TILE ? r * dm : 0);
                acc[r] = 0.f;
            }
            if (UNIFORM) {
#pragma unroll 8
                for (int i = 0; i < K; ++i) rs_tap(acc, table[i], xs, w, i);
            } else {
                const float* __restrict__ trow = table + (long)p * K;
                const int head = t_vec ? min(K, (int)((4 - (((uintptr_t)trow >> 2) & 3)) & 3)) : K;
                int i = 0;
                for (; i < head; ++i) rs_tap(acc, trow[i], xs, w, i);
#pragma unroll 2
                for (; i + 4 <= K; i += 4) {
                    const f32x4 h = *reinterpret_cast<const f32x4*>(trow + i);
                    rs_tap(acc, h[0], xs, w, i);
                    rs_tap(acc, h[1], xs, w, i + 1);
                    rs_tap(acc, h[2], xs, w, i + 2);
                    rs_tap(acc, h[3], xs, w, i + 3);
                }
                for (; i < K; ++i) rs_tap(acc, trow[i], xs, w, i);
            }
#pragma unroll
            for (int r = 0; r < RS_R; ++r)
                if (j0 + r * S < RS_TILE) ys[j0 + r * S] = acc[r];
        }
        __syncthreads();
    }

    float* __restrict__ yb = y + (long)b * y_bstride + t0;
    for (int g = tid * 4; g < tile_n; g += RS_THREADS * 4) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (live) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t0 + g + e < nout) v[e] = ys[g + e];
        }
        if (y_vec && g + 4 <= tile_n) {
            *reinterpret_cast<f32x4*>(yb + g) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (g + e < tile_n) yb[g + e] = v[e];
        }
    }
}

int a2s_resample_rows_impl(hipStream_t st, const float* x, long x_bstride, const int* n_in, int n_in_max, int C, const float* table, int L, int M, int K,
                           int Hh, float* y, long y_bstride, int n_out_max, int B) {
    A2S_REQUIRE(x && n_in && table && y, "resample_rows: null x, n_in, table or y");
    A2S_REQUIRE(x != y, "resample_rows: works out of place (x == y)");
    A2S_REQUIRE(B >= 0 && B <= 65535, "resample_rows: needs 0 <= B <= 65535 (got %d)", B);
    A2S_REQUIRE(C >= 1 && C <= 8, "resample_rows: needs 1 <= C <= 8 channels (got %d)", C);
    A2S_REQUIRE(L >= 1 && L <= 4096 && M >= 1 && M <= 4096, "resample_rows: needs L and M in 1 .. 4096 (got L = %d, M = %d)", L, M);
    A2S_REQUIRE(K >= 1 && K <= 8192 && Hh >= 0 && Hh < K, "resample_rows: needs K in 1 .. 8192 and 0 <= Hh < K (got K = %d, Hh = %d)", K, Hh);
    const long span = (long)(RS_TILE - 1) * M / L + 1;
    A2S_REQUIRE(span + K + 7 <= RS_WINDOW_MAX, "resample_rows: the window of a tile, %ld samples for L = %d, M = %d, K = %d, exceeds %d", span + K + 7, L, M, K,
                RS_WINDOW_MAX);
    A2S_REQUIRE(n_in_max >= 0 && n_out_max >= 1, "resample_rows: needs n_in_max >= 0 and n_out_max >= 1 (got %d, %d)", n_in_max, n_out_max);
    A2S_REQUIRE(x_bstride >= (long)n_in_max * C && y_bstride >= n_out_max,
                "resample_rows: needs an x stride >= n_in_max * C and a y stride >= n_out_max (got %ld, %ld for n_in_max = %d, C = %d, n_out_max = %d)", x_bstride,
                y_bstride, n_in_max, C, n_out_max);
    if (B == 0) return A2S_OK;
    const int wcap = (int)((span + K + 3 + 3) & ~3L);
    const int x_vec = (((uintptr_t)x & 15) == 0 && x_bstride % 4 == 0) ? 1 : 0;
    const int y_vec = (((uintptr_t)y & 15) == 0 && y_bstride % 4 == 0) ? 1 : 0;
    const int t_vec = ((uintptr_t)table & 15) == 0 ? 1 : 0;
    const size_t lds = (size_t)(wcap + RS_TILE) * sizeof(float);
    const dim3 grid(a2s_cdiv(n_out_max, RS_TILE), B);
    const float inv_c = 1.0f / (float)C;
    if (L == 1)
        hipLaunchKernelGGL(resample_rows<true>, grid, dim3(RS_THREADS), lds, st, x, x_bstride, n_in, n_in_max, C, inv_c, table, L, M, K, Hh, y, y_bstride,
                           n_out_max, wcap, x_vec, t_vec, y_vec);
    else
        hipLaunchKernelGGL(resample_rows<false>, grid, dim3(RS_THREADS), lds, st, x, x_bstride, n_in, n_in_max, C, inv_c, table, L, M, K, Hh, y, y_bstride,
                           n_out_max, wcap, x_vec, t_vec, y_vec);
    A2S_CHECK_LAUNCH("resample_rows");
    __atomic_fetch_add(&resample_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_resample_tile_samples_impl(void) { return RS_TILE; }
int a2s_resample_launches_impl(void) { return (int)__atomic_load_n(&resample_launches, __ATOMIC_RELAXED); }
