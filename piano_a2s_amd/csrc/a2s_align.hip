// Audio alignment from the attention weights: every bar step and every note step forms softmax weights over the T encoder
// frames, and frame t is t * hop_length / sample_rate seconds of audio.  attn_align_rows reduces one row of those weights -- the fp32 values the
// attention kernels write through their `attw` argument -- to three summaries:
//     peak     = the lowest frame index among the maxima of the row,
//     weight   = a[peak], bit for bit,
//     centroid = sum_t t * a[t]      (the weights are the softmax's and sum to 1 within rounding: nothing is renormalised).
// A row whose attention was skipped holds zeros and yields (0, 0, 0): weight == 0 is the "nothing ran" mark.
//
// One wave per row, four rows per 256-thread workgroup, no LDS: lanes stride the row by 64; maximum and index go through the butterfly of
// note_step_finalize / log_softmax_rows (value, then lowest index), the sum through wave_sum; lane 0 stores.  Any T >= 1, any row stride >= T;
// nothing is indexed outside [0, T) of a row.
#include "a2s_internal.h"

#define AL_NONE 0x7fffffff        // "no candidate yet" index of the arg-maximum

static long long al_launches = 0;       // launches so far (a2s_align_launches: the tests' proof of the path)

// n_done (decode loop, greedy calls): every row has shown <eos>, the step's attention launch was a no-op and left the previous step's weights behind
__global__ __launch_bounds__(256) void attn_align_rows(const float* __restrict__ a, long ldw, int R, int T, int* __restrict__ peak,
                                                       float* __restrict__ weight, float* __restrict__ centroid, long out_stride,
                                                       const int* __restrict__ n_done, int n_rows_total) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    if (n_done && *n_done >= n_rows_total) return;
    const float* w = a + (long)row * ldw;
    float m = -INFINITY, c = 0.f;
    int mi = AL_NONE;
    for (int t = lane; t < T; t += 64) {
        const float x = w[t];
        if (x > m) { m = x; mi = t; }
        c = fmaf((float)t, x, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64); const int oi = __shfl_xor(mi, o, 64);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    c = wave_sum(c);
    if (lane == 0) {
        const int p = mi != AL_NONE ? mi : 0;            // (a row without one ordered value: frame 0, never an index outside the row)
        peak[(long)row * out_stride] = p;
        weight[(long)row * out_stride] = w[p];
        centroid[(long)row * out_stride] = c;
    }
}

int a2s_attn_align_rows_impl(hipStream_t st, const float* attw, long ldw, int R, int T, int* peak_out, float* weight_out, float* centroid_out,
                             long out_stride, const int* n_done, int n_rows_total) {
    A2S_REQUIRE(attw && peak_out && weight_out && centroid_out, "attn_align_rows: null weights or outputs");
    A2S_REQUIRE(R >= 0 && T >= 1 && ldw >= T && out_stride >= 1, "attn_align_rows: needs R >= 0, T >= 1, a row stride >= T and an output stride >= 1 (got R = %d, T = %d, ldw = %ld, out_stride = %ld)",
                R, T, ldw, out_stride);
    if (R == 0) return A2S_OK;
    hipLaunchKernelGGL(attn_align_rows, dim3(a2s_cdiv(R, 4)), dim3(256), 0, st, attw, ldw, R, T, peak_out, weight_out, centroid_out, out_stride, n_done, n_rows_total);
    A2S_CHECK_LAUNCH("attn_align_rows");
    __atomic_fetch_add(&al_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_align_launches_impl(void) { return (int)__atomic_load_n(&al_launches, __ATOMIC_RELAXED); }
