// Note dynamics by analysis by synthesis: the two device stages between the VQT of a resynthesis and its next render.
//
// note_levels: how loud a note's own partials are in the recording (x) and in the resynthesis (y).  A note row is 8 int32
// [clip, fx, fy, n, b1, b2, b3, prog_row]; its cells are the frames i < n crossed with the columns b_h - 1 .. b_h + 1 of every b_h >= 0, read at row
// fx + i of x and at row fy + i of y.  A cell counts only if its column is in [0, F) and BOTH rows are in [0, T).
//     out[s] = [sum x, sum y, count]          (three doubles)
// One wavefront per row, DY_ROWS rows per workgroup.  The order of summation is fixed by the row alone: cell k = 9 i + 3 h + c (h the partial, c the
// column b_h - 1 + c) belongs to lane k mod 64, a lane adds its cells in ascending k in double (a cell that does not count adds nothing), and the 64
// lane sums are combined by a butterfly (lane ^ 1, ^ 2, ^ 4, ^ 8, ^ 16, ^ 32: every lane ends with the same bits, because a + b = b + a).  n is read
// as min(n, DY_N_MAX): the host writes at most 12.
// Bounds.  Loads: x[clip][fx + i][col] and y[clip][fy + i][col] with clip in [0, B), both rows in [0, T), col in [0, F) only (64-bit index arithmetic;
// the stride padding is never read).  Stores: out[3 s .. 3 s + 2], s < S.
//
// note_amp_update: one workgroup per clip over the clip's rows first[b] .. first[b + 1] (at most DY_MAX_ROWS = 512; a longer run is cut there).
//     d = (float)(80.0 * (Sx - Sy) / count)   (double division; 0 where count = 0);   c = cum + d;   med = the lower median of c;
//     cum' = min(max(c - med, -30), 12);   word 3 of program row prog_row = base_amp * exp2f(cum' * (log2(10) / 20));   cum = cum'.
// fp32, one operation per step and nothing for the compiler to contract.  The median comes from rank counting in LDS: rank(j) = #{i: c_i < c_j} +
// #{i < j: c_i == c_j} is a permutation of 0 .. k - 1 whatever the ties, so exactly one row has rank (k - 1) / 2 and publishes its value.
// Bounds.  Loads: sums[3 s .. 3 s + 2], rows[8 s .. 8 s + 7], cum[s] for the clip's s; first[b], first[b + 1].  Stores: cum[s]; word 3 of row prog_row
// of clip b's program, and only where 1 <= prog_row < rows_per_clip (the header and the other clips' programs cannot be reached).
#include "a2s_internal.h"

#define DY_ROWS 4                                   // note rows (wavefronts) per workgroup of note_levels
#define DY_N_MAX 64                                 // frames per note row at the most
#define DY_THREADS 256                              // note_amp_update
#define DY_MAX_ROWS 512                             // rows per clip at the most (scoregen.MAX_EVENTS = 511)

static long long dynamics_launches = 0;

__global__ __launch_bounds__(DY_ROWS* A2S_WAVE) void note_levels(const float* __restrict__ x, const float* __restrict__ y, long clip_stride, int B, int T,
                                                                   int F, const int* __restrict__ rows, int S, double* __restrict__ out) {
    const int lane = threadIdx.x & (A2S_WAVE - 1);
    const int s = blockIdx.x * DY_ROWS + threadIdx.x / A2S_WAVE;
    if (s >= S) return;                                          // (the whole wavefront; there is no barrier in this kernel)
    const int* r = rows + 8 * (long)s;
    const int clip = r[0], fx = r[1], fy = r[2];
    int n = r[3];
    n = n > DY_N_MAX ? DY_N_MAX : n;
    double sx = 0.0, sy = 0.0, cnt = 0.0;
    if (clip >= 0 && clip < B && n > 0) {
        const float* xc = x + (long)clip * clip_stride;
        const float* yc = y + (long)clip * clip_stride;
        for (int k = lane; k < 9 * n; k += A2S_WAVE) {
            const int i = k / 9, j = k - 9 * i, h = j / 3;
            const int bin = r[4 + h];
            const long col = (long)bin - 1 + (j - 3 * h);
            const long tx = (long)fx + i, ty = (long)fy + i;
            if (bin >= 0 && col >= 0 && col < F && tx >= 0 && tx < T && ty >= 0 && ty < T) {
                sx += (double)xc[tx * F + col];
                sy += (double)yc[ty * F + col];
                cnt += 1.0;
            }
        }
    }
#pragma unroll
    for (int m = 1; m < A2S_WAVE; m <<= 1) {
        sx += __shfl_xor(sx, m, A2S_WAVE);
        sy += __shfl_xor(sy, m, A2S_WAVE);
        cnt += __shfl_xor(cnt, m, A2S_WAVE);
    }
    if (lane == 0) {
        out[3 * (long)s] = sx;
        out[3 * (long)s + 1] = sy;
        out[3 * (long)s + 2] = cnt;
    }
}

__global__ __launch_bounds__(DY_THREADS) void note_amp_update(const double* __restrict__ sums, const int* __restrict__ rows, const int* __restrict__ first,
                                                              float* __restrict__ cum, int* __restrict__ programs, int rows_per_clip, float base_amp) {
    __shared__ float c[DY_MAX_ROWS];
    __shared__ float med_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const long s0 = first[b];
    long k64 = (long)first[b + 1] - s0;
    k64 = k64 > DY_MAX_ROWS ? DY_MAX_ROWS : k64;
    const int k = (int)k64;
    if (s0 < 0 || k <= 0) return;                                // a clip with no rows is left alone (the whole workgroup returns)
    if (tid == 0) med_s = 0.f;                                   // (only a NaN among the levels leaves no row with the median's rank)
    for (int j = tid; j < k; j += DY_THREADS) {
        const double sx = sums[3 * (s0 + j)], sy = sums[3 * (s0 + j) + 1], n = sums[3 * (s0 + j) + 2];
        const float d = n > 0.0 ? (float)(80.0 * (sx - sy) / n) : 0.f;
        c[j] = cum[s0 + j] + d;
    }
    __syncthreads();
    const int want = (k - 1) / 2;
    for (int j = tid; j < k; j += DY_THREADS) {
        const float v = c[j];
        int rank = 0;
        for (int i = 0; i < k; ++i) {                            // (every lane reads the same word: a broadcast, no bank conflict)
            const float w = c[i];
            rank += (w < v) || (w == v && i < j);
        }
        if (rank == want) med_s = v;
    }
    __syncthreads();
    const float med = med_s;
    int* prog = programs + (long)b * rows_per_clip * 8;
    for (int j = tid; j < k; j += DY_THREADS) {
        const float level = fminf(fmaxf(c[j] - med, -30.f), 12.f);
        const int row = rows[8 * (s0 + j) + 7];
        if (row >= 1 && row < rows_per_clip) prog[8 * (long)row + 3] = __builtin_bit_cast(int, base_amp * exp2f(level * 0.16609640474436813f));
        cum[s0 + j] = level;
    }
}

int a2s_note_levels_impl(hipStream_t st, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* rows, int S, double* out) {
    A2S_REQUIRE(x && y && rows && out, "note_levels: null x, y, row table or output");
    A2S_REQUIRE(B >= 1 && T >= 1 && F >= 1, "note_levels: needs B, T, F >= 1 (got B = %d, T = %d, F = %d)", B, T, F);
    A2S_REQUIRE(S >= 0, "note_levels: needs S >= 0 (got %d)", S);
    A2S_REQUIRE(clip_stride >= (long)T * F, "note_levels: clips %ld floats apart overlap (T * F = %ld)", clip_stride, (long)T * F);
    if (S == 0) return A2S_OK;
    hipLaunchKernelGGL(note_levels, dim3(a2s_cdiv(S, DY_ROWS)), dim3(DY_ROWS * A2S_WAVE), 0, st, x, y, clip_stride, B, T, F, rows, S, out);
    A2S_CHECK_LAUNCH("note_levels");
    __atomic_fetch_add(&dynamics_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_note_amp_update_impl(hipStream_t st, const double* sums, const int* rows, const int* first, int B, float* cum, int* programs, int rows_per_clip,
                             float base_amp) {
    A2S_REQUIRE(sums && rows && first && cum && programs, "note_amp_update: null sums, row table, offsets, levels or programs");
    A2S_REQUIRE(B >= 1 && B <= 65535, "note_amp_update: needs 1 <= B <= 65535 (got %d)", B);
    A2S_REQUIRE(rows_per_clip >= 2, "note_amp_update: a program of %d rows has no note row", rows_per_clip);
    A2S_REQUIRE(base_amp > 0.f && base_amp <= 1e30f, "note_amp_update: needs a positive finite base amplitude (got %g)", (double)base_amp);
    hipLaunchKernelGGL(note_amp_update, dim3(B), dim3(DY_THREADS), 0, st, sums, rows, first, cum, programs, rows_per_clip, base_amp);
    A2S_CHECK_LAUNCH("note_amp_update");
    __atomic_fetch_add(&dynamics_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_dynamics_launches_impl(void) { return (int)__atomic_load_n(&dynamics_launches, __ATOMIC_RELAXED); }
