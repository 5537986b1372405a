// Resynthesis at the performed timing: the two device stages between the DTW paths of a round and its next render.  Integers
// only: the device EQUALS tests/retime_oracle.py.
//
// path_warp: the doubled warp of every segment from its path.  Table row s = [clip, f0, f1, r]; n = f1 - f0, read as 0 where it is outside
// [0, n_max].  The path row holds steps[s] cells (i << 16) | j, i the recording's frame and j the score's.  The path is taken only if
// n <= steps <= min(2 n - 1, path_stride), its first cell is (0, 0), its last (n - 1, n - 1) and every step is (1, 1), (1, 0) or (0, 1); then every
// column and every row has exactly one first and one last cell (the one whose predecessor / successor lies in another column / row), and
//     warp2[j] = first i + last i of column j (j < n),   warp2[n] = warp2[n - 1] + 2,   warp2[j] = 2 j behind n;   inverse2 the same over the rows.
// Any other path, steps <= 0 and n = 0 give the identity 2 j over the whole row.  One workgroup per segment; the first and last cells go to four
// 16-bit LDS arrays (4096 * 4 * 2 bytes; an index is below 4096), a flag in LDS collects a bad step; two barriers (the flag's reset, then the sums).
// Bounds.  Loads: table[4 s .. 4 s + 3], steps[s], path[s * path_stride + k], k < steps <= path_stride.  LDS: indices clamped to [0, n).  Stores:
// warp2 / inverse2 [s * (n_max + 1) + j], j <= n_max.
//
// retime_events: one thread per event row [clip, prog_row, seg, bar_start, bar_stop, 0, 0, 0]; words 0 (onset) and 1 (length) of row prog_row of the
// clip's program are moved through the segment's warp2 (include/a2s.h states the rule).  Bounds.  Loads: events[8 e .. 8 e + 4]; table[4 seg + 1],
// [4 seg + 2] with seg in [0, S); warp2[seg * (n_max + 1) + k], k + 1 <= n <= n_max; words 0 and 1 of the program row.  Stores: those two words, and
// only where clip is in [0, B) and 1 <= prog_row < program_rows (the header and the other clips' programs cannot be reached).
#include "a2s_internal.h"

#define RT_THREADS 256
#define RT_N_MAX 4096                               // frames per segment at the most (the DTW's limit; an index fits 16 bits)

static long long retime_launches = 0;

__global__ __launch_bounds__(RT_THREADS) void path_warp(const int* __restrict__ paths, long path_stride, const int* __restrict__ steps,
                                                          const int* __restrict__ table, int n_max, int* __restrict__ warp2, int* __restrict__ inverse2) {
    __shared__ unsigned short col_first[RT_N_MAX], col_last[RT_N_MAX], row_first[RT_N_MAX], row_last[RT_N_MAX];
    __shared__ int bad_step;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int* path = paths + (long)s * path_stride;
    int* w = warp2 + (long)s * (n_max + 1);
    int* v = inverse2 ? inverse2 + (long)s * (n_max + 1) : nullptr;
    const long n64 = (long)table[4 * (long)s + 2] - (long)table[4 * (long)s + 1];
    const int n = n64 < 0 || n64 > n_max ? 0 : (int)n64;
    const int k_end = steps[s];
    // what the whole workgroup sees alike: the counts and the two end cells
    bool take = n >= 1 && k_end >= n && k_end <= 2 * n - 1 && (long)k_end <= path_stride;
    if (take) take = path[0] == 0 && path[k_end - 1] == (((n - 1) << 16) | (n - 1));
    if (tid == 0) bad_step = 0;
    __syncthreads();
    if (take) {
        for (int k = tid; k < k_end; k += RT_THREADS) {
            const int c = path[k], i = c >> 16, j = c & 0xFFFF;
            const int ic = min(max(i, 0), n - 1), jc = min(max(j, 0), n - 1);          // the LDS index is in range whatever the buffer holds
            bool new_col = true, new_row = true, end_col = true, end_row = true;
            if (k > 0) {
                const int p = path[k - 1], di = i - (p >> 16), dj = j - (p & 0xFFFF);
                if (di < 0 || di > 1 || dj < 0 || dj > 1 || di + dj < 1) bad_step = 1;
                new_col = dj != 0;
                new_row = di != 0;
            }
            if (k + 1 < k_end) {
                const int q = path[k + 1];
                end_col = (q & 0xFFFF) != j;
                end_row = (q >> 16) != i;
            }
            if (new_col) col_first[jc] = (unsigned short)ic;
            if (end_col) col_last[jc] = (unsigned short)ic;
            if (new_row) row_first[ic] = (unsigned short)jc;
            if (end_row) row_last[ic] = (unsigned short)jc;
        }
    }
    __syncthreads();
    take = take && bad_step == 0;
    for (int j = tid; j <= n_max; j += RT_THREADS) {
        int a = 2 * j, b = 2 * j;
        if (take && j < n) {
            a = (int)col_first[j] + (int)col_last[j];
            b = (int)row_first[j] + (int)row_last[j];
        } else if (take && j == n) {
            a = (int)col_first[n - 1] + (int)col_last[n - 1] + 2;
            b = (int)row_first[n - 1] + (int)row_last[n - 1] + 2;
        }
        w[j] = a;
        if (v) v[j] = b;
    }
}

// move(t) of include/a2s.h: t + floor(shift2 / 2).  n >= 1; w: the segment's row of warp2.
__device__ __forceinline__ long long rt_move(long long t, const int* __restrict__ w, long long origin, int n, int hop) {
    const long long p = min(max(t - origin, 0LL), (long long)n * hop);
    const int k = min((int)(p / hop), n - 1);
    const int rem = (int)(p - (long long)k * hop);
    const int s2 = (hop - rem) * (w[k] - 2 * k) + rem * (w[k + 1] - 2 * (k + 1));
    return t + (s2 - (s2 & 1)) / 2;                                                // (s2 - (s2 & 1) is even: the division is exact, the floor towards -inf)
}

__global__ __launch_bounds__(RT_THREADS) void retime_events(const int* __restrict__ warp2, int n_max, const int* __restrict__ table, int S,
                                                              const int* __restrict__ events, int E, int hop, int* __restrict__ programs, int B,
                                                              int program_rows) {
    const int e = blockIdx.x * RT_THREADS + threadIdx.x;
    if (e >= E) return;
    const int* r = events + 8 * (long)e;
    const int clip = r[0], row = r[1], seg = r[2], bar_start = r[3], bar_stop = r[4];
    if (clip < 0 || clip >= B || row < 1 || row >= program_rows || seg < 0 || seg >= S || bar_stop <= bar_start) return;
    int* word = programs + ((long)clip * program_rows + row) * 8;
    const int onset = word[0], length = word[1];
    if (length <= 0) return;                                                       // a padding row
    const long f0 = table[4 * (long)seg + 1];
    const long n64 = (long)table[4 * (long)seg + 2] - f0;
    const int n = n64 < 0 || n64 > n_max ? 0 : (int)n64;                           // as path_warp reads it
    long long on = onset, end = (long long)onset + length;
    if (n >= 1) {
        const int* w = warp2 + (long)seg * (n_max + 1);
        const long long origin = (long long)f0 * hop;
        on = rt_move(on, w, origin, n, hop);
        end = rt_move(end, w, origin, n, hop);
    }
    on = min(min(max(on, (long long)bar_start), (long long)bar_stop), (long long)bar_stop - 1);
    end = min(max(end, (long long)bar_start), (long long)bar_stop);
    const long long len = max(1LL, min(max(end - on, (long long)hop), (long long)bar_stop - on));
    word[0] = (int)on;
    word[1] = (int)len;
}

int a2s_path_warp_impl(hipStream_t st, const int* paths, long path_stride, const int* steps, const int* table, int S, int n_max, int* warp2, int* inverse2) {
    A2S_REQUIRE(paths && steps && table && warp2, "path_warp: null paths, steps, table or warp2");
    A2S_REQUIRE(S >= 0, "path_warp: needs S >= 0 (got %d)", S);
    A2S_REQUIRE(n_max >= 1 && n_max <= RT_N_MAX, "path_warp: needs 1 <= n_max <= %d (got %d)", RT_N_MAX, n_max);
    A2S_REQUIRE(path_stride >= 1, "path_warp: needs a path stride >= 1 (got %ld)", path_stride);
    if (S == 0) return A2S_OK;
    hipLaunchKernelGGL(path_warp, dim3(S), dim3(RT_THREADS), 0, st, paths, path_stride, steps, table, n_max, warp2, inverse2);
    A2S_CHECK_LAUNCH("path_warp");
    __atomic_fetch_add(&retime_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_retime_events_impl(hipStream_t st, const int* warp2, int n_max, const int* table, int S, const int* events, int E, int hop, int* programs, int B,
                           int program_rows) {
    A2S_REQUIRE(warp2 && table && events && programs, "retime_events: null warp2, table, events or programs");
    A2S_REQUIRE(S >= 0 && E >= 0 && B >= 0 && program_rows >= 0, "retime_events: negative S, E, B or program_rows (got %d, %d, %d, %d)", S, E, B, program_rows);
    A2S_REQUIRE(n_max >= 1 && n_max <= RT_N_MAX, "retime_events: needs 1 <= n_max <= %d (got %d)", RT_N_MAX, n_max);
    A2S_REQUIRE(hop >= 1 && hop <= 65535, "retime_events: needs 1 <= hop <= 65535 (got %d)", hop);
    if (S == 0 || E == 0) return A2S_OK;
    hipLaunchKernelGGL(retime_events, dim3(a2s_cdiv(E, RT_THREADS)), dim3(RT_THREADS), 0, st, warp2, n_max, table, S, events, E, hop, programs, B, program_rows);
    A2S_CHECK_LAUNCH("retime_events");
    __atomic_fetch_add(&retime_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_retime_launches_impl(void) { return (int)__atomic_load_n(&retime_launches, __ATOMIC_RELAXED); }
