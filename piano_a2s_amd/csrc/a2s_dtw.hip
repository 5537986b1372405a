// Dynamic time warping of two feature tensors, segment by segment: where inside its bar the resynthesis of a decoded score is
// heard in the recording (piano_a2s_amd/resynth.py).  The layout is a2s_segment_agreement's: x and y hold B clips of T rows of F floats, clip b at
// + b * clip_stride; a segment [clip, f0, f1, r] is the rows [f0, f1) of one clip, the SAME rows in both tensors, n = f1 - f0 of them, and r is the
// Sakoe-Chiba half-width: cell (i, j), 0 <= i, j < n, is inside the band when |i - j| <= r; r < 0 or r >= n: no band.  tests/dtw_oracle.py states both
// stages in float64 and restates them in numpy float32.
//
// The segment's block of the cost buffer and of the direction workspace (one float / one byte per cell, the same index in both) starts at
// s * n_max * w_max, w_max = n_max where r_max < 0 and min(n_max, 2 r_max + 1) otherwise, and holds
//     W = 2 r + 1 < n (a band narrower than the square):  n rows of W cells, cell (i, j) at i * W + (j - i + r)   ("banded");
//     otherwise:                                           n rows of n cells, cell (i, j) at i * n + j             ("dense"; with 0 <= r < n the cells
//                                                          outside the band are neither written nor read).
// A segment that does not fit (n > n_max or W > w_max) is treated as empty, like a clip outside [0, B) and an empty range.
//
// dtw_cost: d[i][j] = sum_f e^2, e = (x[f0 + i][f] - y[f0 + j][f]) - off[s]: one fp32 chain per cell, f ascending, acc = fmaf(e, e, acc); two
//     subtractions and one FMA per term.  A workgroup of DC_THREADS owns a tile of DC_TILE x DC_TILE cells and walks F in chunks of DC_KC: the chunk's
//     DC_TILE rows of x and of y sit in LDS, row-major with a row of DC_LD = DC_KC + 4 floats, and the next chunk's rows are already on their way into
//     registers while this one is computed.  A thread keeps 4 x 4 cells, rows ty + 16 a and columns tx + 16 b: its 16-byte LDS reads of x are
//     broadcasts (four addresses per wave), those of y hit 16 rows DC_LD floats apart = 9 sixteen-byte slots, distinct mod 16: no bank conflict.
//     Per four terms a thread issues 8 ds_read_b128 for 192 vector operations.  Tiles wholly outside the segment or its band leave at once.
//     The grid is one-dimensional, ns segments x gx tiles; a workgroup's tile number is permuted so that the workgroups of one L2 (b, b + 8, ...)
//     walk consecutive tiles -- the tiles of a segment read the same rows.  The permutation is a bijection and changes no result.
//     Bounds.  Loads: columns [k, k + 4) (or single floats) with k < F of rows f0 + i, i < n, of clip `clip` in [0, B): inside the clip's T * F cells.
//     Stores: cells of the segment's own block only, i, j < n and inside the band.  LDS: rows < DC_TILE, columns < DC_KC.
// dtw_path: D[0][0] = d[0][0], D[i][j] = d[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) over the predecessors that exist and lie in the band, the
//     first of equals in that order (code 0, 1, 2): one fp32 addition per cell, nothing to contract.  One workgroup of DP_THREADS per segment walks the
//     anti-diagonals i + j = 0 .. 2 n - 2; the cells of a diagonal are independent, a thread takes every DP_THREADS-th of them, and the last three
//     diagonals of D live in LDS, indexed by i (slot = diagonal mod 3): one barrier per diagonal.  The cost of the thread's first cell of the NEXT
//     diagonal is loaded before the barrier.  The direction byte of every cell goes to the workspace.  Behind the last barrier thread 0 walks back from
//     (n - 1, n - 1), writing the cells in descending order into the LDS that D has left; a code read from memory is clamped to 0 .. 2, forced at the
//     edges (i = 0: left, j = 0: up) and replaced by the diagonal where it would leave the band, and the walk stops after 2 n - 1 cells whatever the
//     workspace holds.  Then all threads write the path in ascending order.
//     Bounds.  Loads and stores of cost and workspace: cells of the segment's own block, inside the band.  LDS: D slots [0, n) x 3 <= 3 n_max floats,
//     the path 2 n - 1 <= 3 n_max ints.  Stores: path[s * (2 n_max - 1) + k], k < steps <= 2 n - 1; steps[s]; total[s].
// Nothing is allocated, nothing synchronises with the host, nothing is read back; no atomics.  A segment's bits depend on its own rows, n, r, F and
// the alignment class alone.
#include "a2s_internal.h"

#define DC_THREADS 256
#define DC_TILE 64
#define DC_KC 32
#define DC_LD (DC_KC + 4)
#define DC_BATCH 32768             // segments per launch of dtw_cost: at most 4096 tiles each, a grid below 2^27 workgroups
#define DC_XCDS 8
#define DP_THREADS 256
#define DTW_T_MAX 4096

static long long dtw_launches = 0;

// segment s: n (0: nothing to do), its first row, r (-1: no band) and the width W of a row of its block
__device__ __forceinline__ int dtw_segment(const int* __restrict__ seg, long s, int B, int T, int n_max, int w_max, int* clip, int* first, int* r, int* W) {
    const int c = seg[4 * s];
    int f0 = seg[4 * s + 1], f1 = seg[4 * s + 2], rr = seg[4 * s + 3];
    f0 = f0 < 0 ? 0 : (f0 > T ? T : f0);
    f1 = f1 < 0 ? 0 : (f1 > T ? T : f1);
    const int n = f1 - f0;
    if (c < 0 || c >= B || n <= 0) return 0;
    if (rr < 0 || rr >= n) rr = -1;
    const int w = (rr >= 0 && 2 * rr + 1 < n) ? 2 * rr + 1 : n;
    if (n > n_max || w > w_max) return 0;
    *clip = c;
    *first = f0;
    *r = rr;
    *W = w;
    return n;
}
__device__ __forceinline__ long dtw_cell(int i, int j, int n, int r, int W) { return W < n ? (long)i * W + (j - i + r) : (long)i * n + j; }
__device__ __forceinline__ bool dtw_in_band(int i, int j, int r) { return r < 0 || (i > j ? i - j : j - i) <= r; }

template <int VEC>
__device__ __forceinline__ f32x4 dc_load(const float* __restrict__ row, int k, int F, bool live) {
    f32x4 v = f32x4(0.f);
    if (!live) return v;
    if constexpr (VEC == 4) {
        if (k < F) v = *reinterpret_cast<const f32x4*>(row + k);          // F % 4 == 0: the four floats are inside the row or outside it
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < F) v[e] = row[k + e];
    }
    return v;
}

template <bool OFF, int NK>
__device__ __forceinline__ void dc_terms(const f32x4 (&xa)[4], const f32x4 (&yb)[4], float o, float (&acc)[4][4]) {
#pragma unroll
    for (int e = 0; e < NK; ++e)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                float d = __fsub_rn(xa[a][e], yb[b][e]);
                if (OFF) d = __fsub_rn(d, o);
                acc[a][b] = fmaf(d, d, acc[a][b]);
            }
}

template <int VEC, bool OFF>
__global__ __launch_bounds__(DC_THREADS) void dtw_cost(const float* __restrict__ x, const float* __restrict__ y, long clip_stride, int B, int T, int F,
                                                       const int* __restrict__ seg, int s0, const float* __restrict__ off, int n_max, int w_max, int nt,
                                                       int bwt, int gx, float* __restrict__ cost) {
    __shared__ __attribute__((aligned(16))) float xs[DC_TILE * DC_LD];
    __shared__ __attribute__((aligned(16))) float ys[DC_TILE * DC_LD];
    const int tid = threadIdx.x;
    // Workgroups are dealt round-robin over the DC_XCDS L2s; the tiles of a segment read the same rows.  Workgroup b therefore takes the tile
    // number `at` of the launch such that the workgroups b, b + 8, b + 16, ... (one L2) walk a contiguous eighth of the tiles: a bijection.
    const int total = gridDim.x, q = total / DC_XCDS, rem = total % DC_XCDS;
    const int xcd = blockIdx.x % DC_XCDS;
    const int at = xcd * q + (xcd < rem ? xcd : rem) + (int)(blockIdx.x / DC_XCDS);
    const long s = (long)s0 + at / gx;
    const int tile = at % gx;
    int ti, tj;
    if (bwt < 0) {
        ti = tile / nt;
        tj = tile % nt;
    } else {                                                              // only the tile diagonals a band of r_max can reach
        const int wt = 2 * bwt + 1;
        ti = tile / wt;
        tj = ti + tile % wt - bwt;
        if (tj < 0 || tj >= nt) return;
    }
    int clip, f0, r, W;
    const int n = dtw_segment(seg, s, B, T, n_max, w_max, &clip, &f0, &r, &W);
    const int i0 = ti * DC_TILE, j0 = tj * DC_TILE;
    if (i0 >= n || j0 >= n) return;                                       // (the whole workgroup, before any barrier)
    if (r >= 0 && (i0 > j0 ? i0 - (j0 + DC_TILE - 1) : j0 - (i0 + DC_TILE - 1)) > r) return;
    const float o = OFF ? off[s] : 0.f;
    const float* __restrict__ xc = x + (long)clip * clip_stride + (long)f0 * F;
    const float* __restrict__ yc = y + (long)clip * clip_stride + (long)f0 * F;

    // staging: thread -> two (row, 4 columns) of each operand per chunk
    const int srow = tid >> 3, sk = (tid & 7) * 4;
    const bool xl0 = i0 + srow < n, xl1 = i0 + srow + 32 < n, yl0 = j0 + srow < n, yl1 = j0 + srow + 32 < n;
    const float* xr0 = xc + (long)(i0 + srow) * F;
    const float* xr1 = xc + (long)(i0 + srow + 32) * F;
    const float* yr0 = yc + (long)(j0 + srow) * F;
    const float* yr1 = yc + (long)(j0 + srow + 32) * F;
    f32x4 gx0 = dc_load<VEC>(xr0, sk, F, xl0), gx1 = dc_load<VEC>(xr1, sk, F, xl1);
    f32x4 gy0 = dc_load<VEC>(yr0, sk, F, yl0), gy1 = dc_load<VEC>(yr1, sk, F, yl1);

    const int ty = tid >> 4, tx = tid & 15;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;

    for (int k0 = 0; k0 < F; k0 += DC_KC) {
        *reinterpret_cast<f32x4*>(xs + srow * DC_LD + sk) = gx0;
        *reinterpret_cast<f32x4*>(xs + (srow + 32) * DC_LD + sk) = gx1;
        *reinterpret_cast<f32x4*>(ys + srow * DC_LD + sk) = gy0;
        *reinterpret_cast<f32x4*>(ys + (srow + 32) * DC_LD + sk) = gy1;
        __syncthreads();
        if (k0 + DC_KC < F) {                                             // the next chunk, in flight during this one's arithmetic
            const int k = k0 + DC_KC + sk;
            gx0 = dc_load<VEC>(xr0, k, F, xl0);
            gx1 = dc_load<VEC>(xr1, k, F, xl1);
            gy0 = dc_load<VEC>(yr0, k, F, yl0);
            gy1 = dc_load<VEC>(yr1, k, F, yl1);
        }
        const int kc = F - k0 < DC_KC ? F - k0 : DC_KC;                   // the terms of this chunk: exactly F in all, no padding term
        if (kc == DC_KC) {
#pragma unroll 2
            for (int k4 = 0; k4 < DC_KC; k4 += 4) {
                f32x4 xa[4], yb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    xa[a] = *reinterpret_cast<const f32x4*>(xs + (ty + 16 * a) * DC_LD + k4);
                    yb[a] = *reinterpret_cast<const f32x4*>(ys + (tx + 16 * a) * DC_LD + k4);
                }
                dc_terms<OFF, 4>(xa, yb, o, acc);
            }
        } else {
            for (int k4 = 0; k4 < kc; k4 += 4) {
                f32x4 xa[4], yb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    xa[a] = *reinterpret_cast<const f32x4*>(xs + (ty + 16 * a) * DC_LD + k4);
                    yb[a] = *reinterpret_cast<const f32x4*>(ys + (tx + 16 * a) * DC_LD + k4);
                }
                const int nk = kc - k4;
                if (nk >= 4) dc_terms<OFF, 4>(xa, yb, o, acc);
                else if (nk == 3) dc_terms<OFF, 3>(xa, yb, o, acc);
                else if (nk == 2) dc_terms<OFF, 2>(xa, yb, o, acc);
                else dc_terms<OFF, 1>(xa, yb, o, acc);
            }
        }
        __syncthreads();                                                  // (the tiles are rewritten by the next chunk)
    }

    float* __restrict__ cs = cost + s * ((long)n_max * w_max);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + ty + 16 * a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + tx + 16 * b;
            if (i < n && j < n && dtw_in_band(i, j, r)) cs[dtw_cell(i, j, n, r, W)] = acc[a][b];
        }
    }
}

// the cells of anti-diagonal d inside the band: i in [lo, hi]; lo > hi where there is none (r = 0 and d odd)
__device__ __forceinline__ void dp_range(int d, int n, int r, int* lo, int* hi) {
    int l = d - (n - 1) > 0 ? d - (n - 1) : 0, h = d < n - 1 ? d : n - 1;
    if (r >= 0) {
        const int bl = d - r > 0 ? (d - r + 1) >> 1 : 0, bh = (d + r) >> 1;
        l = l > bl ? l : bl;
        h = h < bh ? h : bh;
    }
    *lo = l;
    *hi = h;
}

__global__ __launch_bounds__(DP_THREADS) void dtw_path(const int* __restrict__ seg, int B, int T, int n_max, int w_max, const float* __restrict__ cost,
                                                       unsigned char* __restrict__ ws, int* __restrict__ path, int* __restrict__ steps,
                                                       float* __restrict__ total) {
    extern __shared__ __attribute__((aligned(16))) float dp_lds[];        // 3 n_max floats: the live diagonals of D, then the path
    __shared__ int dp_steps;
    const int tid = threadIdx.x;
    const long s = blockIdx.x;
    int clip, f0, r, W;
    const int n = dtw_segment(seg, s, B, T, n_max, w_max, &clip, &f0, &r, &W);
    if (n == 0) {
        if (tid == 0) {
            steps[s] = 0;
            total[s] = 0.f;
        }
        return;
    }
    const float* __restrict__ cs = cost + s * ((long)n_max * w_max);
    unsigned char* wsr = ws + s * ((long)n_max * w_max);
    float* Dc = dp_lds;                      // diagonal d
    float* D1 = dp_lds + n_max;              // diagonal d - 1
    float* D2 = dp_lds + 2 * (long)n_max;    // diagonal d - 2

    float pre = tid == 0 ? cs[dtw_cell(0, 0, n, r, W)] : 0.f;
    const int last = 2 * n - 2;
    for (int d = 0; d <= last; ++d) {
        int lo, hi;
        dp_range(d, n, r, &lo, &hi);
        for (int i = lo + tid; i <= hi; i += DP_THREADS) {
            const int j = d - i;
            const long at = dtw_cell(i, j, n, r, W);
            const float c = i == lo + tid ? pre : cs[at];
            float best = 0.f;
            int code = 0;
            bool have = false;
            if (i > 0 && j > 0) {                                         // (the diagonal step keeps i - j: inside the band)
                best = D2[i - 1];
                have = true;
            }
            if (i > 0 && dtw_in_band(i - 1, j, r)) {
                const float v = D1[i - 1];
                if (!have || v < best) {
                    best = v;
                    code = 1;
                    have = true;
                }
            }
            if (j > 0 && dtw_in_band(i, j - 1, r)) {
                const float v = D1[i];
                if (!have || v < best) {
                    best = v;
                    code = 2;
                    have = true;
                }
            }
            const float v = have ? __fadd_rn(c, best) : c;
            Dc[i] = v;
            wsr[at] = (unsigned char)code;
            if (d == last) total[s] = v;
        }
        if (d < last) {                                                   // this thread's first cell of the next diagonal
            int l2, h2;
            dp_range(d + 1, n, r, &l2, &h2);
            const int i = l2 + tid;
            if (i <= h2) pre = cs[dtw_cell(i, d + 1 - i, n, r, W)];
        }
        __syncthreads();
        float* t = D2;
        D2 = D1;
        D1 = Dc;
        Dc = t;
    }

    int* rev = reinterpret_cast<int*>(dp_lds);                            // D is dead: 2 n - 1 <= 3 n_max ints
    if (tid == 0) {
        int i = n - 1, j = n - 1, k = 0;
        rev[k++] = (i << 16) | j;
        while ((i > 0 || j > 0) && k < 2 * n - 1) {
            int code = wsr[dtw_cell(i, j, n, r, W)];
            code = code > 2 ? 0 : code;
            if (i == 0) code = 2;
            else if (j == 0) code = 1;
            else if (code == 1 && !dtw_in_band(i - 1, j, r)) code = 0;
            else if (code == 2 && !dtw_in_band(i, j - 1, r)) code = 0;
            if (code != 2) --i;
            if (code != 1) --j;
            rev[k++] = (i << 16) | j;
        }
        dp_steps = k;
        steps[s] = k;
    }
    __syncthreads();
    const int k = dp_steps;
    int* __restrict__ out = path + s * (2L * n_max - 1);
    for (int t = tid; t < k; t += DP_THREADS) out[t] = rev[k - 1 - t];
}

static long dtw_w_max(int n_max, int r_max) { return r_max < 0 || 2L * r_max + 1 > n_max ? n_max : 2L * r_max + 1; }

size_t a2s_dtw_cost_bytes_impl(int S, int n_max, int r_max) {
    if (S < 0 || n_max < 0) return 0;
    return (size_t)S * (size_t)n_max * (size_t)dtw_w_max(n_max, r_max) * sizeof(float);
}
size_t a2s_dtw_workspace_bytes_impl(int S, int n_max, int r_max) {
    if (S < 0 || n_max < 0) return 0;
    return (size_t)S * (size_t)n_max * (size_t)dtw_w_max(n_max, r_max);
}

int a2s_dtw_cost_impl(hipStream_t st, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* seg, int S, const float* off,
                      int n_max, int r_max, float* cost, size_t cost_bytes) {
    A2S_REQUIRE(x && y && seg && cost, "dtw_cost: null x, y, segment table or cost buffer");
    A2S_REQUIRE(B >= 1 && T >= 1 && F >= 1, "dtw_cost: needs B, T, F >= 1 (got B = %d, T = %d, F = %d)", B, T, F);
    A2S_REQUIRE(T <= DTW_T_MAX, "dtw_cost: needs T <= %d (got %d)", DTW_T_MAX, T);
    A2S_REQUIRE(S >= 0, "dtw_cost: needs S >= 0 (got %d)", S);
    A2S_REQUIRE(clip_stride >= (long)T * F, "dtw_cost: clips %ld floats apart overlap (T * F = %ld)", clip_stride, (long)T * F);
    A2S_REQUIRE(n_max >= 1 && n_max <= T, "dtw_cost: needs 1 <= n_max <= T = %d (got %d)", T, n_max);
    A2S_REQUIRE(cost_bytes >= a2s_dtw_cost_bytes_impl(S, n_max, r_max), "dtw_cost: the cost buffer holds %zu bytes, %zu are needed", cost_bytes,
                a2s_dtw_cost_bytes_impl(S, n_max, r_max));
    if (S == 0) return A2S_OK;
    const bool vec = F % 4 == 0 && clip_stride % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const int w_max = (int)dtw_w_max(n_max, r_max);
    const int nt = a2s_cdiv(n_max, DC_TILE);
    // a segment that fits has |i - j| <= w_max - 1 in every cell it owns (banded: r <= (w_max - 1) / 2; dense: n <= w_max): the tile diagonals
    // |ti - tj| <= reach hold them all; where that is fewer workgroups than the square, only those are launched
    const int reach = (w_max - 1 + DC_TILE - 1) / DC_TILE;
    const int bwt = 2 * reach + 1 < nt ? reach : -1;
    const int gx = bwt < 0 ? nt * nt : nt * (2 * bwt + 1);
    for (int s0 = 0; s0 < S; s0 += DC_BATCH) {
        const int ns = S - s0 < DC_BATCH ? S - s0 : DC_BATCH;
#define DC_LAUNCH(VEC, OFF)                                                                                                                             \
    hipLaunchKernelGGL((dtw_cost<VEC, OFF>), dim3(gx * ns), dim3(DC_THREADS), 0, st, x, y, clip_stride, B, T, F, seg, s0, off, n_max, w_max, nt, bwt, gx, cost)
        if (vec && off) DC_LAUNCH(4, true);
        else if (vec) DC_LAUNCH(4, false);
        else if (off) DC_LAUNCH(1, true);
        else DC_LAUNCH(1, false);
#undef DC_LAUNCH
        A2S_CHECK_LAUNCH("dtw_cost");
        __atomic_fetch_add(&dtw_launches, 1LL, __ATOMIC_RELAXED);
    }
    return A2S_OK;
}

int a2s_dtw_path_impl(hipStream_t st, const int* seg, int S, int B, int T, int n_max, int r_max, const float* cost, size_t cost_bytes, unsigned char* ws,
                      size_t ws_bytes, int* path, int* steps, float* total) {
    A2S_REQUIRE(seg && cost && ws && path && steps && total, "dtw_path: null segment table, cost buffer, workspace, path, steps or total");
    A2S_REQUIRE(B >= 1 && T >= 1, "dtw_path: needs B, T >= 1 (got B = %d, T = %d)", B, T);
    A2S_REQUIRE(T <= DTW_T_MAX, "dtw_path: needs T <= %d (got %d)", DTW_T_MAX, T);
    A2S_REQUIRE(S >= 0, "dtw_path: needs S >= 0 (got %d)", S);
    A2S_REQUIRE(n_max >= 1 && n_max <= T, "dtw_path: needs 1 <= n_max <= T = %d (got %d)", T, n_max);
    A2S_REQUIRE(cost_bytes >= a2s_dtw_cost_bytes_impl(S, n_max, r_max), "dtw_path: the cost buffer holds %zu bytes, %zu are needed", cost_bytes,
                a2s_dtw_cost_bytes_impl(S, n_max, r_max));
    A2S_REQUIRE(ws_bytes >= a2s_dtw_workspace_bytes_impl(S, n_max, r_max), "dtw_path: the workspace holds %zu bytes, %zu are needed", ws_bytes,
                a2s_dtw_workspace_bytes_impl(S, n_max, r_max));
    if (S == 0) return A2S_OK;
    const int w_max = (int)dtw_w_max(n_max, r_max);
    hipLaunchKernelGGL(dtw_path, dim3(S), dim3(DP_THREADS), (size_t)3 * n_max * sizeof(float), st, seg, B, T, n_max, w_max, cost, ws, path, steps, total);
    A2S_CHECK_LAUNCH("dtw_path");
    __atomic_fetch_add(&dtw_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_dtw_launches_impl(void) { return (int)__atomic_load_n(&dtw_launches, __ATOMIC_RELAXED); }
