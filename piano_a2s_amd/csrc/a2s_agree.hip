// Agreement of two feature tensors, segment by segment: the five sums a Pearson correlation needs, over the cells of each
// segment = a run of rows [f0, f1) of one clip.  x and y hold B clips of T rows of F floats; rows are contiguous, so a segment is ONE contiguous run
// of n = (f1 - f0) * F cells that starts at clip * clip_stride + f0 * F, the same in both tensors.  A streaming reduction: every cell is read once.
//
// The split, which fixes the order of summation and depends on nothing but the segment's own n (not on S, on the segment's place in the table, on B
// or on T):
//     chunk c        = the cells [c * AG_CHUNK, min(n, (c + 1) * AG_CHUNK)) of the run, one workgroup of AG_THREADS lanes at a time;
//     lane partial   = fp32, over the lane's at most AG_CHUNK / AG_THREADS = 32 cells of the chunk, in ascending cell order
//                      (16-byte path: the lane's float4 number i is cells 4 (lane + 256 i) .. + 3; scalar path: cell lane + 256 i);
//     P_c            = the 256 lane partials as doubles, summed by a fixed tree (six DPP steps per wave, then ((w0 + w1) + (w2 + w3)));
//     slot j < 64    = P_j + P_(j + 64) + P_(j + 128) + ... in ascending order (double; one workgroup owns the slot and walks its chunks);
//     out            = slot 0 + slot 1 + ... over the slots the segment has, ascending (double; agree_finish, a second small launch).
// So a recording's handful of bars still spreads over up to 64 workgroups each, and no float is ever added atomically.
// The slots live in a device array of the library's own (AG_BATCH segments x 64 slots x 5 doubles): the entry point allocates nothing and takes no
// workspace, and longer tables run as several launch pairs on the same stream.  Calls that could overlap on DIFFERENT streams would share that
// array: the library's rule is one host thread and ordering by stream (include/a2s.h), and the Python side issues these calls on one stream.
//
// Bounds.  clip outside [0, B): n = 0.  f0, f1 clamped to [0, T]; f1 <= f0: n = 0.  Loads: cells [start, start + n) of x and of y only, inside the clip's
// T * F cells (the stride padding is never read).  Stores: slots of segment rows < AG_BATCH, lanes j < 64; out[5 s .. 5 s + 4] for s < S.
// 16-byte loads where F % 4 == 0, clip_stride % 4 == 0 and both bases are 16-byte aligned (every run then starts and ends on a 16-byte boundary);
// 4-byte loads otherwise.
#include "a2s_internal.h"

#define AG_THREADS 256
#define AG_CHUNK 8192
#define AG_SLOTS 64
#define AG_BATCH 2048
#define AG_PER_LANE (AG_CHUNK / AG_THREADS)          // 32 cells per fp32 partial

__device__ double ag_slots[(long)AG_BATCH * AG_SLOTS * 5];
static long long agree_launches = 0;

// the run of segment s: first cell and number of cells (0: nothing to read)
__device__ __forceinline__ long ag_segment(const int* __restrict__ seg, int s, long clip_stride, int B, int T, int F, long* start) {
    const int clip = seg[4 * (long)s];
    int f0 = seg[4 * (long)s + 1], f1 = seg[4 * (long)s + 2];
    f0 = f0 < 0 ? 0 : (f0 > T ? T : f0);
    f1 = f1 < 0 ? 0 : (f1 > T ? T : f1);
    if (clip < 0 || clip >= B || f1 <= f0) { *start = 0; return 0; }
    *start = (long)clip * clip_stride + (long)f0 * F;
    return (long)(f1 - f0) * F;
}

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double ag_dpp_take(double v) {          // the double of the lane CTRL names; +0.0 where there is none
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}
// sum over the 64 lanes in double, valid in lane 63 only (the tree of wave_sum_lane63, a2s_common.h)
__device__ __forceinline__ double ag_wave_sum_lane63(double v) {
    v += ag_dpp_take<A2S_DPP_QUAD_1032>(v);
    v += ag_dpp_take<A2S_DPP_QUAD_2301>(v);
    v += ag_dpp_take<A2S_DPP_ROW_HALF_MIRROR>(v);
    v += ag_dpp_take<A2S_DPP_ROW_MIRROR>(v);
    v += ag_dpp_take<A2S_DPP_ROW_BCAST15, 0xA>(v);
    v += ag_dpp_take<A2S_DPP_ROW_BCAST31, 0xC>(v);
    return v;
}

__device__ __forceinline__ void ag_cell(float a, float b, float* p) {
    p[0] += a;
    p[1] += b;
    p[2] += a * a;
    p[3] += b * b;
    p[4] += a * b;
}

template <int VEC>
__global__ __launch_bounds__(AG_THREADS) void agree_partial(const float* __restrict__ x, const float* __restrict__ y, long clip_stride, int B, int T, int F,
                                                            const int* __restrict__ seg, int s0) {
    __shared__ double red[AG_THREADS / A2S_WAVE][5];
    const int s = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
    long start;
    const long n = ag_segment(seg, s0 + s, clip_stride, B, T, F, &start);
    const long nchunks = (n + AG_CHUNK - 1) / AG_CHUNK;
    if (j >= nchunks) return;                                   // (the whole workgroup: agree_finish reads the slots j < nchunks only)
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                  // the slot, in thread 0
    for (long c = j; c < nchunks; c += AG_SLOTS) {
        const long c0 = c * AG_CHUNK;
        const int len = n - c0 < AG_CHUNK ? (int)(n - c0) : AG_CHUNK;
        const float* xp = x + start + c0;
        const float* yp = y + start + c0;
        float p[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if constexpr (VEC == 4) {
            f32x4 a[AG_PER_LANE / 4], b[AG_PER_LANE / 4];
#pragma unroll
            for (int i = 0; i < AG_PER_LANE / 4; ++i) {
                const int k = (tid + i * AG_THREADS) * 4;       // len % 4 == 0: a float4 is inside the run or outside it
                a[i] = f32x4(0.f);
                b[i] = f32x4(0.f);
                if (k < len) {
                    a[i] = ld_kv<true>(xp + k);
                    b[i] = ld_kv<true>(yp + k);
                }
            }
#pragma unroll
            for (int i = 0; i < AG_PER_LANE / 4; ++i) {
                if ((tid + i * AG_THREADS) * 4 < len) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) ag_cell(a[i][e], b[i][e], p);
                }
            }
        } else {
#pragma unroll 8
            for (int i = 0; i < AG_PER_LANE; ++i) {
                const int k = tid + i * AG_THREADS;
                if (k < len) ag_cell(xp[k], yp[k], p);
            }
        }
#pragma unroll
        for (int v = 0; v < 5; ++v) {
            const double w = ag_wave_sum_lane63((double)p[v]);
            if ((tid & (A2S_WAVE - 1)) == A2S_WAVE - 1) red[tid / A2S_WAVE][v] = w;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int v = 0; v < 5; ++v) acc[v] += (red[0][v] + red[1][v]) + (red[2][v] + red[3][v]);
        }
        __syncthreads();                                        // (red is rewritten by the slot's next chunk)
    }
    if (tid == 0) {
        double* slot = ag_slots + ((long)s * AG_SLOTS + j) * 5;
#pragma unroll
        for (int v = 0; v < 5; ++v) slot[v] = acc[v];
    }
}

__global__ __launch_bounds__(AG_THREADS) void agree_finish(long clip_stride, int B, int T, int F, const int* __restrict__ seg, int s0, int ns,
                                                           double* __restrict__ out) {
    const int idx = blockIdx.x * AG_THREADS + threadIdx.x;
    if (idx >= ns * 5) return;
    const int s = idx / 5, v = idx - 5 * s;
    long start;
    const long n = ag_segment(seg, s0 + s, clip_stride, B, T, F, &start);
    const long nchunks = (n + AG_CHUNK - 1) / AG_CHUNK;
    const int nslots = nchunks < AG_SLOTS ? (int)nchunks : AG_SLOTS;
    double a = 0.0;
    for (int j = 0; j < nslots; ++j) a += ag_slots[((long)s * AG_SLOTS + j) * 5 + v];
    out[(long)(s0 + s) * 5 + v] = a;
}

int a2s_segment_agreement_impl(hipStream_t st, const float* x, const float* y, long clip_stride, int B, int T, int F, const int* seg, int S, double* out) {
    A2S_REQUIRE(x && y && seg && out, "segment_agreement: null x, y, segment table or output");
    A2S_REQUIRE(B >= 1 && T >= 1 && F >= 1, "segment_agreement: needs B, T, F >= 1 (got B = %d, T = %d, F = %d)", B, T, F);
    A2S_REQUIRE(S >= 0, "segment_agreement: needs S >= 0 (got %d)", S);
    A2S_REQUIRE(clip_stride >= (long)T * F, "segment_agreement: clips %ld floats apart overlap (T * F = %ld)", clip_stride, (long)T * F);
    if (S == 0) return A2S_OK;
    const bool vec = F % 4 == 0 && clip_stride % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const long most = ((long)T * F + AG_CHUNK - 1) / AG_CHUNK;          // chunks of the longest possible run
    const int G = most < AG_SLOTS ? (int)most : AG_SLOTS;
    for (int s0 = 0; s0 < S; s0 += AG_BATCH) {
        const int ns = S - s0 < AG_BATCH ? S - s0 : AG_BATCH;
        if (vec) hipLaunchKernelGGL(agree_partial<4>, dim3(G, ns), dim3(AG_THREADS), 0, st, x, y, clip_stride, B, T, F, seg, s0);
        else hipLaunchKernelGGL(agree_partial<1>, dim3(G, ns), dim3(AG_THREADS), 0, st, x, y, clip_stride, B, T, F, seg, s0);
        A2S_CHECK_LAUNCH("agree_partial");
        hipLaunchKernelGGL(agree_finish, dim3(a2s_cdiv(5L * ns, AG_THREADS)), dim3(AG_THREADS), 0, st, clip_stride, B, T, F, seg, s0, ns, out);
        A2S_CHECK_LAUNCH("agree_finish");
        __atomic_fetch_add(&agree_launches, 2LL, __ATOMIC_RELAXED);
    }
    return A2S_OK;
}

int a2s_agreement_launches_impl(void) { return (int)__atomic_load_n(&agree_launches, __ATOMIC_RELAXED); }
int a2s_agreement_partial_cells_impl(void) { return AG_PER_LANE; }
