// Scoring on the device: unit-cost Levenshtein distance of many independent pairs of integer word sequences (the word error rate of the
// VALID / TEST stages, piano_a2s_amd/metrics.py).  The reference scores with jiwer.wer on the host (pretrain.py:216-249).
//
// One wave64 per pair, no LDS, no barrier, nothing shared between waves.  The longer sequence (length L) lies along the lanes: lane l holds
// the EPL consecutive columns j = l * EPL + e + 1 (e < EPL, EPL = ceil(L / 64) rounded up to 4 / 8 / 16 / 32) together with their words, in
// registers; the shorter sequence (length n) gives the rows, so a pair costs n row steps of EPL cells per lane.
//
// A row of the table, cur[j] = min(prev[j] + 1, prev[j-1] + (r_i != h_j), cur[j-1] + 1), cur[0] = i, is kept as D[j] = cur[j] - j.  With
// P = the previous row in that form:   u[j] = min(P[j] + 1, P[j-1] - (r_i == h_j)),  u[0] = i,   D[j] = min over k <= j of u[k]
// -- the chain through cur[j-1] has become a prefix minimum: a running minimum inside the lane, ONE exclusive prefix minimum across the
// lanes (six DPP steps and a one-lane shift), one fix-up pass.  P[j-1] of a lane's first column comes from its left neighbour by a one-lane
// shift.  Columns beyond L are computed like the others and never read: a column depends on columns to its left only.
#include "a2s_internal.h"

#define ED_MAX_EPL 32
#define ED_MAX_LEN (64 * ED_MAX_EPL)
#define ED_BIG 0x3fffffff

static long long ed_launches = 0;
long a2s_edit_distance_launches(void) { return (long)__atomic_load_n(&ed_launches, __ATOMIC_RELAXED); }

// DPP controls of the wave-wide scan (gfx9 encoding): shifts inside a row of 16 lanes, the two row broadcasts, the one-lane wave shift
#define ED_DPP_ROW_SHR(n) (0x110 + (n))
#define ED_DPP_WAVE_SHR1 0x138

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int ed_dpp(int oldv, int v) {          // lanes without a source lane (or outside ROW_MASK) keep oldv
    return __builtin_amdgcn_update_dpp(oldv, v, CTRL, ROW_MASK, 0xf, false);
}
// min(first, v of every lane to the left): lane 0 gets `first`
__device__ __forceinline__ int ed_exclusive_prefix_min(int v, int first) {
    v = min(v, ed_dpp<ED_DPP_ROW_SHR(1)>(ED_BIG, v));
    v = min(v, ed_dpp<ED_DPP_ROW_SHR(2)>(ED_BIG, v));
    v = min(v, ed_dpp<ED_DPP_ROW_SHR(4)>(ED_BIG, v));
    v = min(v, ed_dpp<ED_DPP_ROW_SHR(8)>(ED_BIG, v));              // inclusive inside every row of 16
    v = min(v, ed_dpp<A2S_DPP_ROW_BCAST15, 0xA>(ED_BIG, v));       // rows 1, 3: + the row below
    v = min(v, ed_dpp<A2S_DPP_ROW_BCAST31, 0xC>(ED_BIG, v));       // rows 2, 3: + lanes 0 .. 31
    return min(first, ed_dpp<ED_DPP_WAVE_SHR1>(ED_BIG, v));
}

template <int EPL>
__device__ __forceinline__ int ed_pair(const int* __restrict__ a, int L, const int* __restrict__ b, int n, int lane) {
    int h[EPL], P[EPL];
    const int col0 = lane * EPL;                                   // (0-based) first column of this lane
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        h[e] = col0 + e < L ? a[col0 + e] : 0;
        P[e] = 0;                                                  // row 0: cur[j] = j
    }
    for (int base = 0; base < n; base += 64) {
        const int rv = base + lane < n ? b[base + lane] : 0;       // 64 row words per load, broadcast lane by lane
        const int rows = min(64, n - base);
        for (int ii = 0; ii < rows; ++ii) {
            const int r = __builtin_amdgcn_readlane(rv, ii);
            const int i = base + ii + 1;
            int diag = ed_dpp<ED_DPP_WAVE_SHR1>(i - 1, P[EPL - 1]);  // P[j-1] of the first column; lane 0: D[0] of the row above = i - 1
            int m = ED_BIG;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int up = P[e];
                m = min(m, min(up + 1, diag - (h[e] == r ? 1 : 0)));
                diag = up;
                P[e] = m;
            }
            const int left = ed_exclusive_prefix_min(m, i);
#pragma unroll
            for (int e = 0; e < EPL; ++e) P[e] = min(P[e], left);
        }
    }
    int d = -1;                                                    // the lane that holds column L: cur[L] = D[L] + L; every other lane: -1
#pragma unroll
    for (int e = 0; e < EPL; ++e)
        if (col0 + e == L - 1) d = P[e] + L;
    return d;
}

// grid: one workgroup of one wave per pair.  order (may be NULL): the pair each workgroup scores -- the host sorts the long pairs to the front.
__global__ __launch_bounds__(64) void edit_distance_pairs(const int* __restrict__ ref, const long long* __restrict__ ref_off,
                                                          const int* __restrict__ hyp, const long long* __restrict__ hyp_off,
                                                          const int* __restrict__ order, int n_pairs, int* __restrict__ dist) {
    const int lane = threadIdx.x;
    int p = order ? order[blockIdx.x] : (int)blockIdx.x;
    p = __builtin_amdgcn_readfirstlane(p);
    if (p < 0 || p >= n_pairs) return;
    const long long r0 = ref_off[p], h0 = hyp_off[p];
    int nr = (int)(ref_off[p + 1] - r0), nh = (int)(hyp_off[p + 1] - h0);
    nr = __builtin_amdgcn_readfirstlane(nr);
    nh = __builtin_amdgcn_readfirstlane(nh);
    if (nr < 0 || nh < 0 || nr > ED_MAX_LEN || nh > ED_MAX_LEN) {   // the launcher has refused such a call on the caller's maxima: never indexed
        if (lane == 0) dist[p] = -1;
        return;
    }
    const bool ref_long = nr >= nh;
    const int* a = ref_long ? ref + r0 : hyp + h0;                 // along the lanes
    const int* b = ref_long ? hyp + h0 : ref + r0;                 // the rows
    const int L = ref_long ? nr : nh, n = ref_long ? nh : nr;
    if (L == 0) {
        if (lane == 0) dist[p] = 0;
        return;
    }
    int d;
    if (L <= 64 * 4) d = ed_pair<4>(a, L, b, n, lane);
    else if (L <= 64 * 8) d = ed_pair<8>(a, L, b, n, lane);
    else if (L <= 64 * 16) d = ed_pair<16>(a, L, b, n, lane);
    else d = ed_pair<32>(a, L, b, n, lane);
    if (d >= 0) dist[p] = d;
}

int a2s_edit_distance_max_len_impl(void) { return ED_MAX_LEN; }

int a2s_edit_distance_impl(hipStream_t st, const int* ref, const long long* ref_off, const int* hyp, const long long* hyp_off, const int* order,
                           int n_pairs, int max_ref_len, int max_hyp_len, int* dist) {
    A2S_REQUIRE(n_pairs >= 0, "edit_distance: n_pairs = %d", n_pairs);
    A2S_REQUIRE(max_ref_len >= 0 && max_hyp_len >= 0, "edit_distance: negative length (%d, %d)", max_ref_len, max_hyp_len);
    A2S_REQUIRE(max_ref_len <= ED_MAX_LEN && max_hyp_len <= ED_MAX_LEN, "edit_distance: a sequence of %d words exceeds the capacity of %d",
                max_ref_len > max_hyp_len ? max_ref_len : max_hyp_len, ED_MAX_LEN);
    if (n_pairs == 0) return A2S_OK;
    A2S_REQUIRE(ref_off && hyp_off && dist, "edit_distance: null offsets or result");
    A2S_REQUIRE((ref || max_ref_len == 0) && (hyp || max_hyp_len == 0), "edit_distance: null words");
    hipLaunchKernelGGL(edit_distance_pairs, dim3(n_pairs), dim3(64), 0, st, ref, ref_off, hyp, hyp_off, order, n_pairs, dist);
    A2S_CHECK_LAUNCH("edit_distance_pairs");
    __atomic_fetch_add(&ed_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}
