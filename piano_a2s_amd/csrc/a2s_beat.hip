// Beat and downbeat tracking on the model's own features: the three device stages between the VQT and the host's small decision
// stages (piano_a2s_amd/beats.py).  tests/beat_oracle.py states stages 1 and 2 in float64 and restates stage 3 in numpy float32, bit for bit.
//
// onset_strength: env_full[b][t] = sum_f max(0, x[b][t][f] - x[b][t - lag][f]) for lag <= t < n_rows[b], 0 elsewhere; env_low: the same over f < f_split.
//     x (B, rows, F) holds dB / 80 + 1, so the difference along time does not see a window's peak normalisation.  Plain sums, no division.
//     Grid (ceil(rows / OS_SEG), B), OS_THREADS threads: a workgroup walks OS_SEG consecutive rows of one clip, OS_CHUNK rows per step, all loads of a
//     step issued together.  A thread owns the columns j = VEC * tid + k * VEC * OS_THREADS (VEC = 4: 16-byte loads, where F % 4 == 0, x is 16-byte
//     aligned and both strides are multiples of 4; else VEC = 1) in every row, and keeps the last `lag` rows of its own columns in LDS (hist, slot
//     t mod lag): row t - lag comes from there, the thread that wrote a cell is the one that reads it, no barrier.  With lag = 1 and one column tile
//     (REG) the row before stays in the thread's registers and hist is not used.  Only the `lag` rows in front of a
//     segment are read a second time (by the segment behind them): lag / OS_SEG of the traffic, from the L2 where the neighbour has just run.
//     Sum of a row: per thread k ascending, then its VEC columns ascending; then the butterfly of the wave (os_chunk_sums: the eight rows of a step
//     share it, a lane carries 4, 2 and 1 of them through its first three exchanges); then the waves ascending.  The order
//     is a function of (F, VEC) alone: a clip's bits do not depend on B, on its place in the batch or on n_rows.  Rows t >= n_rows[b] are never
//     loaded (uniform per row).  The results of a segment go through LDS and are written 16 bytes at a time where env's rows allow it.
//     Bounds: loads at columns [0, F) of rows [max(t0 - lag, 0), min(t0 + OS_SEG, n)) of clip b, n = clamp(n_rows[b], 0, rows); stores at
//     [t0, min(t0 + OS_SEG, rows)) of clip b's rows of env_full and env_low; LDS hist at [slot * Fp + j, + VEC), slot < lag, j + VEC <= Fp.
// tempogram: block j of recording r, centred at frame j * hop_b: window frames g = j * hop_b - win / 2 + u, u in [0, win);
//     d[u] = env[g] - mean (over the window's frames inside [0, n[r])) for g inside, 0 outside;  A_j[l] = sum_{u < win - l} d[u] d[u + l] / sum d^2,
//     0 where the denominator is 0.  One workgroup of TG_THREADS threads per (j, r), the window in LDS; a wave owns the lags lag_min + wave,
//     + waves, ...: lanes stride over u (fp32 FMAs, u ascending per lane), xor butterfly.  Every wave forms the denominator itself (same order, same bits).
//     Bounds: loads at [max(g0, 0), min(g0 + win, n)) of recording r's row; stores at the lag_max - lag_min + 1 floats of (r, j).
// beat_dp: for t = 0 .. n - 1, tau = clamp(period[min(t / hop_b, J - 1)], lag_min, lag_max), candidates p in [max(0, t - 2 tau), t - ceil(tau / 2)]:
//     c(p) = S[p] - pen[tau - lag_min][t - p] (one fp32 subtraction), S[t] = ls[t] + max(0, max_p c(p)) (one fp32 addition), back[t] = the arg max,
//     the candidate nearest to t among equals, -1 where none is above 0.  No multiply anywhere: nothing to contract.
//     One persistent workgroup of BD_THREADS threads per recording.  S[t] reads S[p] only at t - p >= ceil(tau(t) / 2), so the frames
//     t_c .. t_c + W - 1 are independent as long as i < ceil(tau(t_c + i) / 2) for every i < W: W is the length of the leading run of frames for which
//     that holds, at most BD_FRAMES, found by every wave for itself (32 lanes look up tau, one ballot), so it follows the SMALLEST half period
//     inside the chunk also where the period changes in the middle of it.  A group of BD_G lanes owns a frame, lanes stride over its candidates, p
//     ascending, and the group reduces (value, p) with an xor butterfly.  The last 2 lag_max + BD_FRAMES scores live in an LDS ring (a power of two);
//     one barrier per chunk.  A slot written in a chunk held S[t - ring], which no frame of the chunk reads.  S and back go to memory with vector
//     (per-lane) stores by the group's first lane.  After the last chunk wave 0 finds the last beat, the first arg max of S over the last tau(n - 1)
//     frames, in the ring; thread 0 follows back from there through memory (the workgroup's own stores, behind a barrier), counts, and writes the
//     beats ascending, as many as fit: count[r] is the true number.  Entries of beats at and behind count[r] are not written.
//     Bounds: loads at [0, n) of ls, [0, J) of period, row tau - lag_min and column t - p in [1, 2 lag_max] of pen ((lag_max - lag_min + 1) rows of
//     2 lag_max + 1 floats); stores at [0, n) of S and back, [0, min(count, max_beats)) of beats, count[r]; n = clamp(n[r], 0, stride).
// Nothing is allocated, nothing synchronises with the host, nothing is read back; no atomics, no waits between workgroups.
#include "a2s_internal.h"

#define OS_THREADS 128
#define OS_WAVES (OS_THREADS / 64)
#define OS_SEG 64                  // rows per workgroup (32 and 128 measured the same)
#define OS_CHUNK 8                // (os_chunk_sums is written for 8)
#define OS_HIST_MAX 12288          // floats of LDS for the `lag` rows a workgroup keeps

#define TG_THREADS 256
#define TG_WAVES (TG_THREADS / 64)
#define TG_WIN_MAX 8192
#define TG_LAGS_MAX 4096

#define BD_THREADS 512
#define BD_G 16
#define BD_FRAMES (BD_THREADS / BD_G)          // 32: the frames of a chunk at most; a wave looks up their periods with its lanes 0 .. 31
#define BD_LAG_MAX 4096

static long long beat_launches = 0;

__device__ __forceinline__ float bt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The sums over the wave of a[0 .. 7], one per row of a chunk: lane l < 8 returns the sum of a[os_chunk_row(l)].  A butterfly that halves what a lane
// carries at every step (4 + 2 + 1 exchanges, then 3 on the one value left) instead of 8 full reductions of 6 exchanges each.
__device__ __forceinline__ int os_chunk_row(int lane) { return ((lane & 1) << 2) | (lane & 2) | ((lane & 4) >> 2); }
__device__ __forceinline__ float os_chunk_sums(const float (&a)[OS_CHUNK], int lane) {
    float b[4], c[2];
    const bool h1 = lane & 1, h2 = lane & 2, h4 = lane & 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = (h1 ? a[i + 4] : a[i]) + __shfl_xor(h1 ? a[i] : a[i + 4], 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) c[i] = (h2 ? b[i + 2] : b[i]) + __shfl_xor(h2 ? b[i] : b[i + 2], 2);
    float v = (h4 ? c[1] : c[0]) + __shfl_xor(h4 ? c[0] : c[1], 4);
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

template <int VEC, bool REG>
__global__ __launch_bounds__(OS_THREADS) void onset_strength(const float* __restrict__ x, long x_bstride, long x_rstride, const int* __restrict__ n_rows,
                                                             int rows, int F, int Fp, int lag, int f_split, float* __restrict__ env_full,
                                                             float* __restrict__ env_low, long env_bstride, int out_vec) {
    typedef typename a2s_row_vec<VEC>::type V;
    extern __shared__ __attribute__((aligned(16))) float os_lds[];
    float* hist = os_lds;                                   // (lag, Fp)
    float* part = hist + (long)lag * Fp;                    // (OS_SEG, OS_WAVES, 2)
    float* res = part + OS_SEG * OS_WAVES * 2;              // (2, OS_SEG)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int t0 = blockIdx.x * OS_SEG;
    int n = n_rows[b];
    n = n < 0 ? 0 : (n > rows ? rows : n);
    const int seg_n = rows - t0 < OS_SEG ? rows - t0 : OS_SEG;
    const bool live = t0 < n;

    if (live) {
        const float* __restrict__ xb = x + (long)b * x_bstride;
        V last;                                                       // REG (lag == 1, one column tile): row t - 1 of this thread's columns
        if (REG) {
            if (t0 > 0 && tid * VEC < F) last = *reinterpret_cast<const V*>(xb + (long)(t0 - 1) * x_rstride + tid * VEC);
        } else {
            for (int t = t0 > lag ? t0 - lag : 0; t < t0; ++t) {      // the rows in front of the segment (t < t0 < n)
                const int s = t % lag;
                for (int j = tid * VEC; j < F; j += OS_THREADS * VEC)
                    *reinterpret_cast<V*>(hist + (long)s * Fp + j) = *reinterpret_cast<const V*>(xb + (long)t * x_rstride + j);
            }
        }
        int slot = t0 % lag;
        for (int c0 = 0; c0 < seg_n && t0 + c0 < n; c0 += OS_CHUNK) {
            float af[OS_CHUNK], al[OS_CHUNK];
#pragma unroll
            for (int r = 0; r < OS_CHUNK; ++r) af[r] = al[r] = 0.0f;
            for (int j = tid * VEC; j < F; j += OS_THREADS * VEC) {
                V cur[OS_CHUNK];
#pragma unroll
                for (int r = 0; r < OS_CHUNK; ++r) {                  // all loads of the step are issued together; t < n is uniform
                    const int t = t0 + c0 + r;
                    if (t < n) cur[r] = *reinterpret_cast<const V*>(xb + (long)t * x_rstride + j);
                }
                int s = slot;
#pragma unroll
                for (int r = 0; r < OS_CHUNK; ++r) {
                    const int t = t0 + c0 + r;
                    if (t < n) {
                        V prev;                                       // row t - lag (whatever the slot held, where t < lag: not used)
                        if (REG) {
                            prev = last;
                            last = cur[r];
                        } else {
                            float* h = hist + (long)s * Fp + j;
                            prev = *reinterpret_cast<const V*>(h);
                            *reinterpret_cast<V*>(h) = cur[r];
                        }
                        if (t >= lag) {
                            float c[VEC], p[VEC];
                            __builtin_memcpy(c, &cur[r], 4 * VEC);
                            __builtin_memcpy(p, &prev, 4 * VEC);
#pragma unroll
                            for (int e = 0; e < VEC; ++e) {
                                const float d = fmaxf(c[e] - p[e], 0.0f);
                                af[r] += d;
                                if (j + e < f_split) al[r] += d;
                            }
                        }
                        s = s + 1 == lag ? 0 : s + 1;
                    }
                }
            }
            slot = (slot + OS_CHUNK) % lag;
            const float sf = os_chunk_sums(af, lane), sl = os_chunk_sums(al, lane);
            if (lane < OS_CHUNK) {
                const int r = os_chunk_row(lane);
                part[((c0 + r) * OS_WAVES + wave) * 2] = sf;
                part[((c0 + r) * OS_WAVES + wave) * 2 + 1] = sl;
            }
        }
    }
    __syncthreads();
    if (tid < OS_SEG) {
        const int t = t0 + tid;
        float sf = 0.0f, sl = 0.0f;
        if (live && t < n && t >= lag) {                              // (exactly the rows whose partial sums were written)
#pragma unroll
            for (int w = 0; w < OS_WAVES; ++w) {
                sf += part[(tid * OS_WAVES + w) * 2];
                sl += part[(tid * OS_WAVES + w) * 2 + 1];
            }
        }
        res[tid] = sf;
        res[OS_SEG + tid] = sl;
    }
    __syncthreads();
    if (tid < 2 * (OS_SEG / 4)) {
        const int which = tid / (OS_SEG / 4), g = (tid % (OS_SEG / 4)) * 4;
        float* __restrict__ out = (which ? env_low : env_full) + (long)b * env_bstride + t0;
        const float* src = res + which * OS_SEG + g;
        if (out_vec && g + 4 <= seg_n) {
            *reinterpret_cast<f32x4*>(out + g) = *reinterpret_cast<const f32x4*>(src);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (g + e < seg_n) out[g + e] = src[e];
        }
    }
}

__global__ __launch_bounds__(TG_THREADS) void tempogram(const float* __restrict__ env, long stride, const int* __restrict__ n, int J, int win, int winp,
                                                        int hop_b, int lag_min, int lag_max, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float tg_lds[];
    float* d = tg_lds;                                      // (winp)
    float* res = d + winp;                                  // (lag_max - lag_min + 1)
    float* red = res + (lag_max - lag_min + 1);             // (TG_WAVES)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = blockIdx.x, r = blockIdx.y;
    long nn = n[r];
    nn = nn < 0 ? 0 : (nn > stride ? stride : nn);
    const long g0 = (long)j * hop_b - win / 2;
    const float* __restrict__ e = env + (long)r * stride;
    const long lo = g0 > 0 ? g0 : 0, hi = g0 + win < nn ? g0 + win : nn;
    const int cnt = hi > lo ? (int)(hi - lo) : 0;
    float s = 0.0f;
    for (int u = tid; u < win; u += TG_THREADS) {
        const long g = g0 + u;
        const float v = (g >= lo && g < hi) ? e[g] : 0.0f;
        d[u] = v;
        s += v;
    }
    s = bt_wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    float total = red[0];
#pragma unroll
    for (int w = 1; w < TG_WAVES; ++w) total += red[w];
    const float mean = cnt > 0 ? total / (float)cnt : 0.0f;
    for (int u = tid; u < win; u += TG_THREADS) {           // (a thread's own cells)
        const long g = g0 + u;
        d[u] = (g >= lo && g < hi) ? d[u] - mean : 0.0f;
    }
    __syncthreads();
    float den = 0.0f;
    for (int u = lane; u < win; u += 64) den = fmaf(d[u], d[u], den);
    den = bt_wave_sum(den);
    for (int l = lag_min + wave; l <= lag_max; l += TG_WAVES) {
        float acc = 0.0f;
        for (int u = lane; u < win - l; u += 64) acc = fmaf(d[u], d[u + l], acc);
        acc = bt_wave_sum(acc);
        if (lane == 0) res[l - lag_min] = den > 0.0f ? acc / den : 0.0f;
    }
    __syncthreads();
    const int nl = lag_max - lag_min + 1;
    float* __restrict__ o = out + ((long)r * J + j) * nl;
    for (int i = tid; i < nl; i += TG_THREADS) o[i] = res[i];
}

__global__ __launch_bounds__(BD_THREADS) void beat_dp(const float* __restrict__ ls, long stride, const int* __restrict__ period, int J, int hop_b,
                                                      const float* __restrict__ pen, int lag_min, int lag_max, const int* __restrict__ n,
                                                      float* __restrict__ S, int* __restrict__ back, int* __restrict__ beats, int max_beats,
                                                      int* __restrict__ count, int mask) {
    extern __shared__ __attribute__((aligned(16))) float ring[];          // mask + 1 scores: S[t] at t & mask
    const int tid = threadIdx.x, lane = tid & 63, gl = tid & (BD_G - 1), fi = tid / BD_G, r = blockIdx.x;
    long nl = n[r];
    const int nn = (int)(nl < 0 ? 0 : (nl > stride ? stride : nl));
    const float* __restrict__ lsr = ls + (long)r * stride;
    const int* __restrict__ per = period + (long)r * J;
    float* __restrict__ Sr = S + (long)r * stride;
    int* backr = back + (long)r * stride;
    const int pw = 2 * lag_max + 1;

    for (int t_c = 0; t_c < nn;) {
        // the chunk: every wave looks up the periods of the next BD_FRAMES frames (lanes 32 .. 63 repeat lanes 0 .. 31) and counts the leading run
        const int i = lane & (BD_FRAMES - 1), tl = t_c + i;
        const int blk = tl / hop_b < J - 1 ? tl / hop_b : J - 1;
        int tau_l = per[blk];
        tau_l = tau_l < lag_min ? lag_min : (tau_l > lag_max ? lag_max : tau_l);
        const bool ok = tl < nn && i < ((tau_l + 1) >> 1);
        const unsigned run = (unsigned)__ballot(ok);                      // bit i: frame t_c + i may join (bit 0 is set: tau >= 1, t_c < nn)
        const int W = run == 0xffffffffu ? BD_FRAMES : __builtin_ctz(~run);
        const int tau = __shfl(tau_l, fi & 63);                           // the period of this group's frame (fi < BD_FRAMES <= 64)
        const bool active = fi < W;
        const int t = t_c + fi;
        const int hi = active ? t - ((tau + 1) >> 1) : -1;
        const int lo = t - 2 * tau > 0 ? t - 2 * tau : 0;
        const float* __restrict__ prow = pen + (long)(tau - lag_min) * pw;
        float best = 0.0f;
        int bp = -1;
        for (int p = lo + gl; p <= hi; p += BD_G) {                       // p ascending: an equal later candidate is nearer to t
            const float c = __fsub_rn(ring[p & mask], prow[t - p]);
            if (c > best || (c == best && bp >= 0)) {
                best = c;
                bp = p;
            }
        }
#pragma unroll
        for (int o = BD_G / 2; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o);
            const int op = __shfl_xor(bp, o);
            if (ov > best || (ov == best && op > bp)) {
                best = ov;
                bp = op;
            }
        }
        if (active && gl == 0) {
            const float s = __fadd_rn(lsr[t], best);
            ring[t & mask] = s;
            Sr[t] = s;
            backr[t] = bp;
        }
        __syncthreads();
        t_c += W;
    }

    if (tid >= 64) return;
    int last = -1;
    if (nn > 0) {
        const int bl = (nn - 1) / hop_b < J - 1 ? (nn - 1) / hop_b : J - 1;
        int tau = per[bl];
        tau = tau < lag_min ? lag_min : (tau > lag_max ? lag_max : tau);
        const int a = nn - tau > 0 ? nn - tau : 0;
        float best = -INFINITY;
        int bt = 0x7fffffff;
        for (int t = a + lane; t < nn; t += 64) {                         // t ascending: the first of equals stays
            const float v = ring[t & mask];
            if (v > best) {
                best = v;
                bt = t;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o);
            const int ot = __shfl_xor(bt, o);
            if (ov > best || (ov == best && ot < bt)) {
                best = ov;
                bt = ot;
            }
        }
        last = bt == 0x7fffffff ? a : bt;                                 // (every score a NaN: the first frame of the range)
    }
    if (tid != 0) return;
    int cnt = 0;
    for (int t = last; t >= 0; t = backr[t]) ++cnt;                       // back[t] < t: the walk ends
    int k = cnt - 1;
    for (int t = last; t >= 0; t = backr[t], --k)
        if (k < max_beats) beats[(long)r * max_beats + k] = t;
    count[r] = cnt;
}

int a2s_onset_strength_impl(hipStream_t st, const float* x, long x_bstride, long x_rstride, const int* n_rows, int B, int rows, int F, int lag, int f_split,
                            float* env_full, float* env_low, long env_bstride) {
    A2S_REQUIRE(x && n_rows && env_full && env_low, "onset_strength: null x, n_rows, env_full or env_low");
    A2S_REQUIRE(B >= 0 && B <= 65535, "onset_strength: needs 0 <= B <= 65535 (got %d)", B);
    A2S_REQUIRE(rows >= 1 && F >= 1, "onset_strength: needs rows >= 1 and F >= 1 (got rows = %d, F = %d)", rows, F);
    A2S_REQUIRE(lag >= 1, "onset_strength: needs lag >= 1 (got %d)", lag);
    A2S_REQUIRE(f_split >= 0 && f_split <= F, "onset_strength: needs 0 <= f_split <= F = %d (got %d)", F, f_split);
    const int Fp = (F + 3) & ~3;
    A2S_REQUIRE((long)lag * Fp <= OS_HIST_MAX, "onset_strength: lag * F = %d * %d exceeds the %d floats a workgroup keeps", lag, F, OS_HIST_MAX);
    A2S_REQUIRE(x_rstride >= F && x_bstride >= (long)(rows - 1) * x_rstride + F && env_bstride >= rows,
                "onset_strength: needs a row stride >= F, a clip stride >= (rows - 1) * row stride + F and an env stride >= rows (got %ld, %ld, %ld)", x_rstride,
                x_bstride, env_bstride);
    if (B == 0) return A2S_OK;
    const int vec = (F % 4 == 0 && ((uintptr_t)x & 15) == 0 && x_rstride % 4 == 0 && x_bstride % 4 == 0) ? 4 : 1;
    const int out_vec = (((uintptr_t)env_full & 15) == 0 && ((uintptr_t)env_low & 15) == 0 && env_bstride % 4 == 0) ? 1 : 0;
    const size_t lds = ((size_t)lag * Fp + OS_SEG * OS_WAVES * 2 + 2 * OS_SEG) * sizeof(float);
    const dim3 grid(a2s_cdiv(rows, OS_SEG), B);
    const bool reg = lag == 1 && F <= OS_THREADS * vec;          // the row before stays in registers
#define OS_LAUNCH(VEC, REG)                                                                                                                            \
    hipLaunchKernelGGL((onset_strength<VEC, REG>), grid, dim3(OS_THREADS), lds, st, x, x_bstride, x_rstride, n_rows, rows, F, Fp, lag, f_split, env_full, \
                       env_low, env_bstride, out_vec)
    if (vec == 4 && reg) OS_LAUNCH(4, true);
    else if (vec == 4) OS_LAUNCH(4, false);
    else if (reg) OS_LAUNCH(1, true);
    else OS_LAUNCH(1, false);
#undef OS_LAUNCH
    A2S_CHECK_LAUNCH("onset_strength");
    __atomic_fetch_add(&beat_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_tempogram_impl(hipStream_t st, const float* env, long stride, const int* n, int R, int J, int win, int hop_b, int lag_min, int lag_max, float* out) {
    A2S_REQUIRE(env && n && out, "tempogram: null env, n or out");
    A2S_REQUIRE(R >= 0 && R <= 65535, "tempogram: needs 0 <= R <= 65535 (got %d)", R);
    A2S_REQUIRE(stride >= 1 && J >= 1, "tempogram: needs stride >= 1 and J >= 1 (got %ld, %d)", stride, J);
    A2S_REQUIRE(win >= 1 && win <= TG_WIN_MAX && hop_b >= 1, "tempogram: needs 1 <= win <= %d and hop_b >= 1 (got %d, %d)", TG_WIN_MAX, win, hop_b);
    A2S_REQUIRE(lag_min >= 0 && lag_min <= lag_max && lag_max - lag_min < TG_LAGS_MAX,
                "tempogram: needs 0 <= lag_min <= lag_max and at most %d lags (got %d, %d)", TG_LAGS_MAX, lag_min, lag_max);
    if (R == 0) return A2S_OK;
    const int winp = (win + 3) & ~3;
    const size_t lds = ((size_t)winp + (lag_max - lag_min + 1) + TG_WAVES) * sizeof(float);
    hipLaunchKernelGGL(tempogram, dim3(J, R), dim3(TG_THREADS), lds, st, env, stride, n, J, win, winp, hop_b, lag_min, lag_max, out);
    A2S_CHECK_LAUNCH("tempogram");
    __atomic_fetch_add(&beat_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_beat_dp_impl(hipStream_t st, const float* ls, long stride, const int* period, int J, int hop_b, const float* pen, int lag_min, int lag_max,
                     const int* n, int R, float* S, int* back, int* beats, int max_beats, int* count) {
    A2S_REQUIRE(ls && period && pen && n && S && back && beats && count, "beat_dp: null ls, period, pen, n, S, back, beats or count");
    A2S_REQUIRE(R >= 0 && R <= 65535, "beat_dp: needs 0 <= R <= 65535 (got %d)", R);
    A2S_REQUIRE(stride >= 1 && J >= 1 && hop_b >= 1, "beat_dp: needs stride >= 1, J >= 1 and hop_b >= 1 (got %ld, %d, %d)", stride, J, hop_b);
    A2S_REQUIRE(lag_min >= 1 && lag_min <= lag_max && lag_max <= BD_LAG_MAX, "beat_dp: needs 1 <= lag_min <= lag_max <= %d (got %d, %d)", BD_LAG_MAX, lag_min,
                lag_max);
    A2S_REQUIRE(max_beats >= 1, "beat_dp: needs max_beats >= 1 (got %d)", max_beats);
    if (R == 0) return A2S_OK;
    int ring = 64;
    while (ring < 2 * lag_max + BD_FRAMES) ring *= 2;
    hipLaunchKernelGGL(beat_dp, dim3(R), dim3(BD_THREADS), (size_t)ring * sizeof(float), st, ls, stride, period, J, hop_b, pen, lag_min, lag_max, n, S, back,
                       beats, max_beats, count, ring - 1);
    A2S_CHECK_LAUNCH("beat_dp");
    __atomic_fetch_add(&beat_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_beat_launches_impl(void) { return (int)__atomic_load_n(&beat_launches, __ATOMIC_RELAXED); }
