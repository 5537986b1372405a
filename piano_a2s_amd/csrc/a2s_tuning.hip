// The tuning of a recording from the model's own features: the two device stages in front of a2s_shift_bins.
// tests/tuning_oracle.py states both in float64 and exact integers; the kernels reproduce the first integer for integer, the second bit for bit.
//
// tuning_profile: x (B, rows, F) holds dB / 80 + 1, bin 0 is A0, S bins per semitone.  Over the frames t < clamp(n_rows[b], 0, rows) and the bins
//     1 <= f <= F - 2, with a, c, e = x[t][f - 1], x[t][f], x[t][f + 1]: a PEAK is c > a && c >= e && c >= thr (false with a NaN).  In double:
//         delta = 0.5 (a - e) / ((a - c) + (e - c))  (a NaN -- only cells at +-inf give one -- reads as 0);   u = ((f mod S) + delta) + S / 2,
//         u -= S where u >= S;   cell = min(H - 1, floor(u * H / S));   weight = 1 + rint(min(c - thr, 1) * Q)
//     hist[b][cell] += weight, hist[b][H] += 1.  H = 100 cells, one cent each; cell k stands for a deviation of [k - 50, k - 49) cents.
//     Grid (ceil(rows / TN_SEG), B), TN_THREADS threads.  A WAVE owns whole rows: TN_ROWS rows at a time, 64 * VEC consecutive columns per step
//     (VEC = 4: 16-byte loads, where F % 4 == 0, x is 16-byte aligned and both strides are multiples of 4; else VEC = 1); the loads of the next
//     step are issued before the current one is examined.  Every cell is read from memory once: the left neighbour of a lane's first column and the
//     right neighbour of its last come from the lanes beside it (cross-lane moves), across a step from lane 63 of the step before and from lane 0
//     of the step after, which the wave already holds.  Two peaks cannot be neighbours (c > a on one side, c >= e on the other), so a lane has at
//     most VEC / 2 of them and walks its own bit mask.
//     Every wave keeps its own H cells in LDS (32-bit, integer LDS atomics; nothing is shared between waves, so the kernel has no barrier) and adds
//     its non-zero cells to hist with 64-bit integer global atomics: at the end of its rows, and before the cells it has examined since the last
//     flush exceed TN_FLUSH_CELLS = 2^20 -- at most 2^19 peaks of weight <= Q + 1 = 4097, below 2^32.  The peak count travels in a register and
//     is added once per wave.  Integers only: the result does not depend on the order of arrival, on B, on the strides or on the clip's place.
//     Bounds.  Loads: columns [0, F) of the rows [t0, min(t0 + TN_SEG, n)) of clip b, n = clamp(n_rows[b], 0, rows); 16-byte loads at columns
//     j = 4 i with j + 3 < F only.  LDS: cells[wave][0 .. H - 1], cell clamped to [0, H - 1].  Global atomics: hist[b][0 .. H].
// tuning_estimate: one workgroup per group g of the clips first[g] .. first[g + 1] - 1 (clamped to [0, B]): h = their histograms added (int64);
//     sm[k] = sum_j (7 - |j|) h[(k + j) mod H], j = -6 .. 6 (int64, exact); k* = the first arg max; then in double, one operation per step:
//         conf = sm[k*] * H / sum(sm) (0 where the sum is 0);   with A, C, E = sm[k* - 1], sm[k*], sm[k* + 1] (circular), den = (A - C) + (E - C):
//         delta = 0.5 (A - E) / den where den < 0, else 0;   cents = ((k* + 0.5) + delta) * 100 / H - 50, cents -= 100 where it reaches 50;
//     est[g] = [cents, conf, peaks]; eff_bins[b] = (float)(-cents * S / 100) for the group's clips where peaks >= min_peaks && conf >= min_conf,
//     else 0.  An empty group gives [-49.5, 0, 0].  The clips are added by TE_PARTS threads per cell, every TE_PARTS-th clip each.  Thread 0
//     finds the arg max by walking the 100 cells: exact, and nothing next to the sums.
//     Bounds.  Loads: first[g], first[g + 1], hist rows [lo, hi) with 0 <= lo <= hi <= B.  Stores: est[3 g .. 3 g + 2], eff_bins[lo .. hi).
// Nothing is allocated, nothing synchronises with the host, nothing is read back; no float atomics.
#include "a2s_internal.h"

#define TN_H 100
#define TN_Q 4096.0
#define TN_THREADS 256
#define TN_WAVES (TN_THREADS / A2S_WAVE)
#define TN_SEG 64                  // rows per workgroup: 16 per wave
#define TN_ROWS 4                  // rows a wave has in flight
#define TN_FLUSH_CELLS (1 << 20)
#define TN_HALF_WINDOW 6
#define TE_THREADS 512
#define TE_PARTS (TE_THREADS / 128)    // the clips of a group are added in TE_PARTS interleaved parts (integers: any order gives the same sum)

static long long tuning_launches = 0;

__device__ __forceinline__ void tn_add_peak(unsigned int* h, float a, float c, float e, long f, int S, double thr) {
#pragma clang fp contract(off)
    const double da = a, dc = c, de = e, dS = (double)S;
    double delta = 0.5 * (da - de) / ((da - dc) + (de - dc));
    if (delta != delta) delta = 0.0;
    double u = ((double)(int)(f % S) + delta) + 0.5 * dS;
    if (u >= dS) u -= dS;
    int cell = (int)floor(u * (double)TN_H / dS);
    cell = cell < 0 ? 0 : (cell > TN_H - 1 ? TN_H - 1 : cell);
    const unsigned int w = 1u + (unsigned int)rint(fmin(dc - thr, 1.0) * TN_Q);
    atomicAdd(h + cell, w);
}

// the wave's cells -> hist, and zero again (an exchange: it stays behind the wave's own earlier adds to the cell)
__device__ __forceinline__ void tn_flush(unsigned int* h, unsigned long long* out, int lane) {
    for (int c = lane; c < TN_H; c += A2S_WAVE) {
        const unsigned int v = atomicExch(h + c, 0u);
        if (v) atomicAdd(out + c, (unsigned long long)v);
    }
}

template <int VEC>
__global__ __launch_bounds__(TN_THREADS) void tuning_profile(const float* __restrict__ x, long x_bstride, long x_rstride, const int* __restrict__ n_rows,
                                                             int rows, int F, int S, float thr, unsigned long long* __restrict__ hist) {
    typedef typename a2s_row_vec<VEC>::type V;
    __shared__ unsigned int cells[TN_WAVES][TN_H];
    const int tid = threadIdx.x, lane = tid & (A2S_WAVE - 1), wave = tid / A2S_WAVE, b = blockIdx.y;
    const long t0 = (long)blockIdx.x * TN_SEG;
    long n = n_rows[b];
    n = n < 0 ? 0 : (n > rows ? rows : n);
    const long t_end = t0 + TN_SEG < n ? t0 + TN_SEG : n;
    if (t0 + wave * TN_ROWS >= t_end) return;                        // (the whole wave; there is no barrier in this kernel)
    unsigned int* h = cells[wave];
    for (int c = lane; c < TN_H; c += A2S_WAVE) h[c] = 0u;
    unsigned long long* out = hist + (long)b * (TN_H + 1);
    const float* __restrict__ xb = x + (long)b * x_bstride;
    const double dthr = (double)thr;
    const long W = (long)A2S_WAVE * VEC, steps = (F + W - 1) / W;
    unsigned int peaks = 0;
    int pending = 0;                                                  // cells examined since the last flush (uniform)
    V zero;
    __builtin_memset(&zero, 0, sizeof(V));

    for (long tb = t0 + wave * TN_ROWS; tb < t_end; tb += TN_WAVES * TN_ROWS) {
        V cur[TN_ROWS], nxt[TN_ROWS];
        float last[TN_ROWS];                                          // the last column of the step before (lane 0's left neighbour)
#pragma unroll
        for (int r = 0; r < TN_ROWS; ++r) {
            last[r] = 0.f;
            nxt[r] = zero;
            cur[r] = (tb + r < t_end && (long)lane * VEC < F) ? *reinterpret_cast<const V*>(xb + (tb + r) * x_rstride + (long)lane * VEC) : zero;
        }
        for (long k = 0; k < steps; ++k) {
            const long j = k * W + (long)lane * VEC;
            const bool more = k + 1 < steps;
#pragma unroll
            for (int r = 0; r < TN_ROWS; ++r)                         // the next step's loads, all issued together
                nxt[r] = (more && tb + r < t_end && j + W < F) ? *reinterpret_cast<const V*>(xb + (tb + r) * x_rstride + j + W) : zero;
            if (pending > TN_FLUSH_CELLS - TN_ROWS * (int)W) {
                tn_flush(h, out, lane);
                pending = 0;
            }
            pending += TN_ROWS * (int)W;
#pragma unroll
            for (int r = 0; r < TN_ROWS; ++r) {
                if (tb + r >= t_end) continue;                        // (uniform)
                float v[VEC + 2], first_next[1];
                __builtin_memcpy(v + 1, &cur[r], sizeof(V));
                __builtin_memcpy(first_next, &nxt[r], sizeof(float));
                const float up = __shfl_up(v[VEC], 1), down = __shfl_down(v[1], 1), over = __shfl(first_next[0], 0);
                v[0] = lane == 0 ? last[r] : up;
                v[VEC + 1] = lane == A2S_WAVE - 1 ? over : down;
                last[r] = __shfl(v[VEC], A2S_WAVE - 1);
                unsigned int m = 0;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const long f = j + e;
                    if (f >= 1 && f <= (long)F - 2 && v[e + 1] > v[e] && v[e + 1] >= v[e + 2] && v[e + 1] >= thr) m |= 1u << e;
                }
                peaks += __popc(m);
                while (m) {
                    const int e = __ffs(m) - 1;
                    m &= m - 1;
                    float a = v[0], c = v[1], d = v[2];
#pragma unroll
                    for (int i = 1; i < VEC; ++i)
                        if (e == i) {
                            a = v[i];
                            c = v[i + 1];
                            d = v[i + 2];
                        }
                    tn_add_peak(h, a, c, d, j + e, S, dthr);
                }
            }
#pragma unroll
            for (int r = 0; r < TN_ROWS; ++r) cur[r] = nxt[r];
        }
    }
    tn_flush(h, out, lane);
#pragma unroll
    for (int o = A2S_WAVE / 2; o > 0; o >>= 1) peaks += __shfl_xor(peaks, o);
    if (lane == 0 && peaks) atomicAdd(out + TN_H, (unsigned long long)peaks);
}

__global__ __launch_bounds__(TE_THREADS) void tuning_estimate(const long long* __restrict__ hist, const int* __restrict__ first, int B, int S, double min_conf,
                                                              int min_peaks, double* __restrict__ est, float* __restrict__ eff_bins) {
#pragma clang fp contract(off)
    __shared__ long long part[TE_PARTS][TN_H + 1], h[TN_H + 1], sm[TN_H];
    __shared__ float shift;
    const int g = blockIdx.x, tid = threadIdx.x, cell = tid & 127, p = tid >> 7;
    long lo = first[g], hi = first[g + 1];
    lo = lo < 0 ? 0 : (lo > B ? B : lo);
    hi = hi < lo ? lo : (hi > B ? B : hi);
    if (cell <= TN_H) {
        long long s = 0;
#pragma unroll 4
        for (long b = lo + p; b < hi; b += TE_PARTS) s += hist[b * (TN_H + 1) + cell];
        part[p][cell] = s;
    }
    __syncthreads();
    if (tid <= TN_H) {
        long long s = 0;
#pragma unroll
        for (int q = 0; q < TE_PARTS; ++q) s += part[q][tid];
        h[tid] = s;
    }
    __syncthreads();
    if (tid < TN_H) {
        long long s = 0;
#pragma unroll
        for (int j = -TN_HALF_WINDOW; j <= TN_HALF_WINDOW; ++j) s += (long long)(TN_HALF_WINDOW + 1 - (j < 0 ? -j : j)) * h[(tid + j + TN_H) % TN_H];
        sm[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int k = 0;
        long long total = 0;
        for (int i = 0; i < TN_H; ++i) {
            total += sm[i];
            if (sm[i] > sm[k]) k = i;                                 // (the first of equals stays)
        }
        const long long A = sm[(k + TN_H - 1) % TN_H], C = sm[k], E = sm[(k + 1) % TN_H], den = (A - C) + (E - C);
        const double conf = total != 0 ? (double)C * (double)TN_H / (double)total : 0.0;
        const double delta = den < 0 ? 0.5 * (double)(A - E) / (double)den : 0.0;
        double cents = (((double)k + 0.5) + delta) * 100.0 / (double)TN_H - 50.0;
        if (cents >= 50.0) cents -= 100.0;
        const long long peaks = h[TN_H];
        est[3 * (long)g] = cents;
        est[3 * (long)g + 1] = conf;
        est[3 * (long)g + 2] = (double)peaks;
        shift = (peaks >= (long long)min_peaks && conf >= min_conf) ? (float)(-cents * (double)S / 100.0) : 0.f;
    }
    __syncthreads();
    const float s = shift;
    for (long b = lo + tid; b < hi; b += TE_THREADS) eff_bins[b] = s;
}

int a2s_tuning_profile_impl(hipStream_t st, const float* x, long x_bstride, long x_rstride, const int* n_rows, int B, int rows, int F,
                            int bins_per_semitone, float thr, long long* hist) {
    A2S_REQUIRE(x && n_rows && hist, "tuning_profile: null x, n_rows or hist");
    A2S_REQUIRE(B >= 0 && B <= 65535, "tuning_profile: needs 0 <= B <= 65535 (got %d)", B);
    A2S_REQUIRE(rows >= 1 && F >= 1, "tuning_profile: needs rows >= 1 and F >= 1 (got rows = %d, F = %d)", rows, F);
    A2S_REQUIRE(bins_per_semitone >= 1 && bins_per_semitone <= 64, "tuning_profile: needs 1 <= bins_per_semitone <= 64 (got %d)", bins_per_semitone);
    A2S_REQUIRE(thr >= 0.f && thr <= 1.f, "tuning_profile: needs a threshold in 0 .. 1 (got %g)", (double)thr);
    A2S_REQUIRE(x_rstride >= F && x_bstride >= (long)(rows - 1) * x_rstride + F,
                "tuning_profile: needs a row stride >= F and a clip stride >= (rows - 1) * row stride + F (got %ld, %ld)", x_rstride, x_bstride);
    if (B == 0) return A2S_OK;
    const hipError_t e = hipMemsetAsync(hist, 0, (size_t)B * (TN_H + 1) * sizeof(long long), st);
    if (e != hipSuccess) A2S_FAIL(A2S_ERR_HIP, "tuning_profile: zeroing hist: %s", hipGetErrorString(e));
    if (F < 3) return A2S_OK;                                        // no bin has two neighbours: zeros
    const int vec = (F % 4 == 0 && ((uintptr_t)x & 15) == 0 && x_rstride % 4 == 0 && x_bstride % 4 == 0) ? 4 : 1;
    const dim3 grid(a2s_cdiv(rows, TN_SEG), B);
    if (vec == 4)
        hipLaunchKernelGGL(tuning_profile<4>, grid, dim3(TN_THREADS), 0, st, x, x_bstride, x_rstride, n_rows, rows, F, bins_per_semitone, thr,
                           reinterpret_cast<unsigned long long*>(hist));
    else
        hipLaunchKernelGGL(tuning_profile<1>, grid, dim3(TN_THREADS), 0, st, x, x_bstride, x_rstride, n_rows, rows, F, bins_per_semitone, thr,
                           reinterpret_cast<unsigned long long*>(hist));
    A2S_CHECK_LAUNCH("tuning_profile");
    __atomic_fetch_add(&tuning_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_tuning_estimate_impl(hipStream_t st, const long long* hist, const int* first, int G, int B, int bins_per_semitone, double min_conf, int min_peaks,
                             double* est, float* eff_bins) {
    A2S_REQUIRE(first && est && (B == 0 || (hist && eff_bins)), "tuning_estimate: null hist, first, est or eff_bins");
    A2S_REQUIRE(G >= 0 && G <= 65535 && B >= 0, "tuning_estimate: needs 0 <= G <= 65535 and B >= 0 (got G = %d, B = %d)", G, B);
    A2S_REQUIRE(bins_per_semitone >= 1 && bins_per_semitone <= 64, "tuning_estimate: needs 1 <= bins_per_semitone <= 64 (got %d)", bins_per_semitone);
    A2S_REQUIRE(min_conf == min_conf && min_conf - min_conf == 0.0 && min_peaks >= 0, "tuning_estimate: needs a finite min_conf and min_peaks >= 0 (got %g, %d)",
                min_conf, min_peaks);
    if (G == 0) return A2S_OK;
    hipLaunchKernelGGL(tuning_estimate, dim3(G), dim3(TE_THREADS), 0, st, hist, first, B, bins_per_semitone, min_conf, min_peaks, est, eff_bins);
    A2S_CHECK_LAUNCH("tuning_estimate");
    __atomic_fetch_add(&tuning_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_tuning_launches_impl(void) { return (int)__atomic_load_n(&tuning_launches, __ATOMIC_RELAXED); }
