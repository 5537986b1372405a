// Transposition augmentation of a training batch on the device: the score is respelled, the feature rows are shifted.
//
// transpose_targets: one workgroup of 256 threads per clip.  Clip b has s = semitones[b] and, per bar, the row interval[s + 6][key[b][bar]] of
//     token_map (bars of one clip may carry different keys: they share s and differ in the row).  Pass 1 reads every key and token of the clip and
//     ORs "not representable" over the workgroup: s outside [-6, 6], a key outside [0, 14), a row outside [0, n_rows), a token outside [0, V) or a
//     token that maps to -1.  Pass 2 (only if nothing was flagged and s != 0) rewrites upper / lower in place, then -- behind a barrier, because the
//     rows are found from the OLD keys -- the keys.  Thread 0 writes eff_bins[b] = float(bins_per_semitone * s) + detune[b] (representable) or
//     detune[b], and adds to counters[0 .. 2] = clips seen, clips transposed (s != 0 and representable), clips kept because not representable.
//     Bounds: key [b * bars, (b + 1) * bars), upper [b * bars * U, ...), lower [b * bars * L, ...), the tables at checked indices only.
// shift_bins: y[b][t][j] = (1 - a) x[b][t][j - m] + a x[b][t][j - m - 1], x = 0 outside [0, F), n = eff_bins[b], m = floor(n), a = n - m.
//     A copy whose source window is misaligned by m floats.  Grid (ceil(rows / 16), B), block (128, 2): threadIdx.x walks the columns (four floats
//     per thread when F % 4 == 0 and y is 16-byte aligned: F = 480 is 120 of 128 lanes), threadIdx.y and an unrolled loop of 8 walk the
//     workgroup's 16 rows, so a thread has eight independent 16-byte loads in flight.  m and a are uniform per workgroup; no index is divided.  A
//     group of four outputs whose taps all lie inside the row loads one 4-byte-aligned 16-byte vector (and, with a != 0, the one float in front of it:
//     a hit in the line the neighbouring lane fetched); a group at the row's edge takes guarded scalar loads.  Every store is a whole aligned 16-byte
//     vector.  a == 0 selects x itself (no arithmetic): the shifted input bit for bit, n == 0 a copy.  |n| >= F + 1, or n not finite: zeros.
//     Bounds: loads at columns [0, F) of row t < rows of clip b only; stores likewise.
#include "a2s_internal.h"

#define AUG_THREADS 256
#define AUG_SHIFTS 13          // s = -6 .. 6
#define AUG_KEYS 14
#define SB_TX 128
#define SB_TY 2
#define SB_ROWS 16

static long long aug_launches = 0;

__global__ __launch_bounds__(AUG_THREADS) void transpose_targets(const int* __restrict__ new_key, const int* __restrict__ interval,
                                                                 const int* __restrict__ token_map, int n_rows, int V, const int* __restrict__ semitones,
                                                                 const float* __restrict__ detune, long long* __restrict__ key, long long* __restrict__ upper,
                                                                 long long* __restrict__ lower, int bars, int U, int L, int bins_per_semitone,
                                                                 float* __restrict__ eff_bins, int* __restrict__ counters) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int s = semitones[b];
    const bool s_ok = s >= -(AUG_SHIFTS / 2) && s <= AUG_SHIFTS / 2;
    long long* kb = key + (long)b * bars;
    long long* ub = upper + (long)b * bars * U;
    long long* lb = lower + (long)b * bars * L;
    const int* irow = interval + (s_ok ? s + AUG_SHIFTS / 2 : 0) * AUG_KEYS;

    int bad = s_ok ? 0 : 1;
    if (s_ok) {
        for (int bar = 0; bar < bars; ++bar) {
            const long long k = kb[bar];
            if (k < 0 || k >= AUG_KEYS) { bad = 1; continue; }
            const int row = irow[k];
            if (row < 0 || row >= n_rows) { bad = 1; continue; }
            const int* map = token_map + (long)row * V;
            for (int i = tid; i < U; i += AUG_THREADS) {
                const long long t = ub[(long)bar * U + i];
                if (t < 0 || t >= V || map[t] < 0 || map[t] >= V) bad = 1;
            }
            for (int i = tid; i < L; i += AUG_THREADS) {
                const long long t = lb[(long)bar * L + i];
                if (t < 0 || t >= V || map[t] < 0 || map[t] >= V) bad = 1;
            }
        }
    }
    bad = __syncthreads_or(bad);          // (also the barrier between pass 1's reads and pass 2's writes)

    if (tid == 0) {
        const float d = detune[b];
        eff_bins[b] = bad ? d : (float)(bins_per_semitone * s) + d;
        atomicAdd(&counters[0], 1);
        if (bad) atomicAdd(&counters[2], 1);
        else if (s != 0) atomicAdd(&counters[1], 1);
    }
    if (bad || s == 0) return;

    for (int bar = 0; bar < bars; ++bar) {
        const int* map = token_map + (long)irow[kb[bar]] * V;
        for (int i = tid; i < U; i += AUG_THREADS) {
            long long* p = ub + (long)bar * U + i;
            *p = map[*p];
        }
        for (int i = tid; i < L; i += AUG_THREADS) {
            long long* p = lb + (long)bar * L + i;
            *p = map[*p];
        }
    }
    __syncthreads();                       // every row above came from an old key
    const int* krow = new_key + (s + AUG_SHIFTS / 2) * AUG_KEYS;
    for (int bar = tid; bar < bars; bar += AUG_THREADS) kb[bar] = krow[kb[bar]];
}

// one group of VEC outputs at columns [j, j + VEC) of a row: xr / yr point at the row's column 0
template <int VEC>
__device__ __forceinline__ void sb_group(const float* __restrict__ xr, float* __restrict__ yr, int j, int F, int m, float a, bool frac) {
    const int c = j - m;                   // source column of output j
    if constexpr (VEC == 4) {
        f32x4 x0, x1;
        if (c - (frac ? 1 : 0) >= 0 && c + 3 < F) {
            __builtin_memcpy(&x0, xr + c, 16);                         // 4-byte aligned
            x1 = f32x4{frac ? xr[c - 1] : 0.f, x0.x, x0.y, x0.z};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c0 = c + i, c1 = c + i - 1;
                x0[i] = (c0 >= 0 && c0 < F) ? xr[c0] : 0.f;
                x1[i] = (frac && c1 >= 0 && c1 < F) ? xr[c1] : 0.f;
            }
        }
        *reinterpret_cast<f32x4*>(yr + j) = frac ? (1.0f - a) * x0 + a * x1 : x0;
    } else {
        const float x0 = (c >= 0 && c < F) ? xr[c] : 0.f;
        const float x1 = (frac && c - 1 >= 0 && c - 1 < F) ? xr[c - 1] : 0.f;
        yr[j] = frac ? (1.0f - a) * x0 + a * x1 : x0;
    }
}

template <int VEC>
__global__ __launch_bounds__(SB_TX * SB_TY) void shift_bins(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ eff_bins,
                                                            int rows, int F) {
    const int b = blockIdx.y, tx = threadIdx.x, ty = threadIdx.y;
    const float n = eff_bins[b];
    const bool zero = !(fabsf(n) < (float)F + 1.0f);                     // (also a NaN)
    const float fl = zero ? 0.f : floorf(n);
    const int m = (int)fl;
    const float a = zero ? 0.f : n - fl;
    const bool frac = a != 0.f;
    const long clip = (long)b * rows * F;
    const int t0 = blockIdx.x * SB_ROWS + ty;
    if (zero) {
#pragma unroll
        for (int r = 0; r < SB_ROWS / SB_TY; ++r) {
            const int t = t0 + r * SB_TY;
            if (t >= rows) break;
            float* yr = y + clip + (long)t * F;
            for (int j = tx * VEC; j < F; j += SB_TX * VEC) {
                if (VEC == 4) *reinterpret_cast<f32x4*>(yr + j) = f32x4{0.f, 0.f, 0.f, 0.f};
                else yr[j] = 0.f;
            }
        }
        return;
    }
    constexpr int NR = SB_ROWS / SB_TY;
    const long step = (long)SB_TY * F;                                  // from one of this thread's rows to its next
    const float* x0r = x + clip + (long)t0 * F;
    float* y0r = y + clip + (long)t0 * F;
    const bool full = t0 + (NR - 1) * SB_TY < rows;                     // all NR rows of this thread exist
    for (int j = tx * VEC; j < F; j += SB_TX * VEC) {
        if constexpr (VEC == 4) {
            const int c = j - m;
            // the column group is interior or at the edge for every row alike: the NR rows' loads are issued together, then the stores
            if (full && c - (frac ? 1 : 0) >= 0 && c + 3 < F) {
                f32x4 v[NR];
                float p[NR];
#pragma unroll
                for (int r = 0; r < NR; ++r) __builtin_memcpy(&v[r], x0r + r * step + c, 16);          // 4-byte aligned
                if (frac) {
#pragma unroll
                    for (int r = 0; r < NR; ++r) p[r] = x0r[r * step + c - 1];
#pragma unroll
                    for (int r = 0; r < NR; ++r)
                        *reinterpret_cast<f32x4*>(y0r + r * step + j) = (1.0f - a) * v[r] + a * f32x4{p[r], v[r].x, v[r].y, v[r].z};
                } else {
#pragma unroll
                    for (int r = 0; r < NR; ++r) *reinterpret_cast<f32x4*>(y0r + r * step + j) = v[r];
                }
                continue;
            }
        }
        for (int r = 0; r < NR && t0 + r * SB_TY < rows; ++r) sb_group<VEC>(x0r + r * step, y0r + r * step, j, F, m, a, frac);
    }
}

int a2s_transpose_targets_impl(hipStream_t st, const int* new_key, const int* interval, const int* token_map, int n_rows, int V, const int* semitones,
                               const float* detune, long long* key, long long* upper, long long* lower, int bars, int U, int L, int bins_per_semitone,
                               float* eff_bins, int* counters, int B) {
    A2S_REQUIRE(new_key && interval && token_map && semitones && detune && key && upper && lower && eff_bins && counters,
                "transpose_targets: null table, draw, target, eff_bins or counter pointer");
    A2S_REQUIRE(B >= 0 && n_rows >= 1 && V >= 1 && bars >= 1 && U >= 1 && L >= 1 && bins_per_semitone >= 1,
                "transpose_targets: needs B >= 0, n_rows >= 1, V >= 1, bars >= 1, U >= 1, L >= 1 and bins_per_semitone >= 1 (got B = %d, n_rows = %d, V = %d, bars = %d, "
                "U = %d, L = %d, bins_per_semitone = %d)", B, n_rows, V, bars, U, L, bins_per_semitone);
    A2S_REQUIRE(bins_per_semitone <= 1 << 20, "transpose_targets: bins_per_semitone %d is not a feature resolution", bins_per_semitone);
    if (B == 0) return A2S_OK;
    hipLaunchKernelGGL(transpose_targets, dim3(B), dim3(AUG_THREADS), 0, st, new_key, interval, token_map, n_rows, V, semitones, detune, key, upper, lower,
                       bars, U, L, bins_per_semitone, eff_bins, counters);
    A2S_CHECK_LAUNCH("transpose_targets");
    __atomic_fetch_add(&aug_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_shift_bins_impl(hipStream_t st, const float* x, float* y, const float* eff_bins, int B, int rows, int F) {
    A2S_REQUIRE(x && y && eff_bins, "shift_bins: null x, y or eff_bins");
    A2S_REQUIRE(x != y, "shift_bins: works out of place (x == y)");
    A2S_REQUIRE(B >= 0 && rows >= 1 && F >= 1, "shift_bins: needs B >= 0, rows >= 1 and F >= 1 (got B = %d, rows = %d, F = %d)", B, rows, F);
    A2S_REQUIRE(B <= 65535, "shift_bins: at most 65535 clips per call (got %d)", B);
    A2S_REQUIRE((long long)rows * F < (1LL << 31), "shift_bins: a clip of %d rows x %d bins is too large", rows, F);
    if (B == 0) return A2S_OK;
    const dim3 grid(a2s_cdiv(rows, SB_ROWS), B), block(SB_TX, SB_TY);
    if (a2s_row_vec_width(F, y) == 4) {
        hipLaunchKernelGGL(shift_bins<4>, grid, block, 0, st, x, y, eff_bins, rows, F);
    } else {
        hipLaunchKernelGGL(shift_bins<1>, grid, block, 0, st, x, y, eff_bins, rows, F);
    }
    A2S_CHECK_LAUNCH("shift_bins");
    __atomic_fetch_add(&aug_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_augment_launches_impl(void) { return (int)__atomic_load_n(&aug_launches, __ATOMIC_RELAXED); }
