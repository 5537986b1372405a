// Room acoustics of the rendered synthetic corpus: every clip's waveform is convolved with a synthetic impulse response of its own,
// between the synthesiser (a2s_render.hip) and the VQT.  The float64 definition is tests/room_oracle.py.
//
// params (B, 4) int32 per clip, computed by the host in float64: [pre, L, wet f32 bits, decay f32 bits].  L is clamped to [1, L_max] on the device.
// room_ir: ir[b][k], k in [0, L_max):  1 at k = 0;  0 at 0 < k < pre and at k >= L;  wet * u(k) * exp(-(k - pre) * decay) at pre <= k < L,
//     u(k) = (hash32(room_seed + (k + 3) * 0x9E3779B9) >> 8) * 2^-23 - 1  (hash32 and the constant as in a2s_render.hip).
//     Grid (ceil(L_max / 256), B), one tap per thread.  Bounds: stores at [0, L_max) of clip b's row of ir only.
// fir_rows: y[b][n] = sum_{k = 0 .. min(L - 1, n)} ir[b][k] * x[b][n - k], n in [0, n_samples): direct form, fp32 FMAs, k ascending.
//     Grid (ceil(n_samples / FIR_TILE), B), 256 threads, FIR_R = 8 CONSECUTIVE outputs per thread in registers.  A tile at t0 uses the taps below
//     Leff = min(L, t0 + FIR_TILE) (a later tap meets only the zero history of every sample of the tile) and walks them in chunks of FIR_CHUNK:
//     per chunk at c0 the workgroup stages xs[i] = x[t0 - c0 - FIR_CHUNK + i], i in [0, FIR_TILE + FIR_CHUNK), in LDS -- zero where the index is
//     below 0 or not below n_samples -- and then takes the chunk 8 steps at a time.  The 8 outputs are 4 pairs (y[n0 + 2p], y[n0 + 2p + 1]) for the
//     packed fp32 FMA, and the ODD output of a pair runs one tap ahead of the even one: in step s the even output takes tap s and the odd one tap
//     s + 1, and both meet the same sample x[n0 + 2p - s].  So the packed FMA broadcasts ONE register of the window to both halves and takes the
//     taps (h[s], h[s + 1]) from a scalar register pair; with both outputs on the same tap every odd tap would need two window registers put
//     together first (a fifth of the vector instructions of the first version of this kernel).  Tap 0 of the odd outputs is taken before the first
//     step and the clip's last tap by the even outputs alone, so no product with a made-up zero is formed anywhere: a sample is the sum of its own
//     products, k ascending, and of nothing else.  For the steps s0 .. s0 + 7 a thread needs the 14 samples x[n0 - s0 - 7 .. n0 - s0 + 6]: the upper 8
//     of its window are the lower 8 of the block before, so each block reads 8 new floats (two 16-byte LDS reads at a multiple of 32 bytes) for
//     its 64 FMAs.  The taps are the same for the whole workgroup: they are read through the scalar unit straight from ir (9 consecutive floats per
//     block), never at or behind Leff: the last, partial block of a clip reads its taps one by one under s < Leff, so that what lies in ir behind L
//     (NaN included) never reaches a product.
//     One thread forms a sample's whole sum and the tile grid is anchored at sample 0: a sample's bits do not depend on B, on the other clips or
//     on n_samples.  No atomics, nothing persistent, no waits between workgroups, plain loads and vector stores only.
//     Bounds: x is read at [0, n_samples) of clip b's row, ir at [0, Leff) of clip b's row, y is written at [0, n_samples) of clip b's row; LDS reads at
//     [8 * tid + FIR_CHUNK - kb - 8, 8 * tid + FIR_CHUNK - kb + 8), kb in [0, FIR_CHUNK) a multiple of 8: inside [0, FIR_TILE + FIR_CHUNK).
#include "a2s_internal.h"

#define FIR_THREADS 256
#define FIR_R 8
#define FIR_TILE (FIR_THREADS * FIR_R)
#define FIR_CHUNK 512
#define FIR_LDS (FIR_TILE + FIR_CHUNK)
#define RI_THREADS 256

static long long room_launches = 0;

__device__ __forceinline__ unsigned ro_hash32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__global__ __launch_bounds__(RI_THREADS) void room_ir(const unsigned* __restrict__ room_seed, const int* __restrict__ params, float* __restrict__ ir,
                                                      long ir_bstride, int L_max) {
    const int b = blockIdx.y, k = blockIdx.x * RI_THREADS + threadIdx.x;
    if (k >= L_max) return;
    const int* p = params + 4 * (long)b;
    const int pre = p[0], L = min(max(p[1], 1), L_max);
    float h = 0.f;
    if (k == 0) {
        h = 1.0f;
    } else if (k >= pre && k < L) {
        const float wet = __int_as_float(p[2]), decay = __int_as_float(p[3]);
        const unsigned hsh = ro_hash32(room_seed[b] + (unsigned)(k + 3) * 0x9E3779B9u);
        const float u = (float)(hsh >> 8) * 0x1p-23f - 1.0f;
        h = wet * u * expf(-(float)(k - pre) * decay);
    }
    ir[(long)b * ir_bstride + k] = h;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// One step on a thread's 8 outputs, held as 4 pairs (y[2p], y[2p + 1]): the even output takes tap s, the odd one tap s + 1 -- both meet the SAME sample
// x[n0 + 2p - s], so the packed FMA broadcasts one register of the window and no pair of registers has to be put together.  w[8 + i] = x[n0 - s0 + i].
template <int DS>
__device__ __forceinline__ void fir_step(f32x2 (&acc)[4], float h_even, float h_odd, const float (&w)[16]) {
    const f32x2 hh = {h_even, h_odd};
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = __builtin_elementwise_fma(hh, f32x2(w[8 + 2 * p - DS]), acc[p]);
}

template <int DS>
__device__ __forceinline__ void fir_steps(f32x2 (&acc)[4], const float (&hk)[9], const float (&w)[16]) {
    fir_step<DS>(acc, hk[DS], hk[DS + 1], w);
    if constexpr (DS < 7) fir_steps<DS + 1>(acc, hk, w);
}

// the last steps of a clip, one by one: steps below `packed` are whole, the step `packed` itself (the clip's last tap) belongs to the even outputs alone
template <int DS>
__device__ __forceinline__ void fir_tail(f32x2 (&acc)[4], const float* __restrict__ h, int s0, int packed, const float (&w)[16]) {
    const int s = s0 + DS;
    if (s < packed) {
        fir_step<DS>(acc, h[s], h[s + 1], w);
    } else if (s == packed) {
        const float hl = h[s];
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[p].x = fmaf(hl, w[8 + 2 * p - DS], acc[p].x);
    }
    if constexpr (DS < 7) fir_tail<DS + 1>(acc, h, s0, packed, w);
}

#define FIR_WINDOW(lo0, lo1, hi0, hi1) {lo0[0], lo0[1], lo0[2], lo0[3], lo1[0], lo1[1], lo1[2], lo1[3], hi0[0], hi0[1], hi0[2], hi0[3], hi1[0], hi1[1], hi1[2], hi1[3]}

__global__ __launch_bounds__(FIR_THREADS) void fir_rows(const float* __restrict__ x, long x_bstride, const float* __restrict__ ir, long ir_bstride,
                                                        const int* __restrict__ params, float* __restrict__ y, long y_bstride, int n_samples, int L_max,
                                                        int x_vec, int y_vec) {
    __shared__ __attribute__((aligned(16))) float xs[FIR_LDS];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int t0 = blockIdx.x * FIR_TILE;
    const float* __restrict__ xb = x + (long)b * x_bstride;
    const float* __restrict__ hb = ir + (long)b * ir_bstride;
    const int L = min(max(params[4 * (long)b + 1], 1), L_max);
    const int Leff = (int)min((long)L, (long)t0 + FIR_TILE);
    f32x2 acc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = f32x2(0.f);

    for (int c0 = 0; c0 < Leff; c0 += FIR_CHUNK) {
        // ---- stage the chunk's window of x: xs[i] = x[g0 + i] (g0 is a multiple of 4, and so is every group's first index)
        const long g0 = (long)t0 - c0 - FIR_CHUNK;
        if (c0 > 0) __syncthreads();          // (the steps of the chunk before still read xs)
        for (int i = tid * 4; i < FIR_LDS; i += FIR_THREADS * 4) {
            const long g = g0 + i;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (x_vec && g >= 0 && g + 4 <= (long)n_samples) {
                v = *reinterpret_cast<const f32x4*>(xb + g);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (g + e >= 0 && g + e < (long)n_samples) v[e] = xb[g + e];
            }
            *reinterpret_cast<f32x4*>(xs + i) = v;
        }
        __syncthreads();
        // ---- the chunk's steps, 8 per block; the window slides down by 8 floats per block
        const int steps = min(Leff - c0, FIR_CHUNK);                  // step s: tap s for the even outputs, tap s + 1 for the odd ones
        const int packed = min(Leff - 1 - c0, FIR_CHUNK);             // the steps of this chunk whose tap s + 1 exists
        const int full = packed & ~7;
        const float* xw = xs + tid * FIR_R + FIR_CHUNK;               // x[n0 - c0]
        f32x4 hi0 = *reinterpret_cast<const f32x4*>(xw), hi1 = *reinterpret_cast<const f32x4*>(xw + 4);
        if (c0 == 0) {                                                // tap 0 of the odd outputs: they run one tap ahead from here on
            const float h0 = hb[0];
            acc[0].y = h0 * hi0[1], acc[1].y = h0 * hi0[3], acc[2].y = h0 * hi1[1], acc[3].y = h0 * hi1[3];
        }
        int kb = 0;
#pragma unroll 2
        for (; kb < full; kb += 8) {
            const f32x4 lo0 = *reinterpret_cast<const f32x4*>(xw - kb - 8), lo1 = *reinterpret_cast<const f32x4*>(xw - kb - 4);
            float hk[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) hk[t] = hb[c0 + kb + t];
            const float w[16] = FIR_WINDOW(lo0, lo1, hi0, hi1);
            fir_steps<0>(acc, hk, w);
            hi0 = lo0;
            hi1 = lo1;
        }
        if (kb < steps) {                     // the clip's last, partial block
            const f32x4 lo0 = *reinterpret_cast<const f32x4*>(xw - kb - 8), lo1 = *reinterpret_cast<const f32x4*>(xw - kb - 4);
            const float w[16] = FIR_WINDOW(lo0, lo1, hi0, hi1);
            fir_tail<0>(acc, hb + c0, kb, packed, w);
        }
    }

    const int n0 = t0 + tid * FIR_R;
    if (n0 >= n_samples) return;
    float* dst = y + (long)b * y_bstride + n0;
    if (y_vec && n0 + FIR_R <= n_samples) {
        *reinterpret_cast<f32x4*>(dst) = f32x4{acc[0].x, acc[0].y, acc[1].x, acc[1].y};
        *reinterpret_cast<f32x4*>(dst + 4) = f32x4{acc[2].x, acc[2].y, acc[3].x, acc[3].y};
    } else {
#pragma unroll
        for (int j = 0; j < FIR_R; ++j)
            if (n0 + j < n_samples) dst[j] = acc[j >> 1][j & 1];
    }
}

int a2s_room_ir_impl(hipStream_t st, const unsigned* room_seed, const int* params, int B, float* ir, long ir_bstride, int L_max) {
    A2S_REQUIRE(room_seed && params && ir, "room_ir: null room_seed, params or ir");
    A2S_REQUIRE(B >= 0 && B <= 65535, "room_ir: needs 0 <= B <= 65535 (got %d)", B);
    A2S_REQUIRE(L_max >= 1 && ir_bstride >= L_max, "room_ir: needs L_max >= 1 and an ir stride >= L_max (got L_max = %d, stride = %ld)", L_max, ir_bstride);
    if (B == 0) return A2S_OK;
    hipLaunchKernelGGL(room_ir, dim3(a2s_cdiv(L_max, RI_THREADS), B), dim3(RI_THREADS), 0, st, room_seed, params, ir, ir_bstride, L_max);
    A2S_CHECK_LAUNCH("room_ir");
    __atomic_fetch_add(&room_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_fir_rows_impl(hipStream_t st, const float* x, long x_bstride, const float* ir, long ir_bstride, const int* params, float* y, long y_bstride, int B,
                      int n_samples, int L_max) {
    A2S_REQUIRE(x && ir && params && y, "fir_rows: null x, ir, params or y");
    A2S_REQUIRE(x != y, "fir_rows: works out of place (x == y)");
    A2S_REQUIRE(B >= 0 && B <= 65535, "fir_rows: needs 0 <= B <= 65535 (got %d)", B);
    A2S_REQUIRE(n_samples >= 1 && L_max >= 1, "fir_rows: needs n_samples >= 1 and L_max >= 1 (got n_samples = %d, L_max = %d)", n_samples, L_max);
    A2S_REQUIRE(x_bstride >= n_samples && y_bstride >= n_samples && ir_bstride >= L_max,
                "fir_rows: needs x and y strides >= n_samples and an ir stride >= L_max (got %ld, %ld, %ld for n_samples = %d, L_max = %d)", x_bstride, y_bstride,
                ir_bstride, n_samples, L_max);
    if (B == 0) return A2S_OK;
    const int x_vec = (((uintptr_t)x & 15) == 0 && x_bstride % 4 == 0) ? 1 : 0;
    const int y_vec = (((uintptr_t)y & 15) == 0 && y_bstride % 4 == 0) ? 1 : 0;
    hipLaunchKernelGGL(fir_rows, dim3(a2s_cdiv(n_samples, FIR_TILE), B), dim3(FIR_THREADS), 0, st, x, x_bstride, ir, ir_bstride, params, y, y_bstride, n_samples,
                       L_max, x_vec, y_vec);
    A2S_CHECK_LAUNCH("fir_rows");
    __atomic_fetch_add(&room_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_fir_tile_samples_impl(void) { return FIR_TILE; }
int a2s_fir_tap_chunk_impl(void) { return FIR_CHUNK; }
int a2s_room_launches_impl(void) { return (int)__atomic_load_n(&room_launches, __ATOMIC_RELAXED); }
