// The tiled weight-gradient kernels of the ConvStack's 3x3 convolutions (layouts and the forward / data-gradient kernels: a2s_conv.hip) and
// their dispatcher: the first layer (Cin = 1), and every launch the row-streaming kernel of a2s_conv_wrows.hip is not eligible for.
#include "a2s_internal.h"

// ------------------------------------------------------------------------------------------- conv weight gradient
// Optional fused BatchNorm backward of the layer's OUTPUT side: instead of a ready dy the kernel gets g (gradient wrt the activation
// relu(bn(y))) and y (the layer's pre-BN output) and forms  dy = scale_c * (g' - c1_c - (y - mean_c) * invstd_c * c2_c),
// g' = g where bn(y) > 0 else 0  (exactly bn_bwd_apply) while staging -- and writes dy out for the data-gradient convolution that
// follows.  The weight-gradient kernels are MFMA-bound with HBM bandwidth to spare, so the separate apply pass (read g, y, write dx:
// 71 GB per 40-channel layer at B = 256) disappears from the step.
struct BnBwdFuse {
    const float* y;          // (B, T, Cout, F) pre-BN output of this layer; null = dy is given ready-made
    const float* mean; const float* invstd; const float* scale; const float* shift;
    const float* c12;        // [Cout][2] = (sum g', sum g' xhat) / count  (bn_bwd_finalize)
    float* dy_out;           // (B, T, Cout, F) or null
};
__device__ __forceinline__ float bn_bwd_value(float g, float yv, float mean, float invstd, float scale, float shift, float c1, float c2) {
    const float gm = (yv * scale + shift > 0.f) ? g : 0.f;
    return scale * (gm - c1 - (yv - mean) * invstd * c2);
}

// dW[co][ci][tap] += sum_{b,t,f} dy[b,t,co,f] * in[b, t+dt-1, ci, f+df-1],  in = relu(x*scale+shift) (or x).
// GEMM view on v_mfma_f32_16x16x4_f32: M = co, N = (ci_local, tap) of one 20-channel chunk (blockIdx.y), K = positions
// (4 consecutive f per MFMA).  gridDim.x persistent workgroups walk the (b, 4-row strip, 32-column) tiles; each writes
// ONE partial slab [Cout][180]; wgrad_reduce sums the slabs in fixed order (deterministic).
template <int COUT, bool BN>
__global__ __launch_bounds__(256, 3) void conv3x3_wgrad(const float* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ in_scale, const float* __restrict__ in_shift,
                                                     float* __restrict__ partial, int B, int T, int F, int Cin, BnBwdFuse bn) {
    constexpr int MT = (COUT + 15) / 16;
    constexpr int NTW = 3;                               // n-tiles per wave: 4 waves x 3 x 16 = 192 >= 180
    // LDS layouts chosen by exhaustive search for conflict-free fragment reads (each half-wave = 16 M/N indices x 2 k-slots must
    // hit 32 distinct banks; PMC on the first layout: 77 % of the LDS cycles were bank-conflict cycles, 8-way on the dy image):
    //   dy   : [r][co][34]  -> lane stride 34 floats (== 2 mod 32) between output channels;
    //   input: [c][6 rows][36], plane 240; interior at column 2 (halos at 1 / 34).  Rows are 8-byte aligned -> float2 stores.
    constexpr int DRS = CV_FT + 2;                       // 34
    constexpr int WRS = 36;
    constexpr int WPL = 240;
    constexpr int WC0 = 2;                               // LDS column of f0
    __shared__ __attribute__((aligned(16))) float lin[CV_CK * WPL];
    __shared__ __attribute__((aligned(16))) float ldy[CV_TR * MT * 16 * DRS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int c0 = blockIdx.y * CV_CK;
    const int tilesF = (F + CV_FT - 1) / CV_FT, tilesT = (T + CV_TR - 1) / CV_TR;
    const long ntiles = (long)B * tilesT * tilesF;
    const bool vec_ok = (F % 4 == 0) && ((((uintptr_t)x | (uintptr_t)dy) & 15) == 0);

    int boff[NTW];                                       // LDS offset of this lane's (ci, dt, df) column per n-tile
    bool bok[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int n = (wave * NTW + j) * 16 + li;
        bok[j] = n < CV_CK * 9 && (c0 + n / 9) < Cin;
        const int c = n / 9, tap = n % 9;
        boff[j] = bok[j] ? c * WPL + (tap / 3) * WRS + (tap % 3) + WC0 - 1 : 0;
    }
    f32x4 acc[MT][NTW];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // rows of the dy image that belong to padded output channels (co >= COUT) stay zero for the whole kernel
    for (int e = tid; e < CV_TR * (MT * 16 - COUT) * DRS; e += 256) {
        const int r = e / ((MT * 16 - COUT) * DRS), rem = e % ((MT * 16 - COUT) * DRS);
        ldy[(r * MT * 16 + COUT) * DRS + rem] = 0.f;
    }

    // XCD-aware walk (see conv3x3_wgrad_split): each XCD's workgroups (id % 8) share a contiguous eighth of the tile space
    long t_begin = blockIdx.x, t_end = ntiles, t_step = gridDim.x;
    if (gridDim.x % 8 == 0) {
        const long chunk = (ntiles + 7) / 8;
        t_begin = (blockIdx.x % 8) * chunk + blockIdx.x / 8;
        t_end = min(ntiles, (long)(blockIdx.x % 8 + 1) * chunk);
        t_step = gridDim.x / 8;
    }
    for (long tile = t_begin; tile < t_end; tile += t_step) {
        long bid = tile;
        const int ft = (int)(bid % tilesF); bid /= tilesF;
        const int tt = (int)(bid % tilesT); const int b = (int)(bid / tilesT);
        const int t0 = tt * CV_TR, f0 = ft * CV_FT;
        // ---- staging: ALL global loads of the tile are issued first (one round trip instead of ~10 dependent ones), then transformed
        // (producer's BN+ReLU) and stored to LDS
        constexpr int XIT = (CV_CK * (CV_TR + 2) * (CV_FT / 4) + 255) / 256;      // 4
        constexpr int DIT = (COUT * CV_TR * (CV_FT / 4) + 255) / 256;             // 5 (Cout 40) / 3 (Cout 20)
        f32x4 xreg[XIT], dreg[DIT], yreg[BN ? DIT : 1];
        float hreg = 0.f;
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            const int e = tid + 256 * it;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (e < CV_CK * (CV_TR + 2) * (CV_FT / 4)) {
                const int j = e % (CV_FT / 4), row = e / (CV_FT / 4);
                const int r = row % (CV_TR + 2), c = row / (CV_TR + 2);
                const int t = t0 + r - 1, f = f0 + 4 * j, ci = c0 + c;
                if (t >= 0 && t < T && f < F && ci < Cin) {
                    const float* src = x + (((long)b * T + t) * Cin + ci) * F + f;
                    if (vec_ok && f + 3 < F) v = *reinterpret_cast<const f32x4*>(src);
                    else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) if (f + q < F) v[q] = src[q];
                    }
                }
            }
            xreg[it] = v;
        }
        if (tid < CV_CK * (CV_TR + 2) * 2) {
            const int side = tid & 1, row = tid >> 1;
            const int r = row % (CV_TR + 2), c = row / (CV_TR + 2);
            const int t = t0 + r - 1, f = side ? f0 + CV_FT : f0 - 1, ci = c0 + c;
            hreg = (t >= 0 && t < T && f >= 0 && f < F && ci < Cin) ? x[(((long)b * T + t) * Cin + ci) * F + f] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < DIT; ++it) {
            const int e = tid + 256 * it;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (e < COUT * CV_TR * (CV_FT / 4)) {
                const int j = e % (CV_FT / 4), row = e / (CV_FT / 4);
                const int r = row % CV_TR, co = row / CV_TR;
                const int t = t0 + r, f = f0 + 4 * j;
                f32x4 yv = {0.f, 0.f, 0.f, 0.f};
                if (t < T && f < F) {
                    const long off = (((long)b * T + t) * COUT + co) * F + f;
                    if (vec_ok && f + 3 < F) {
                        v = *reinterpret_cast<const f32x4*>(dy + off);
                        if (BN) yv = *reinterpret_cast<const f32x4*>(bn.y + off);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) if (f + q < F) { v[q] = dy[off + q]; if (BN) yv[q] = bn.y[off + q]; }
                    }
                }
                if (BN) yreg[it] = yv;
            }
            dreg[it] = v;
        }
        __syncthreads();                   // previous tile fully consumed (the loads above are already in flight)
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            const int e = tid + 256 * it;
            if (e < CV_CK * (CV_TR + 2) * (CV_FT / 4)) {
                const int j = e % (CV_FT / 4), row = e / (CV_FT / 4);
                const int r = row % (CV_TR + 2), c = row / (CV_TR + 2);
                const int t = t0 + r - 1, f = f0 + 4 * j, ci = c0 + c;
                f32x4 v = xreg[it];
                if (in_scale && t >= 0 && t < T && f < F && ci < Cin) {
                    const float sc = in_scale[ci], sh = in_shift[ci];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = (f + q < F) ? fmaxf(v[q] * sc + sh, 0.f) : 0.f;
                }
                float2* dst = reinterpret_cast<float2*>(lin + c * WPL + r * WRS + WC0 + 4 * j);
                dst[0] = make_float2(v[0], v[1]); dst[1] = make_float2(v[2], v[3]);
            }
        }
        if (tid < CV_CK * (CV_TR + 2) * 2) {
            const int side = tid & 1, row = tid >> 1;
            const int r = row % (CV_TR + 2), c = row / (CV_TR + 2);
            const int t = t0 + r - 1, f = side ? f0 + CV_FT : f0 - 1, ci = c0 + c;
            float v = hreg;
            if (in_scale && t >= 0 && t < T && f >= 0 && f < F && ci < Cin) v = fmaxf(v * in_scale[ci] + in_shift[ci], 0.f);
            lin[c * WPL + r * WRS + (side ? WC0 + CV_FT : WC0 - 1)] = v;
        }
#pragma unroll
        for (int it = 0; it < DIT; ++it) {
            const int e = tid + 256 * it;
            if (e < COUT * CV_TR * (CV_FT / 4)) {
                const int j = e % (CV_FT / 4), row = e / (CV_FT / 4);
                const int r = row % CV_TR, co = row / CV_TR;
                f32x4 v = dreg[it];
                if (BN) {                   // fused BatchNorm backward (positions outside the image stay 0)
                    const int t = t0 + r, f = f0 + 4 * j;
                    const float mean = bn.mean[co], invstd = bn.invstd[co], sc = bn.scale[co], sh = bn.shift[co];
                    const float c1 = bn.c12[2 * co], c2 = bn.c12[2 * co + 1];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = (t < T && f + q < F) ? bn_bwd_value(v[q], yreg[it][q], mean, invstd, sc, sh, c1, c2) : 0.f;
                    if (bn.dy_out && blockIdx.y == 0 && t < T && f < F) {
                        float* dst = bn.dy_out + (((long)b * T + t) * COUT + co) * F + f;
                        if (vec_ok && f + 3 < F) *reinterpret_cast<f32x4*>(dst) = v;
                        else {
#pragma unroll
                            for (int q = 0; q < 4; ++q) if (f + q < F) dst[q] = v[q];
                        }
                    }
                }
                float2* dst = reinterpret_cast<float2*>(ldy + (r * MT * 16 + co) * DRS + 4 * j);
                dst[0] = make_float2(v[0], v[1]); dst[1] = make_float2(v[2], v[3]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < CV_TR; ++r) {
#pragma unroll
            for (int ks = 0; ks < CV_FT / 4; ++ks) {
                float a[MT], bv[NTW];
#pragma unroll
                for (int i = 0; i < MT; ++i) a[i] = ldy[(r * MT * 16 + i * 16 + li) * DRS + ks * 4 + lk];
#pragma unroll
                for (int j = 0; j < NTW; ++j) bv[j] = bok[j] ? lin[boff[j] + r * WRS + ks * 4 + lk] : 0.f;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NTW; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    // D[row = co (lk*4+r)][col = n (li)]
    float* slab = partial + ((long)blockIdx.y * gridDim.x + blockIdx.x) * COUT * (CV_CK * 9);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            const int n = (wave * NTW + j) * 16 + li;
            if (n >= CV_CK * 9) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = i * 16 + lk * 4 + r;
                if (co < COUT) slab[(long)co * (CV_CK * 9) + n] = acc[i][j][r];
            }
        }
}

// dW[co][c0+ci][tap] += sum over slabs (fixed order)
__global__ void wgrad_reduce(const float* __restrict__ partial, float* __restrict__ dW, int nslabs, int Cout, int Cin, int chunks) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int per = Cout * CV_CK * 9;
    if (idx >= per * chunks) return;
    const int chunk = idx / per, rem = idx % per;
    const int co = rem / (CV_CK * 9), n = rem % (CV_CK * 9);
    const int ci = chunk * CV_CK + n / 9, tap = n % 9;
    if (ci >= Cin) return;
    const float* p = partial + (long)chunk * nslabs * per + rem;
    float s = 0.f;
    for (int i = 0; i < nslabs; ++i) s += p[(long)i * per];
    dW[((long)co * Cin + ci) * 9 + tap] += s;
}

#define WGRAD_SLABS 768

// First layer (Cin = 1): dW[co][tap] = sum_{b,t,f} dy[b,t,co,f] * x[b, t+dt-1, f+df-1].  53 GFLOP at B = 256 against 12 GB of dy: a
// streaming kernel (the MFMA kernel above would spend a full 20-channel chunk on one real input channel).  Persistent workgroups walk
// the (b,t) rows; a row's dy block (Cout x F) and the 3 x (F+2) input window go through LDS; thread = (co, slice of F) keeps its 9
// tap sums in registers; one slab [Cout][9] per workgroup, reduced in fixed order by wgrad_reduce_c1.
#define C1W_PARTS 12
#define C1W_XIT 10                          // float4 loads per thread and row in the fused path (20 x 480 / 4 / 256 = 9.4)
__global__ __launch_bounds__(256) void conv3x3_wgrad_c1(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ partial,
                                                        int B, int T, int F, int Cout, BnBwdFuse bn) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* ldy = sm;                            // Cout * F
    float* lx = sm + Cout * F;                  // 3 * (F + 2)
    __shared__ float lconst[20 * 6];            // per channel: mean, invstd, scale, shift, c1, c2 (fused BatchNorm backward)
    const int tid = threadIdx.x;
    if (bn.y && tid < Cout) {
        float* k = lconst + tid * 6;
        k[0] = bn.mean[tid]; k[1] = bn.invstd[tid]; k[2] = bn.scale[tid]; k[3] = bn.shift[tid]; k[4] = bn.c12[2 * tid]; k[5] = bn.c12[2 * tid + 1];
    }
    const int co = tid / C1W_PARTS, part = tid % C1W_PARTS;
    const int fper = (F + C1W_PARTS - 1) / C1W_PARTS;
    const int fa = part * fper, fb = min(F, fa + fper);
    const bool worker = co < Cout;
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.f;
    const long rows = (long)B * T;
    const bool vec_ok = (F % 4 == 0) && (((uintptr_t)dy & 15) == 0);
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int t = (int)(row % T);
        const long b = row / T;
        __syncthreads();
        const float* drow = dy + row * (long)Cout * F;
        if (bn.y && vec_ok && (((uintptr_t)bn.y & 15) == 0) && Cout * F <= 4 * 256 * C1W_XIT) {
            // fused BatchNorm backward of the dy operand (see BnBwdFuse): all loads of the row first (one round trip), constants from LDS
            const float* yrow = bn.y + row * (long)Cout * F;
            f32x4 g4[C1W_XIT], y4[C1W_XIT];
#pragma unroll
            for (int it = 0; it < C1W_XIT; ++it) {
                const int e = tid + 256 * it;
                if (e < Cout * F / 4) { g4[it] = reinterpret_cast<const f32x4*>(drow)[e]; y4[it] = reinterpret_cast<const f32x4*>(yrow)[e]; }
            }
#pragma unroll
            for (int it = 0; it < C1W_XIT; ++it) {
                const int e = tid + 256 * it;
                if (e < Cout * F / 4) {
                    const int c = (e * 4) / F;
                    const float* k = lconst + c * 6;
                    f32x4 v;
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = bn_bwd_value(g4[it][q], y4[it][q], k[0], k[1], k[2], k[3], k[4], k[5]);
                    reinterpret_cast<f32x4*>(ldy)[e] = v;
                    if (bn.dy_out) reinterpret_cast<f32x4*>(bn.dy_out + row * (long)Cout * F)[e] = v;
                }
            }
        } else if (bn.y) {
            const float* yrow = bn.y + row * (long)Cout * F;
            for (int e = tid; e < Cout * F; e += 256) {
                const int c = e / F;
                const float v = bn_bwd_value(drow[e], yrow[e], bn.mean[c], bn.invstd[c], bn.scale[c], bn.shift[c], bn.c12[2 * c], bn.c12[2 * c + 1]);
                ldy[e] = v;
                if (bn.dy_out) bn.dy_out[row * (long)Cout * F + e] = v;
            }
        } else if (vec_ok) {
            for (int e = tid; e < Cout * F / 4; e += 256) reinterpret_cast<f32x4*>(ldy)[e] = reinterpret_cast<const f32x4*>(drow)[e];
        } else {
            for (int e = tid; e < Cout * F; e += 256) ldy[e] = drow[e];
        }
        for (int e = tid; e < 3 * (F + 2); e += 256) {
            const int r = e / (F + 2), c = e % (F + 2);
            const int tt = t + r - 1, f = c - 1;
            lx[e] = (tt >= 0 && tt < T && f >= 0 && f < F) ? x[(b * T + tt) * F + f] : 0.f;
        }
        __syncthreads();
        if (worker) {
            const float* d = ldy + co * F;
            float w[3][3];                                  // input window, slid along f: 3 new values per position instead of 9
#pragma unroll
            for (int dt = 0; dt < 3; ++dt) { w[dt][1] = lx[dt * (F + 2) + fa]; w[dt][2] = lx[dt * (F + 2) + fa + 1]; }
            for (int f = fa; f < fb; ++f) {
                const float g = d[f];
#pragma unroll
                for (int dt = 0; dt < 3; ++dt) {
                    w[dt][0] = w[dt][1]; w[dt][1] = w[dt][2]; w[dt][2] = lx[dt * (F + 2) + f + 2];
#pragma unroll
                    for (int df = 0; df < 3; ++df) acc[dt * 3 + df] = fmaf(g, w[dt][df], acc[dt * 3 + df]);
                }
            }
        }
    }
    __syncthreads();
    float* red = sm;                            // 256 * 9 floats (fits: Cout * F >= 2304 for the model's F)
#pragma unroll
    for (int k = 0; k < 9; ++k) red[tid * 9 + k] = worker ? acc[k] : 0.f;
    __syncthreads();
    if (tid < Cout * 9) {
        const int c = tid / 9, k = tid % 9;
        float s = 0.f;
        for (int p = 0; p < C1W_PARTS; ++p) s += red[(c * C1W_PARTS + p) * 9 + k];
        partial[(long)blockIdx.x * Cout * 9 + tid] = s;
    }
}

__global__ void wgrad_reduce_c1(const float* __restrict__ partial, float* __restrict__ dW, int nslabs, int n) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    float s = 0.f;
    for (int i = 0; i < nslabs; ++i) s += partial[(long)i * n + idx];
    dW[idx] += s;
}

// The model's case of conv3x3_wgrad_c1 (fused BatchNorm backward, F a multiple of 4 * C1W_PARTS) restructured for the memory system -- same
// rows per workgroup, same order of additions per tap sum, so the slabs are bit-identical:
//   * the NEXT row's dy / y / input loads are issued before the current row's tap sums are computed (the old kernel alternated a load phase
//     and a compute phase per workgroup, 4.1 TB/s);
//   * the tap sums read LDS 16 bytes at a time: one quad of dy and one quad per window row for 4 positions (the old loop: 4 scalar reads
//     per position, 2-4-way bank conflicts -- SQ_LDS_BANK_CONFLICT / SQ_LDS_ACTIVE = 0.67).  The window rows are stored at a stride of
//     F + 8 with x[f] at column 4 + f, so the quads are aligned and the zero borders sit at columns 3 and F + 4.
#define C1W_XN 2                            // input-window quads per thread and row: 3 * F / 4 <= 2 * 256
template <int COUT, int F>
__global__ __launch_bounds__(256, 3) void conv3x3_wgrad_c1_stream(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ partial,
                                                                  int B, int T, BnBwdFuse bn) {
    static_assert(F % (4 * C1W_PARTS) == 0 && 3 * F / 4 <= 256 * C1W_XN && COUT * F <= 4 * 256 * C1W_XIT && COUT * C1W_PARTS <= 256, "shape");
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int LXS = F + 8;
    float* ldy = sm;                            // COUT * F
    float* lx = sm + COUT * F;                  // 3 * LXS
    __shared__ float lconst[COUT * 6];
    const int tid = threadIdx.x;
    if (tid < COUT) {
        float* k = lconst + tid * 6;
        k[0] = bn.mean[tid]; k[1] = bn.invstd[tid]; k[2] = bn.scale[tid]; k[3] = bn.shift[tid]; k[4] = bn.c12[2 * tid]; k[5] = bn.c12[2 * tid + 1];
    }
    const int co = tid / C1W_PARTS, part = tid % C1W_PARTS;
    constexpr int fper = F / C1W_PARTS, nq = COUT * F / 4, nx = 3 * F / 4;      // quads of a dy row, of the 3-row input window
    const int fa = part * fper;
    const bool worker = co < COUT;
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.f;
    const long rows = (long)B * T;
    f32x4 g4[C1W_XIT], y4[C1W_XIT];
    f32x4 xv[C1W_XN];
    auto issue = [&](long row) {
        const f32x4* drow = reinterpret_cast<const f32x4*>(dy + row * (long)COUT * F);
        const f32x4* yrow = reinterpret_cast<const f32x4*>(bn.y + row * (long)COUT * F);
#pragma unroll
        for (int it = 0; it < C1W_XIT; ++it) {
            const int e = tid + 256 * it;
            if (e < nq) { g4[it] = drow[e]; y4[it] = yrow[e]; }
        }
        const int t = (int)(row % T);
#pragma unroll
        for (int it = 0; it < C1W_XN; ++it) {
            const int e = tid + 256 * it, r = e / (F / 4), tt = t + r - 1;
            xv[it] = (e < nx && tt >= 0 && tt < T) ? reinterpret_cast<const f32x4*>(x + (row + r - 1) * F)[e % (F / 4)] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    if (tid < 6) lx[(tid >> 1) * LXS + ((tid & 1) ? F + 4 : 3)] = 0.f;        // the zero borders left and right of the window rows
    if ((long)blockIdx.x < rows) issue(blockIdx.x);
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        __syncthreads();                        // the previous row's tap sums are done with LDS (and lconst is written)
#pragma unroll
        for (int it = 0; it < C1W_XIT; ++it) {
            const int e = tid + 256 * it;
            if (e < nq) {
                const float* k = lconst + ((e * 4) / F) * 6;
                f32x4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = bn_bwd_value(g4[it][q], y4[it][q], k[0], k[1], k[2], k[3], k[4], k[5]);
                reinterpret_cast<f32x4*>(ldy)[e] = v;
                if (bn.dy_out) reinterpret_cast<f32x4*>(bn.dy_out + row * (long)COUT * F)[e] = v;
            }
        }
#pragma unroll
        for (int it = 0; it < C1W_XN; ++it) {
            const int e = tid + 256 * it;
            if (e < nx) *reinterpret_cast<f32x4*>(lx + (e / (F / 4)) * LXS + 4 + 4 * (e % (F / 4))) = xv[it];
        }
        if (row + gridDim.x < rows) issue(row + gridDim.x);      // in flight while this row's tap sums are computed
        __syncthreads();
        if (worker) {
            const float* d = ldy + co * F + fa;
            const float* xr = lx + 4 + fa;
            float left[3];
            f32x4 cur[3];
#pragma unroll
            for (int dt = 0; dt < 3; ++dt) { left[dt] = xr[dt * LXS - 1]; cur[dt] = *reinterpret_cast<const f32x4*>(xr + dt * LXS); }
#pragma unroll 2
            for (int j = 0; j < fper; j += 4) {                 // (fully unrolled, the 40 quad reads are all issued first: 100 spilled registers)
                const f32x4 g = *reinterpret_cast<const f32x4*>(d + j);
#pragma unroll
                for (int dt = 0; dt < 3; ++dt) {
                    const f32x4 nxt = *reinterpret_cast<const f32x4*>(xr + dt * LXS + j + 4);      // only [0] is used past the row's end: the border
                    const float w[6] = {left[dt], cur[dt][0], cur[dt][1], cur[dt][2], cur[dt][3], nxt[0]};
#pragma unroll
                    for (int p = 0; p < 4; ++p)
#pragma unroll
                        for (int df = 0; df < 3; ++df) acc[dt * 3 + df] = fmaf(g[p], w[p + df], acc[dt * 3 + df]);
                    left[dt] = cur[dt][3]; cur[dt] = nxt;
                }
            }
        }
    }
    __syncthreads();
    float* red = sm;                            // 256 * 9 floats
#pragma unroll
    for (int k = 0; k < 9; ++k) red[tid * 9 + k] = worker ? acc[k] : 0.f;
    __syncthreads();
    if (tid < COUT * 9) {
        const int c = tid / 9, k = tid % 9;
        float s = 0.f;
        for (int p = 0; p < C1W_PARTS; ++p) s += red[(c * C1W_PARTS + p) * 9 + k];
        partial[(long)blockIdx.x * COUT * 9 + tid] = s;
    }
}

// ---- weight gradient on the bf16 matrix pipes with 3-term split operands (see conv3x3_bf16x3).  K = positions: a fragment is 8
// consecutive f positions of ONE channel row, so dy (M = co) and the input (N = ci) both stay position-contiguous in LDS; an N-tile is
// 16 input channels at ONE tap, which makes the +-1 column shift of the tap uniform per MFMA: the lane reads the aligned 8 positions plus
// the dword before and after -- df = 1 is the aligned window, df = 0 / 2 are four v_alignbit_b32 each.  One 512-thread workgroup per CU
// walks (clip, 2-row strip, 64-column) tiles; the 9 x ceil(Cin/16) (tap, channel-tile) column tiles are dealt round robin to the 8 waves
// (<= 4 each, 12 accumulator tiles); every other tile accumulates the negated sum (dy negated while staging) against the pipe's
// truncation bias.  One partial slab [Cout][Cin][9] per workgroup, summed in fixed order by wgrad_reduce_c1.
#define W4_XROW 160                       // bytes per staged input row: 80 bf16, interior at element 8 (halo columns at 7 and 72)
#define W4_XCI (4 * W4_XROW + 16)         // 656: channel stride (pad -> conflict-free fragment reads across the 16 channels of a tile)
#define W4_DYCO (2 * 128 + 16)            // 272: output-channel stride of the dy image [co][2 rows][64]
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#ifdef C4_TRACE
// timing instrumentation (tools/conv_trace.py with A2S_TRACE_WGRAD=1), the shape of a2s_conv_trace_read's buffer.  A buffer and a reader
// of this file's own: without relocatable device code a __device__ variable is not shared between translation units
__device__ unsigned long long w4_trace[C4_TRACE_WGS * C4_TRACE_STAGES * 8];
extern "C" int a2s_conv_wgrad_trace_read(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(w4_trace), sizeof(w4_trace));
}
#endif
// TERMS = 3: bf16 three-term split (six products); TERMS = 2: fp16 two-term split (three products), dy scaled by the power of two that
// brings max |dy| (dy_absmax, device scalar; null = unscaled) to 2^12, the slab unscaled on the way out -- see conv3x3_split.
template <int COUT, int TERMS>
__global__ __launch_bounds__(512, 1) void conv3x3_wgrad_split(const float* __restrict__ dy, const float* __restrict__ x,
                                                              const float* __restrict__ in_scale, const float* __restrict__ in_shift,
                                                              float* __restrict__ partial, int B, int T, int F, int Cin,
                                                              const float* __restrict__ dy_absmax, const float* __restrict__ act_absmax) {
    constexpr int MT = (COUT + 15) / 16;
    constexpr int XPL = 48 * W4_XCI;          // bytes per term plane of the input image (48 channel planes; beyond Cin they stay zero)
    constexpr int DPL = MT * 16 * W4_DYCO;
    __shared__ __attribute__((aligned(16))) unsigned char lx[TERMS * XPL];
    __shared__ __attribute__((aligned(16))) unsigned char ldy[TERMS * DPL];
    __shared__ __attribute__((aligned(16))) float lsc[48], lsh[48];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int nc16 = (Cin + 15) / 16, npair = 9 * nc16;
    for (int e = tid; e < TERMS * XPL / 16; e += 512) reinterpret_cast<uint4*>(lx)[e] = make_uint4(0u, 0u, 0u, 0u);
    for (int e = tid; e < TERMS * DPL / 16; e += 512) reinterpret_cast<uint4*>(ldy)[e] = make_uint4(0u, 0u, 0u, 0u);
    float dscale = 1.f, unscale = 1.f;
    if (TERMS == 2 && dy_absmax) {
        const int kd = pow2_scale_exp(*dy_absmax, 12);
        dscale = ldexpf(1.f, kd); unscale = ldexpf(1.f, -kd);
    }
    // act_absmax: device scalar bounding the activated operand relu(x scale_c + shift_c) (a2s_act_bound).  Its power-of-two scale is
    // folded into scale / shift (relu commutes with it) and undone with the slab: the operand's fp16 terms neither overflow nor sink
    // into the subnormal range whatever BatchNorm's gamma is.  Without it the operand is used as it is (and clamped at +-65000).
    int ka = 0;
    if (TERMS == 2 && act_absmax && in_scale) {
        ka = pow2_scale_exp(*act_absmax, 14);
        unscale *= ldexpf(1.f, -ka);
    }
    if (tid < 48) {
        lsc[tid] = (in_scale && tid < Cin) ? ldexpf(in_scale[tid], ka) : 0.f;
        lsh[tid] = (in_scale && tid < Cin) ? ldexpf(in_shift[tid], ka) : 0.f;
    }
    f32x4 acc[4][MT];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int tilesF = (F + 63) / 64, tilesT = (T + 1) / 2;
    const long ntiles = (long)B * tilesT * tilesF;
    const bool vec_ok = (F % 4 == 0) && ((((uintptr_t)x | (uintptr_t)dy) & 15) == 0);
    int pj_off[4], pj_df[4];                  // this wave's (tap, channel-tile) column tiles: LDS offset of the lane's channel row, column shift
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = min(wave + 8 * j, npair - 1), tap = p / nc16, c16 = p % nc16;
        pj_off[j] = (c16 * 16 + li) * W4_XCI + (tap / 3) * W4_XROW;
        pj_df[j] = tap % 3;
    }
    bool acc_neg = false;
    int round = 0;
    // register prefetch: the global loads of the NEXT tile are issued before the multiply of the current one and committed after it
    constexpr int DIT = (COUT * 32 + 511) / 512, XIT = 5;           // 16-byte loads per thread: dy (3 / 2), input (<= 40 ch x 4 rows x 16)
    f32x4 dreg[DIT], xreg[XIT];
    float hreg = 0.f;
    // one slice = one 16-byte load per thread (slices 0 .. DIT-1: dy, then XIT of the input; the halo columns ride on the last)
    auto issue_slice = [&](long tile, int slice) {
        long bid = tile;
        const int ft = (int)(bid % tilesF); bid /= tilesF;
        const int tt = (int)(bid % tilesT); const int b = (int)(bid / tilesT);
        const int t0 = tt * 2, f0 = ft * 64;
#pragma unroll
        for (int it = 0; it < DIT; ++it) {
            if (it != slice) continue;
            const int e = tid + 512 * it;
            const int co = e >> 5, r = (e >> 4) & 1, fq = e & 15;
            const int t = t0 + r, f = f0 + 4 * fq;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (e < COUT * 32 && t < T && f < F) {
                const float* src = dy + (((long)b * T + t) * COUT + co) * F + f;
                if (vec_ok && f + 3 < F) v = *reinterpret_cast<const f32x4*>(src);
                else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) if (f + q < F) v[q] = src[q];
                }
            }
            dreg[it] = v;
        }
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            if (DIT + it != slice) continue;
            const int e = tid + 512 * it;
            const int ci = e >> 6, row = (e >> 4) & 3, fq = e & 15;
            const int t = t0 + row - 1, f = f0 + 4 * fq;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (e < Cin * 64 && t >= 0 && t < T && f < F) {
                const float* src = x + (((long)b * T + t) * Cin + ci) * F + f;
                if (vec_ok && f + 3 < F) v = *reinterpret_cast<const f32x4*>(src);
                else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) if (f + q < F) v[q] = src[q];
                }
            }
            xreg[it] = v;
        }
        if (slice != DIT + XIT - 1) return;
        hreg = 0.f;
        if (tid < Cin * 8) {                 // halo columns f0 - 1 and f0 + 64
            const int ci = tid >> 3, row = (tid >> 1) & 3, side = tid & 1;
            const int t = t0 + row - 1, f = side ? f0 + 64 : f0 - 1;
            if (t >= 0 && t < T && f >= 0 && f < F) hreg = x[(((long)b * T + t) * Cin + ci) * F + f];
        }
    };
    auto commit = [&](long tile, unsigned sgn) {
        long bid = tile;
        const int ft = (int)(bid % tilesF); bid /= tilesF;
        const int tt = (int)(bid % tilesT);
        const int t0 = tt * 2, f0 = ft * 64;
#pragma unroll
        for (int it = 0; it < DIT; ++it) {
            const int e = tid + 512 * it;
            if (e >= COUT * 32) continue;
            const int co = e >> 5, r = (e >> 4) & 1, fq = e & 15;
            f32x4 v = dreg[it];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = __uint_as_float(__float_as_uint(v[q]) ^ sgn);
            uint2 o[TERMS];
            if (TERMS == 3) {
                split3_pair(v[0], v[1], o[0].x, o[1].x, o[TERMS - 1].x);
                split3_pair(v[2], v[3], o[0].y, o[1].y, o[TERMS - 1].y);
            } else {
                split2_pair_f16(v[0] * dscale, v[1] * dscale, o[0].x, o[1].x);
                split2_pair_f16(v[2] * dscale, v[3] * dscale, o[0].y, o[1].y);
            }
#pragma unroll
            for (int sp = 0; sp < TERMS; ++sp) *reinterpret_cast<uint2*>(ldy + sp * DPL + co * W4_DYCO + r * 128 + fq * 8) = o[sp];
        }
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            const int e = tid + 512 * it;
            if (e >= Cin * 64) continue;
            const int ci = e >> 6, row = (e >> 4) & 3, fq = e & 15;
            const int t = t0 + row - 1, f = f0 + 4 * fq;
            f32x4 v = xreg[it];
            if (in_scale && t >= 0 && t < T && f < F) {
                const float sc = lsc[ci], sh = lsh[ci];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = (f + q < F) ? fmaxf(v[q] * sc + sh, 0.f) : 0.f;
            }
            uint2 o[TERMS];
            if (TERMS == 3) {
                split3_pair(v[0], v[1], o[0].x, o[1].x, o[TERMS - 1].x);
                split3_pair(v[2], v[3], o[0].y, o[1].y, o[TERMS - 1].y);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = fminf(fmaxf(v[q], -65000.f), 65000.f);
                split2_pair_f16(v[0], v[1], o[0].x, o[1].x);
                split2_pair_f16(v[2], v[3], o[0].y, o[1].y);
            }
#pragma unroll
            for (int sp = 0; sp < TERMS; ++sp) *reinterpret_cast<uint2*>(lx + sp * XPL + ci * W4_XCI + row * W4_XROW + (8 + 4 * fq) * 2) = o[sp];
        }
        if (tid < Cin * 8) {
            const int ci = tid >> 3, row = (tid >> 1) & 3, side = tid & 1;
            const int t = t0 + row - 1, f = side ? f0 + 64 : f0 - 1;
            float v = hreg;
            if (in_scale && t >= 0 && t < T && f >= 0 && f < F) v = fmaxf(v * lsc[ci] + lsh[ci], 0.f);
            unsigned p0, p1, p2 = 0;
            if (TERMS == 3) split3_pair(v, 0.f, p0, p1, p2);
            else split2_pair_f16(fminf(fmaxf(v, -65000.f), 65000.f), 0.f, p0, p1);
            unsigned char* dst = lx + ci * W4_XCI + row * W4_XROW + (side ? 72 : 7) * 2;
            *reinterpret_cast<unsigned short*>(dst) = (unsigned short)p0;
            *reinterpret_cast<unsigned short*>(dst + XPL) = (unsigned short)p1;
            if (TERMS == 3) *reinterpret_cast<unsigned short*>(dst + (TERMS - 1) * XPL) = (unsigned short)p2;
        }
    };
    // XCD-aware walk: workgroup ids are dealt round-robin to the 8 XCDs (id % 8); every XCD walks its own contiguous eighth of the tile
    // space, its workgroups side by side on consecutive tiles -- the 8 column tiles of a row strip (the whole 1920-byte rows) and the
    // strips above / below (shared halo rows) then meet in ONE L2 instead of eight.
    long t_begin = blockIdx.x, t_end = ntiles, t_step = gridDim.x;
    if (gridDim.x % 8 == 0) {
        const long chunk = (ntiles + 7) / 8;
        t_begin = (blockIdx.x % 8) * chunk + blockIdx.x / 8;
        t_end = min(ntiles, (long)(blockIdx.x % 8 + 1) * chunk);
        t_step = gridDim.x / 8;
    }
#ifdef C4_TRACE
    const int trace_wg = (blockIdx.x >= 64 && blockIdx.x < 64 + C4_TRACE_WGS) ? (int)blockIdx.x - 64 : -1;
#define W4_STAMP(k) do { if (trace_wg >= 0 && round >= 100 && round < 100 + C4_TRACE_STAGES && tid == 0) w4_trace[(trace_wg * C4_TRACE_STAGES + round - 100) * 8 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define W4_STAMP(k) do {} while (0)
#endif
    auto issue = [&](long tile) {
#pragma unroll
        for (int sl = 0; sl < DIT + XIT; ++sl) issue_slice(tile, sl);
    };
    if (t_begin < t_end) issue(t_begin);
    for (long tile = t_begin; tile < t_end; tile += t_step, ++round) {
        const bool neg = round & 1;
        W4_STAMP(0);
        __syncthreads();                     // previous tile consumed (first round: the zero fill is complete)
        W4_STAMP(1);
        commit(tile, neg ? 0x80000000u : 0u);
        W4_STAMP(2);
        __syncthreads();
        W4_STAMP(3);
        // in flight during the multiply below.  (Issuing them slice by slice BETWEEN the MFMAs of the multiply instead of as one burst was
        // measured: the burst's 2.3 k clocks of back-pressure disappear, but the multiply grows from 8.1 k to 12.8 k clocks per tile -- a
        // wave stalled on a full memory queue issues no MFMAs either.)
        if (tile + t_step < t_end) issue(tile + t_step);
        W4_STAMP(4);
        if (neg != acc_neg) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[j][i][r] = -acc[j][i][r];
            acc_neg = neg;
        }
        // A lane group owns 16 consecutive positions of a row: two k-steps (positions 16 lk + 8 h + [0, 8), h = 0 / 1 -- any k order is
        // fine as long as dy and the input agree) share ONE set of loads, so the two conflict-prone 4-byte neighbour reads are paid
        // once per 16 positions.
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            u32x4 a[2][TERMS][MT];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int sp = 0; sp < TERMS; ++sp)
#pragma unroll
                    for (int i = 0; i < MT; ++i)
                        a[h][sp][i] = *reinterpret_cast<const u32x4*>(ldy + sp * DPL + (i * 16 + li) * W4_DYCO + r * 128 + (lk * 16 + h * 8) * 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (wave + 8 * j >= npair) continue;            // uniform per wave
                const int df = pj_df[j];
                const unsigned char* base = lx + pj_off[j] + r * W4_XROW + (lk * 16 + 8) * 2;
                u32x4 bfrag[2][TERMS];
#pragma unroll
                for (int sp = 0; sp < TERMS; ++sp) {
                    const u32x4 d0 = *reinterpret_cast<const u32x4*>(base + sp * XPL);
                    const u32x4 d1 = *reinterpret_cast<const u32x4*>(base + sp * XPL + 16);
                    u32x4 w0 = d0, w1 = d1;                      // df == 1: the aligned windows
                    if (df == 0) {
                        const unsigned dm1 = *reinterpret_cast<const unsigned*>(base + sp * XPL - 4);
                        w0[0] = __builtin_amdgcn_alignbit(d0[0], dm1, 16); w0[1] = __builtin_amdgcn_alignbit(d0[1], d0[0], 16);
                        w0[2] = __builtin_amdgcn_alignbit(d0[2], d0[1], 16); w0[3] = __builtin_amdgcn_alignbit(d0[3], d0[2], 16);
                        w1[0] = __builtin_amdgcn_alignbit(d1[0], d0[3], 16); w1[1] = __builtin_amdgcn_alignbit(d1[1], d1[0], 16);
                        w1[2] = __builtin_amdgcn_alignbit(d1[2], d1[1], 16); w1[3] = __builtin_amdgcn_alignbit(d1[3], d1[2], 16);
                    } else if (df == 2) {
                        const unsigned d8 = *reinterpret_cast<const unsigned*>(base + sp * XPL + 32);
                        w0[0] = __builtin_amdgcn_alignbit(d0[1], d0[0], 16); w0[1] = __builtin_amdgcn_alignbit(d0[2], d0[1], 16);
                        w0[2] = __builtin_amdgcn_alignbit(d0[3], d0[2], 16); w0[3] = __builtin_amdgcn_alignbit(d1[0], d0[3], 16);
                        w1[0] = __builtin_amdgcn_alignbit(d1[1], d1[0], 16); w1[1] = __builtin_amdgcn_alignbit(d1[2], d1[1], 16);
                        w1[2] = __builtin_amdgcn_alignbit(d1[3], d1[2], 16); w1[3] = __builtin_amdgcn_alignbit(d8, d1[3], 16);
                    }
                    bfrag[0][sp] = w0;
                    bfrag[1][sp] = w1;
                }
#define W4_PRODUCT(SA, SB)                                                                                                   \
                _Pragma("unroll") for (int h = 0; h < 2; ++h)                                                                \
                    _Pragma("unroll") for (int i = 0; i < MT; ++i)                                                           \
                        acc[j][i] = (TERMS == 3) ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[h][SA][i]), __builtin_bit_cast(bf16x8, bfrag[h][SB]), acc[j][i], 0, 0, 0) \
                                                 : __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a[h][SA][i]), __builtin_bit_cast(f16x8, bfrag[h][SB]), acc[j][i], 0, 0, 0);
                if (TERMS == 3) { W4_PRODUCT(TERMS - 1, 0) W4_PRODUCT(1, 1) W4_PRODUCT(0, TERMS - 1) }
                W4_PRODUCT(1, 0) W4_PRODUCT(0, 1) W4_PRODUCT(0, 0)
#undef W4_PRODUCT
            }
        }
        W4_STAMP(5);
    }
    // slab [Cout][Cin][9]; C/D map: lane holds column n = li (input channel of the tile), rows 4 lk + r (output channel)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = wave + 8 * j;
        if (p >= npair) continue;
        const int tap = p / nc16, c16 = p % nc16, ci = c16 * 16 + li;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = i * 16 + lk * 4 + r;
                if (co < COUT && ci < Cin) partial[(((long)blockIdx.x * COUT + co) * Cin + ci) * 9 + tap] = (acc_neg ? -acc[j][i][r] : acc[j][i][r]) * unscale;
            }
    }
}

size_t a2s_conv3x3_wgrad_workspace_bytes_impl(int Cin, int Cout) {
    const int chunks = (Cin + CV_CK - 1) / CV_CK;
    return (size_t)chunks * 1024 * Cout * CV_CK * 9 * sizeof(float);
}

int a2s_conv3x3_wgrad_impl(hipStream_t st, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dW,
                           float* ws, size_t ws_bytes, int B, int T, int F, int Cin, int Cout, const float* bn_y, const float* bn_mean,
                           const float* bn_invstd, const float* bn_scale, const float* bn_shift, const float* bn_c12, float* dy_out,
                           const float* dy_absmax, const float* act_absmax) {
    A2S_REQUIRE(dy && x && dW && ws, "conv3x3_wgrad: null tensor");
    A2S_REQUIRE(!bn_y || (bn_mean && bn_invstd && bn_scale && bn_shift && bn_c12), "conv3x3_wgrad: the fused BatchNorm backward needs all of its tensors");
    A2S_REQUIRE(!dy_out || bn_y, "conv3x3_wgrad: dy_out is only written by the fused BatchNorm backward");
    const BnBwdFuse bn{bn_y, bn_mean, bn_invstd, bn_scale, bn_shift, bn_c12, dy_out};
    A2S_REQUIRE(ws_bytes >= a2s_conv3x3_wgrad_workspace_bytes_impl(Cin, Cout), "conv3x3_wgrad: workspace too small");
    if (Cin == 1 && !in_scale && Cout * C1W_PARTS <= 256 && (size_t)Cout * F >= 256 * 9) {
        const size_t shm = ((size_t)Cout * F + 3 * (F + 8)) * sizeof(float);
        if (shm <= 64 * 1024) {
            const bool stream = a2s_sw(A2S_SW_conv_c1_fast) && bn_y && Cout == 20 && F == 480 && (((uintptr_t)dy | (uintptr_t)bn_y | (uintptr_t)dy_out | (uintptr_t)x) & 15) == 0;
            if (stream) hipLaunchKernelGGL((conv3x3_wgrad_c1_stream<20, 480>), dim3(WGRAD_SLABS), dim3(256), shm, st, dy, x, ws, B, T, bn);
            else hipLaunchKernelGGL(conv3x3_wgrad_c1, dim3(WGRAD_SLABS), dim3(256), shm, st, dy, x, ws, B, T, F, Cout, bn);
            A2S_CHECK_LAUNCH("conv3x3_wgrad_c1");
            hipLaunchKernelGGL(wgrad_reduce_c1, dim3(a2s_cdiv(Cout * 9, 256)), dim3(256), 0, st, ws, dW, WGRAD_SLABS, Cout * 9);
            A2S_CHECK_LAUNCH("wgrad_reduce_c1");
            return A2S_OK;
        }
    }
    const bool two = a2s_sw(A2S_SW_wgrad_f16x2) && dy_absmax;          // two fp16 terms: with the operand's max |dy| only
    // round 3: the row-streaming kernel (a2s_conv_wrows.hip) wherever its operand ranges are known
    if (two && !bn_y && a2s_wgrad_rows_eligible(F, Cin, Cout) && (!in_scale || act_absmax))
        return a2s_conv3x3_wgrad_rows_impl(st, dy, x, in_scale, in_shift, dW, ws, ws_bytes, B, T, F, Cin, Cout, dy_absmax, act_absmax);
    // measured at B = 64 (tools/conv_f16x2_check.py; fp32-input kernel / three bf16 terms / two fp16 terms): 40 -> 40: 12.3 / 9.9 / 7.1 ms,
    // 20 -> 40: 6.3 / 7.4 / 5.3 ms, 20 -> 20: 4.6 / 6.2 / 4.6 ms -- the three-term kernel only pays off at 40 -> 40 channels, the two-term
    // one for 40 output channels (wgrad_bf16x3 = 2 / wgrad_f16x2 = 2: every eligible launch regardless)
    const bool split_here = a2s_sw(A2S_SW_wgrad_bf16x3) > 1 || (Cin == 40 && Cout == 40) || (two && (Cout == 40 || a2s_sw(A2S_SW_wgrad_f16x2) > 1));
    if (a2s_sw(A2S_SW_wgrad_bf16x3) && !bn_y && Cin > 1 && Cin <= 40 && (Cout == 20 || Cout == 40) && split_here) {
        const int nslabs = 256;               // one 512-thread workgroup per CU
        A2S_REQUIRE(ws_bytes >= (size_t)nslabs * Cout * Cin * 9 * sizeof(float), "conv3x3_wgrad: workspace too small for the split-operand kernel");
        if (two && Cout == 20) hipLaunchKernelGGL((conv3x3_wgrad_split<20, 2>), dim3(nslabs), dim3(512), 0, st, dy, x, in_scale, in_shift, ws, B, T, F, Cin, dy_absmax, act_absmax);
        else if (two) hipLaunchKernelGGL((conv3x3_wgrad_split<40, 2>), dim3(nslabs), dim3(512), 0, st, dy, x, in_scale, in_shift, ws, B, T, F, Cin, dy_absmax, act_absmax);
        else if (Cout == 20) hipLaunchKernelGGL((conv3x3_wgrad_split<20, 3>), dim3(nslabs), dim3(512), 0, st, dy, x, in_scale, in_shift, ws, B, T, F, Cin, (const float*)nullptr, (const float*)nullptr);
        else hipLaunchKernelGGL((conv3x3_wgrad_split<40, 3>), dim3(nslabs), dim3(512), 0, st, dy, x, in_scale, in_shift, ws, B, T, F, Cin, (const float*)nullptr, (const float*)nullptr);
        A2S_CHECK_LAUNCH("conv3x3_wgrad_split");
        hipLaunchKernelGGL(wgrad_reduce_c1, dim3(a2s_cdiv(Cout * Cin * 9, 256)), dim3(256), 0, st, ws, dW, nslabs, Cout * Cin * 9);
        A2S_CHECK_LAUNCH("wgrad_reduce_c1");
        return A2S_OK;
    }
    const int chunks = (Cin + CV_CK - 1) / CV_CK;
    // persistent workgroups: one full round of the occupancy the kernel reaches (__launch_bounds__(256, 3): 3 per CU for Cout 40,
    // 4 per CU for Cout 20 -- without the bound the compiler spent 200 registers and dropped Cout 40 to 2 per CU)
    const int slabs = Cout == 20 ? 1024 : WGRAD_SLABS;
    dim3 grid(slabs, chunks);
    if (Cout == 20 && !bn_y) hipLaunchKernelGGL((conv3x3_wgrad<20, false>), grid, dim3(256), 0, st, dy, x, in_scale, in_shift, ws, B, T, F, Cin, bn);
    else if (Cout == 20) hipLaunchKernelGGL((conv3x3_wgrad<20, true>), grid, dim3(256), 0, st, dy, x, in_scale, in_shift, ws, B, T, F, Cin, bn);
    else if (Cout == 40 && !bn_y) hipLaunchKernelGGL((conv3x3_wgrad<40, false>), grid, dim3(256), 0, st, dy, x, in_scale, in_shift, ws, B, T, F, Cin, bn);
    else if (Cout == 40) hipLaunchKernelGGL((conv3x3_wgrad<40, true>), grid, dim3(256), 0, st, dy, x, in_scale, in_shift, ws, B, T, F, Cin, bn);
    else A2S_FAIL(A2S_ERR_ARG, "conv3x3_wgrad: Cout must be 20 or 40 (got %d)", Cout);
    A2S_CHECK_LAUNCH("conv3x3_wgrad");
    const int n = Cout * CV_CK * 9 * chunks;
    hipLaunchKernelGGL(wgrad_reduce, dim3(a2s_cdiv(n, 256)), dim3(256), 0, st, ws, dW, slabs, Cout, Cin, chunks);
    A2S_CHECK_LAUNCH("wgrad_reduce");
    return A2S_OK;
}
