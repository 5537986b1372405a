// ConvStack kernels (reference models.py:463-543): 3x3 convolutions (stride 1,
// zero pad 1, no bias) with BatchNorm (batch statistics) + ReLU, on activations laid out (B, T, C, F) fp32.
//
// Layout: the reference keeps NCHW = (B, C, T, F) and then does transpose(1,2).flatten(2) to get
// (B, T, C*F) rows for the 19200->256 Linear (models.py:537).  Here every activation lives as (B, T, C, F)
// from the start: the network input (B,1,T,F) is already that layout, each (b,t) row holds C planes of F
// contiguous floats (coalesced along F), and the last layer's output IS the (B*T, C*F) GEMM operand with the
// reference's column order c*F+f -- the 92 MB/clip transpose copy never exists.
//
// conv3x3_mfma: implicit GEMM on v_mfma_f32_16x16x4_f32.  M = 16 consecutive f positions, N = 16 output
//   channels, K = (dt, df, ci) with ci fastest (4 consecutive input channels per MFMA).  A workgroup owns
//   TR=4 rows x FT=32 columns x all Cout; input channels are streamed through LDS in chunks of 20 together
//   with their weight slice, so LDS stays at ~46 KB and 3 workgroups share a CU (one stages while others
//   multiply).  The previous layer's BatchNorm+ReLU is applied while staging (y = max(0, x*scale+shift)),
//   so post-activation tensors are never written; the epilogue emits per-workgroup per-channel sum / sum of
//   squares for THIS layer's batch statistics (reduced in a fixed order by bn_finalize -> deterministic).
// conv3x3_c1: the first layer (Cin = 1, K = 9) as a direct VALU kernel (0.7 % of the stack's flops).
//
// This file: the tiled forward and data-gradient kernels.  BatchNorm (statistics, apply, backward) is a2s_bn.hip, the tiled weight
// gradient a2s_conv_wgrad.hip; the row-streaming kernels the model's shapes run on are a2s_conv_rows.hip / a2s_conv_wrows.hip.
#include "a2s_internal.h"

#define CV_RS 36                 // LDS row stride (FT + 2 halo, padded)
#define CV_PLANE 240             // LDS plane stride: (TR+2)*RS = 216 -> 240 (== 16 mod 32: conflict-free k pairs)
#define CV_WS 48                 // weight row stride in LDS (3 n-tiles of 16)

struct ConvArgs {
    const float* x;      // (B, T, Cin, F)   pre-activation of the previous layer (or the spectrogram)
    const float* w;      // (Cout, Cin, 3, 3) reference layout
    float* y;            // (B, T, Cout, F)  pre-BN conv output
    const float* in_scale; const float* in_shift;   // per input channel; null -> identity, no ReLU
    float* stat_partial; // [nblocks][Cout][2] sum, sumsq over the block's valid positions (null -> skip)
    int B, T, F, Cin, Cout;
    int flip;            // 1: use w as a transposed/flipped kernel (dgrad): w'[ci][co][2-dt][2-df]
    // data-gradient launches only (template BNRED): the output g is the gradient wrt relu(bn(yl)) of the layer below; its BatchNorm
    // backward statistics  sum g', sum g' xhat  (g' = g where bn(yl) > 0) are accumulated in the epilogue and written to stat_partial
    // in the layout bn_bwd_finalize reads -- the separate statistics pass over (g, yl) disappears
    const float* yl; const float* yl_mean; const float* yl_invstd; const float* yl_scale; const float* yl_shift;
    // two-term fp16 split (conv3x3_split<.., 2>) only: device scalars holding max|x| (null: the operand is used unscaled) and max|w|
    const float* x_absmax; const float* w_absmax;
    float* out_absmax;   // [Cout] max |y| per output channel (atomic max of non-negative floats; zeroed by the launcher), or null
};

// ---- v2 geometry (round 1, after profiling: the first version spent more time staging than multiplying -- scalar loads with
// div/mod per element and a 34 KB weight slice re-derived from the (Cout,Cin,3,3) layout per 128 outputs).
//   * tile = 4 rows x 64 columns (4 m-tiles per wave): the weight slice is amortised over twice the outputs;
//   * weights are pre-packed ONCE per call into the LDS image [chunk][9*CK][48] (conv_pack_weights) -> straight 16-byte copies;
//   * the input tile is staged with 16-byte loads (interior) + 2 halo scalars per row; interior starts at column 4 of a 72-float
//     LDS row so the vector stores are aligned; plane stride 6*72 = 432 == 16 (mod 32) keeps the k-pair fragment reads conflict-free.
#define C2_FT 64
#define C2_RS 72
#define C2_PLANE (6 * C2_RS)
#define C2_WCHUNK (9 * CV_CK * CV_WS)      // floats per packed weight chunk

__global__ void conv_pack_weights(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int flip, int chunks) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= chunks * C2_WCHUNK) return;
    const int chunk = e / C2_WCHUNK, rem = e % C2_WCHUNK;
    const int n = rem % CV_WS, k = rem / CV_WS;
    const int c = k % CV_CK, tap = k / CV_CK;
    const int ci = chunk * CV_CK + c;
    float v = 0.f;
    if (n < Cout && ci < Cin) v = flip ? w[((long)ci * Cout + n) * 9 + (8 - tap)] : w[((long)n * Cin + ci) * 9 + tap];
    wp[e] = v;
}

// ---- v3 (round 1, after measuring that a workgroup spent ~2/3 of a chunk's wall time staging: every one of its ~17 global loads per
// thread was followed by its own LDS store, i.e. 17 serialised L2 round trips per chunk):
//   * a workgroup walks C3_TPW consecutive row tiles; the (tile, chunk) pairs form one pipeline of stages;
//   * the global loads of stage q+1 (input tile, weight slice if it changes) are issued into registers BEFORE the multiply of stage q
//     and committed to LDS after it -- one round trip per stage, hidden behind ~540 MFMAs per wave;
//   * with one input chunk (Cin = 20) the packed weights are staged once per workgroup; with two, consecutive tiles visit the chunks
//     in serpentine order (0,1 | 1,0 | 0,1 ...) so the weight slice changes every other stage only;
//   * batch-statistics partials are accumulated over the workgroup's tiles and written once.
#define C3_TPW 8
#define C3_WIT ((C2_WCHUNK / 4 + 255) / 256)                                  // float4 weight loads per thread and stage (9)
#define C3_XIT ((CV_CK * (CV_TR + 2) * (C2_FT / 4) + 255) / 256)              // float4 input loads per thread and stage (8)

template <int COUT, bool BNRED>
__global__ __launch_bounds__(256, 2) void conv3x3_mfma(ConvArgs a, const float* __restrict__ wpack) {
    constexpr int NT = (COUT + 15) / 16;               // n-tiles: 2 (Cout 20) or 3 (Cout 40)
    __shared__ __attribute__((aligned(16))) float lin[CV_CK * C2_PLANE];       // 34560 B
    __shared__ __attribute__((aligned(16))) float lw[C2_WCHUNK];               // 34560 B
    __shared__ float red[4][NT * 16][2];

    const int tilesF = (a.F + C2_FT - 1) / C2_FT;
    const int tilesT = (a.T + CV_TR - 1) / CV_TR;
    const int groupsT = (tilesT + C3_TPW - 1) / C3_TPW;
    int bid = blockIdx.x;
    const int ft = bid % tilesF; bid /= tilesF;
    const int tg = bid % groupsT; const int b = bid / groupsT;
    const int f0 = ft * C2_FT;
    const int tile0 = tg * C3_TPW, ntile = min(C3_TPW, tilesT - tile0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const bool vec_ok = (a.F % 4 == 0) && (((uintptr_t)a.x & 15) == 0);
    const int nchunks = a.Cin / CV_CK;
    const int nstage = ntile * nchunks;

    f32x4 acc[4][NT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float st_s[NT], st_s2[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) { st_s[j] = 0.f; st_s2[j] = 0.f; }

    // stage q -> (tile, chunk): serpentine over the chunks so that consecutive stages share the weight slice where possible
    auto stage_tile = [&](int q) { return q / nchunks; };
    auto stage_chunk = [&](int q) { const int i = q / nchunks, c = q % nchunks; return (i & 1) ? nchunks - 1 - c : c; };

    f32x4 wreg[C3_WIT], xreg[C3_XIT];
    float hreg = 0.f;
    bool wreg_valid = false;
    auto issue = [&](int q, int resident_chunk) {
        const int ch = stage_chunk(q), t0 = (tile0 + stage_tile(q)) * CV_TR, c0 = ch * CV_CK;
        wreg_valid = ch != resident_chunk;
        if (wreg_valid) {
            const f32x4* wsrc4 = reinterpret_cast<const f32x4*>(wpack + (long)ch * C2_WCHUNK);
#pragma unroll
            for (int it = 0; it < C3_WIT; ++it) {
                const int e = tid + 256 * it;
                wreg[it] = e < C2_WCHUNK / 4 ? wsrc4[e] : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int it = 0; it < C3_XIT; ++it) {
            const int e = tid + 256 * it;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (e < CV_CK * (CV_TR + 2) * (C2_FT / 4)) {
                const int j = e % (C2_FT / 4), row = e / (C2_FT / 4);
                const int r = row % (CV_TR + 2), c = row / (CV_TR + 2);
                const int t = t0 + r - 1, f = f0 + 4 * j, ci = c0 + c;
                if (t >= 0 && t < a.T && f < a.F) {
                    const float* src = a.x + (((long)b * a.T + t) * a.Cin + ci) * a.F + f;
                    if (vec_ok && f + 3 < a.F) v = *reinterpret_cast<const f32x4*>(src);
                    else {
#pragma unroll
                        for (int qq = 0; qq < 4; ++qq) if (f + qq < a.F) v[qq] = src[qq];
                    }
                }
            }
            xreg[it] = v;
        }
        if (tid < CV_CK * (CV_TR + 2) * 2) {           // halo columns f0-1 and f0+64
            const int side = tid & 1, row = tid >> 1;
            const int r = row % (CV_TR + 2), c = row / (CV_TR + 2);
            const int t = t0 + r - 1, f = side ? f0 + C2_FT : f0 - 1, ci = c0 + c;
            hreg = (t >= 0 && t < a.T && f >= 0 && f < a.F) ? a.x[(((long)b * a.T + t) * a.Cin + ci) * a.F + f] : 0.f;
        }
    };
    auto commit = [&](int q) {     // registers -> LDS; BN+ReLU of the producer folded in; zero = padding (of the ACTIVATED tensor)
        const int ch = stage_chunk(q), t0 = (tile0 + stage_tile(q)) * CV_TR, c0 = ch * CV_CK;
        if (wreg_valid) {
#pragma unroll
            for (int it = 0; it < C3_WIT; ++it) {
                const int e = tid + 256 * it;
                if (e < C2_WCHUNK / 4) reinterpret_cast<f32x4*>(lw)[e] = wreg[it];
            }
        }
#pragma unroll
        for (int it = 0; it < C3_XIT; ++it) {
            const int e = tid + 256 * it;
            if (e < CV_CK * (CV_TR + 2) * (C2_FT / 4)) {
                const int j = e % (C2_FT / 4), row = e / (C2_FT / 4);
                const int r = row % (CV_TR + 2), c = row / (CV_TR + 2);
                const int t = t0 + r - 1, f = f0 + 4 * j, ci = c0 + c;
                f32x4 v = xreg[it];
                if (a.in_scale && t >= 0 && t < a.T && f < a.F) {
                    const float sc = a.in_scale[ci], sh = a.in_shift[ci];
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) v[qq] = (f + qq < a.F) ? fmaxf(v[qq] * sc + sh, 0.f) : 0.f;
                }
                *reinterpret_cast<f32x4*>(lin + c * C2_PLANE + r * C2_RS + 4 + 4 * j) = v;
            }
        }
        if (tid < CV_CK * (CV_TR + 2) * 2) {
            const int side = tid & 1, row = tid >> 1;
            const int r = row % (CV_TR + 2), c = row / (CV_TR + 2);
            const int t = t0 + r - 1, f = side ? f0 + C2_FT : f0 - 1, ci = c0 + c;
            float v = hreg;
            if (a.in_scale && t >= 0 && t < a.T && f >= 0 && f < a.F) v = fmaxf(v * a.in_scale[ci] + a.in_shift[ci], 0.f);
            lin[c * C2_PLANE + r * C2_RS + (side ? 4 + C2_FT : 3)] = v;
        }
    };

    int resident = -1;
    issue(0, resident);
    for (int q = 0; q < nstage; ++q) {
        __syncthreads();                      // previous stage fully consumed
        commit(q);
        resident = stage_chunk(q);
        __syncthreads();
        if (q + 1 < nstage) issue(q + 1, resident);      // in flight during the multiply below
        // ---- multiply: 9 taps x CK/4 k-steps, 4 m-tiles x NT n-tiles per wave
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dt = tap / 3, df = tap % 3;
#pragma unroll
            for (int cs = 0; cs < CV_CK / 4; ++cs) {
                const int c = cs * 4 + lk;
                const float* src = lin + c * C2_PLANE + (wave + dt) * C2_RS + 3 + df + li;
                float av[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) av[i] = src[i * 16];
                const float* wsrc = lw + (tap * CV_CK + c) * CV_WS + li;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const float bv = wsrc[j * 16];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv, acc[i][j], 0, 0, 0);
                }
            }
        }
        if ((q + 1) % nchunks != 0) continue;
        // ---- tile epilogue.  C/D map: lane holds column n = li (channel), rows lk*4+r (f positions) of each m-tile.
        const int t = (tile0 + stage_tile(q)) * CV_TR + wave;
        const bool row_ok = t < a.T;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int co = j * 16 + li;
            float bm = 0.f, bi = 0.f, bsc = 0.f, bsh = 0.f;
            f32x4 yv[4];
            if (BNRED && row_ok && co < COUT) {          // layer-below BatchNorm constants of this lane's channel + its yl values
                bm = a.yl_mean[co]; bi = a.yl_invstd[co]; bsc = a.yl_scale[co]; bsh = a.yl_shift[co];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int f = f0 + i * 16 + lk * 4;
                    const float* src = a.yl + (((long)b * a.T + t) * COUT + co) * a.F + f;
                    if (f + 3 < a.F && (a.F % 4 == 0)) yv[i] = *reinterpret_cast<const f32x4*>(src);
                    else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) yv[i][r] = (f + r < a.F) ? src[r] : 0.f;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = f0 + i * 16 + lk * 4;
                if (row_ok && co < COUT) {
                    float* dst = a.y + (((long)b * a.T + t) * COUT + co) * a.F + f;
                    const bool full = f + 3 < a.F && (a.F % 4 == 0);
                    if (full) *reinterpret_cast<f32x4*>(dst) = acc[i][j];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (!full && f + r >= a.F) continue;
                        const float v = acc[i][j][r];
                        if (!full) dst[r] = v;
                        if (BNRED) {
                            const float xv = yv[i][r];
                            const float gm = (xv * bsc + bsh > 0.f) ? v : 0.f;
                            st_s[j] += gm; st_s2[j] += gm * (xv - bm) * bi;
                        } else { st_s[j] += v; st_s2[j] += v * v; }
                    }
                }
                acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    if (a.stat_partial) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            float s = st_s[j], s2 = st_s2[j];
            s += __shfl_xor(s, 16, 64); s2 += __shfl_xor(s2, 16, 64);
            s += __shfl_xor(s, 32, 64); s2 += __shfl_xor(s2, 32, 64);
            if (lk == 0) { red[wave][j * 16 + li][0] = s; red[wave][j * 16 + li][1] = s2; }
        }
        __syncthreads();
        if (tid < COUT) {
            float s = 0.f, s2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { s += red[w][tid][0]; s2 += red[w][tid][1]; }
            a.stat_partial[((long)blockIdx.x * COUT + tid) * 2 + 0] = s;
            a.stat_partial[((long)blockIdx.x * COUT + tid) * 2 + 1] = s2;
        }
    }
}

// ---- v4: the same fp32 convolution on the bf16 matrix pipes (16x the fp32-input MFMA rate).  Every fp32 operand is split
// EXACTLY into three bf16 terms x = x0 + x1 + x2 (8 significand bits each, by truncation; the residuals are exact in fp32), and a
// product is formed from the six term products of order >= 2^-16:  a0b0 + (a0b1 + a1b0) + (a0b2 + a1b1 + a2b0), each exact in the
// fp32 accumulator (8 x 8 bits); the dropped terms are <= 3 * 2^-24 |a||b| -- the size of one fp32 rounding.  Same tile / pipeline
// as v3; what changes:
//   * K = (tap, 8-channel group): v_mfma_f32_16x16x32_bf16 takes 8 consecutive k per lane = the 8 channels of a group at one tap,
//     the four 16-lane groups of a k-step take four consecutive (tap, group) pairs of the chunk (pair p = tap * ncg + group);
//   * input chunk = 2 channel groups (16 channels; the last chunk of Cin = 20 / 40 has one), staged position-major:
//     lin[term][row 6][position 66][16 ch] bf16, so a lane's A fragment is ONE ds_read_b128 (32-byte position stride: conflict-free
//     within the hardware's 16-lane read groups);  a thread stages (row, position, group) items: 8 scalar loads (coalesced along
//     f, halo columns included -- no separate halo path), BatchNorm+ReLU, split, three 16-byte LDS stores;
//   * weights are pre-split and pre-packed per chunk as [term][pair slot 20][n COUT][8 ch] bf16 (conv_pack_weights_bf16x3).
#define C4_POS 66
#define C4_PSTR 32                              // bytes per position (2 groups x 8 bf16)
#define C4_ROWB (C4_POS * C4_PSTR)              // 2112
#define C4_INPL ((CV_TR + 2) * C4_ROWB)         // bytes per term plane of the input tile (12672)
#define C4_SLOTS 20                             // pair slots per chunk (5 k-steps x 4)
#define C4_XIT 4                                // staging items per thread and stage (792 items / 256)
#define C4_ITEMS ((CV_TR + 2) * C4_POS)         // items per channel group (396)

__host__ __device__ inline int c4_chunks(int Cin) { return ((Cin + 7) / 8 + 1) / 2; }
// Weight slots of a term plane: the even slots first, the odd ones from a 256-byte aligned base -- the two slots a hardware
// ds_read_b128 lane group touches (pairs p, p+1) then start on the same bank and their 8 + 8 lanes interleave without conflicts.
__host__ __device__ constexpr int c4_odd_base(int Cout) { return (C4_SLOTS / 2 * Cout * 16 + 255) / 256 * 256; }
__host__ __device__ constexpr int c4_wpl(int Cout) { return c4_odd_base(Cout) + C4_SLOTS / 2 * Cout * 16; }
__host__ __device__ inline size_t c4_chunk_bytes(int Cout, int terms = 3) { return ((size_t)terms * c4_wpl(Cout) + 4095) / 4096 * 4096; }   // whole LDS-DMA rounds

template <int TERMS>
__global__ void conv_pack_weights_split(const float* __restrict__ w, unsigned short* __restrict__ wp, int Cin, int Cout, int flip,
                                        const float* __restrict__ w_absmax) {
    const int ncgs = (Cin + 7) / 8, nchunks = (ncgs + 1) / 2;
    const int per_term = C4_SLOTS * Cout * 8;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nchunks * per_term) return;
    const int chunk = e / per_term, rem = e % per_term;
    const int k8 = rem % 8, n = (rem / 8) % Cout, p = rem / (8 * Cout);
    const int ncg = min(2, ncgs - 2 * chunk);
    float v = 0.f;
    if (p < 9 * ncg) {
        const int tap = p / ncg, ci = (chunk * 2 + p % ncg) * 8 + k8;
        if (ci < Cin) v = flip ? w[((long)ci * Cout + n) * 9 + (8 - tap)] : w[((long)n * Cin + ci) * 9 + tap];
    }
    const int wpl = c4_wpl(Cout) / 2;                 // in 16-bit elements
    unsigned short* dst = wp + (long)chunk * (c4_chunk_bytes(Cout, TERMS) / 2) + (p & 1) * (c4_odd_base(Cout) / 2) + ((p >> 1) * Cout + n) * 8 + k8;
    if (TERMS == 3) {
        unsigned t0, t1, t2;
        split3_pair(v, 0.f, t0, t1, t2);
        dst[0] = (unsigned short)t0; dst[wpl] = (unsigned short)t1; dst[2 * wpl] = (unsigned short)t2;      // pads are zeroed by the launcher
    } else {
        unsigned t0, t1;
        split2_pair_f16(ldexpf(v, pow2_scale_exp(*w_absmax, 13)), 0.f, t0, t1);
        dst[0] = (unsigned short)t0; dst[wpl] = (unsigned short)t1;
    }
}

#define C4_MH 2          // m-tiles per pass of a k-step (2: half the A-fragment registers, B fragments read twice)
// two-term fp16 variant of c4_multiply: three products per k-step, smallest first.
//   * product-major order: each product runs over ALL MT x NT accumulators before the next product touches them again (an MFMA that
//     accumulates into the register its predecessor-but-one wrote would stall on the 8-pass latency of v_mfma_f32_16x16x32);
//   * the fragment reads are software-pipelined: the 2 (MT + NT) ds_read_b128 of k-step s+1 are issued BETWEEN the MFMAs of k-step s
//     (sched_group_barrier: one read, then three MFMAs, ...), into a second register set.  hipcc's own schedule issued every read right
//     before its first use (s_waitcnt lgkmcnt straight after the read, three to five times per k-step): with two waves per SIMD the
//     ~130-cycle LDS latency was exposed each time -- the multiply phase alone ran at 35 % matrix-pipe utilisation.
// MT = m-tiles computed (2: the last column tile of F = 480 holds 32 valid columns).
template <int MT, int NT>
struct C2Frag { f16x8 a[2][MT], b[2][NT]; };
template <int MT, int NT, int COUT>
__device__ __forceinline__ void c2_load(C2Frag<MT, NT>& f, const unsigned char* __restrict__ lin, const unsigned char* __restrict__ lw, int aoff, int boff, int s) {
    constexpr int WPL = c4_wpl(COUT);
#pragma unroll
    for (int sp = 0; sp < 2; ++sp)
#pragma unroll
        for (int i = 0; i < MT; ++i) f.a[sp][i] = *reinterpret_cast<const f16x8*>(lin + sp * C4_INPL + aoff + i * 16 * C4_PSTR);
#pragma unroll
    for (int sp = 0; sp < 2; ++sp)
#pragma unroll
        for (int j = 0; j < NT; ++j) f.b[sp][j] = *reinterpret_cast<const f16x8*>(lw + sp * WPL + boff + s * 2 * COUT * 16 + j * 256);
}
template <int MT, int NT, bool PIN>
__device__ __forceinline__ void c2_products(const C2Frag<MT, NT>& f, f32x4 (&acc)[4][NT]) {
#define C4_PRODUCT(SA, SB)                                                                                                   \
    _Pragma("unroll") for (int j = 0; j < NT; ++j)                                                                           \
        _Pragma("unroll") for (int i = 0; i < MT; ++i)                                                                       \
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.a[SA][i], f.b[SB][j], acc[i][j], 0, 0, 0);
    // PIN (the last k-step, nothing to interleave): keep the three products apart -- left alone, hipcc groups the three MFMAs of each
    // accumulator back to back (a dependent chain: three times the 8-pass latency per accumulator)
    C4_PRODUCT(1, 0)
    if (PIN) __builtin_amdgcn_sched_barrier(0);
    C4_PRODUCT(0, 1)
    if (PIN) __builtin_amdgcn_sched_barrier(0);
    C4_PRODUCT(0, 0)
    if (PIN) __builtin_amdgcn_sched_barrier(0);
#undef C4_PRODUCT
}
template <int KS, int MT, int NT, int COUT>
__device__ __forceinline__ void c4_multiply_f16x2(const unsigned char* __restrict__ lin, const unsigned char* __restrict__ lw,
                                                  const int (&aoff)[KS], int boff, f32x4 (&acc)[4][NT]) {
    constexpr int NREAD = 2 * (MT + NT), NMFMA = 3 * MT * NT, PER = NMFMA / NREAD;        // MFMAs between two reads
    C2Frag<MT, NT> f[2];
    c2_load<MT, NT, COUT>(f[0], lin, lw, aoff[0], boff, 0);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if (s + 1 < KS) c2_load<MT, NT, COUT>(f[(s + 1) & 1], lin, lw, aoff[s + 1], boff, s + 1);
        if (s + 1 < KS) c2_products<MT, NT, false>(f[s & 1], acc);
        else { __builtin_amdgcn_sched_barrier(0); c2_products<MT, NT, true>(f[s & 1], acc); }
        if (s + 1 < KS) {
#pragma unroll
            for (int r = 0; r < NREAD; ++r) {
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                  // one DS read
                __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);                // PER MFMAs
            }
            __builtin_amdgcn_sched_group_barrier(0x008, NMFMA - PER * NREAD, 0);
        }
    }
}

template <int KS, int NT, int COUT>
__device__ __forceinline__ void c4_multiply(const unsigned char* __restrict__ lin, const unsigned char* __restrict__ lw,
                                            const int (&aoff)[KS], int boff, f32x4 (&acc)[4][NT], int nh) {
    constexpr int WPL = c4_wpl(COUT);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
        for (int h = 0; h < 4 / C4_MH; ++h) {
            if (h >= nh) break;                     // uniform: the right half of the last column tile of F = 480 lies outside the row
            bf16x8 av[3][C4_MH];
#pragma unroll
            for (int sp = 0; sp < 3; ++sp)
#pragma unroll
                for (int i = 0; i < C4_MH; ++i) av[sp][i] = *reinterpret_cast<const bf16x8*>(lin + sp * C4_INPL + aoff[s] + (C4_MH * h + i) * 16 * C4_PSTR);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                bf16x8 bv[3];
#pragma unroll
                for (int sp = 0; sp < 3; ++sp) bv[sp] = *reinterpret_cast<const bf16x8*>(lw + sp * WPL + boff + s * 2 * COUT * 16 + j * 256);
                // smallest terms first
#define C4_PRODUCT(SA, SB)                                                                                                   \
                _Pragma("unroll") for (int i = 0; i < C4_MH; ++i)                                                            \
                    acc[C4_MH * h + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[SA][i], bv[SB], acc[C4_MH * h + i][j], 0, 0, 0);
                C4_PRODUCT(2, 0) C4_PRODUCT(1, 1) C4_PRODUCT(0, 2) C4_PRODUCT(1, 0) C4_PRODUCT(0, 1) C4_PRODUCT(0, 0)
#undef C4_PRODUCT
            }
        }
    }
}

// TERMS = 3: every fp32 operand as three bf16 terms, six products (conv3x3_bf16x3 of round 1).  TERMS = 2: two fp16 terms, THREE
// products -- half the matrix-pipe work and two thirds of the LDS traffic for the same fp32-level result (a2s_common.h:
// split2_pair_f16); fp16's narrow exponent range is handled by exact power-of-two scales: the weights by 2^(13 - exponent of max|w|)
// (pack kernel), a gradient operand by 2^(12 - exponent of max|x|) (x_absmax, written by the kernel that produced it), an activated
// forward operand by the same power of two of its bound max_c(|scale_c| max|x_c| + |shift_c|) (the launcher puts that scalar in x_absmax); the
// accumulators are multiplied by the inverse power of two in the epilogue.
#ifdef C4_TRACE
// timing instrumentation (tools/conv_trace.py): shader-clock stamps of wave 0 of a few mid-grid workgroups, 8 stamps per stage
__device__ unsigned long long c4_trace[C4_TRACE_WGS * C4_TRACE_STAGES * 8];
extern "C" int a2s_conv_trace_read(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(c4_trace), sizeof(c4_trace));
}
#define C4_STAMP(k)                                                                                                           \
    do {                                                                                                                      \
        if (trace_wg >= 0 && q < C4_TRACE_STAGES && tid == 0) c4_trace[(trace_wg * C4_TRACE_STAGES + q) * 8 + (k)] = __builtin_readcyclecounter(); \
    } while (0)
#else
#define C4_STAMP(k) do {} while (0)
#endif
// workgroups per CU the two-term kernel is compiled for: its 52.9 KB of LDS would let a third in, but at the 168 registers that leaves
// there is room for ONE fragment register set only, and c4_multiply_f16x2 hides the LDS latency behind a second one
#define C4_WGS 2
template <int COUT, bool BNRED, int TERMS>
__global__ __launch_bounds__(256, (TERMS == 2 ? C4_WGS : 2)) void conv3x3_split(ConvArgs a, const unsigned char* __restrict__ wpack) {
    constexpr int NT = (COUT + 15) / 16;
    constexpr int WPL = c4_wpl(COUT);                    // bytes per term plane of a packed weight chunk
    constexpr int WCH = (TERMS * WPL + 4095) / 4096 * 4096;  // chunk stride of the packed image: whole 4 x 1 KB LDS-DMA rounds
    // LDS copy of a chunk: whole 1 KB DMA pieces.  The B fragments of the last n-tile read up to 7 rows past a slot (channels 40..47): past the
    // last slot that is beyond this array -- whatever lies there only reaches accumulator columns >= COUT, which are never stored.
    constexpr int WLDS = (TERMS * WPL + 1023) / 1024 * 1024;
    __shared__ __attribute__((aligned(16))) unsigned char lin[TERMS * C4_INPL];      // 38016 B (3 terms)
    __shared__ __attribute__((aligned(16))) unsigned char lw[WLDS];
    __shared__ float red[4][NT * 16][2];
    __shared__ __attribute__((aligned(16))) float lsc[48], lsh[48];                   // producer's BatchNorm scale / shift (0 beyond Cin)

    const int tilesF = (a.F + C2_FT - 1) / C2_FT;
    const int tilesT = (a.T + CV_TR - 1) / CV_TR;
    const int groupsT = (tilesT + C3_TPW - 1) / C3_TPW;
    // XCD-aware order: the hardware deals consecutive workgroup ids round-robin to the 8 XCDs (id % 8), each with its own L2.  Logical
    // tile L = (id % 8) * (n / 8) + id / 8 gives every XCD a contiguous run of tiles, so the F-tiles of a row group -- which share halo
    // columns and together read each 1920-byte activation row in full -- are resident on ONE XCD at the same time.
    int bid = blockIdx.x;
    {
        const int per = (int)gridDim.x / 8;
        if (bid < per * 8) bid = (bid % 8) * per + bid / 8;
    }
    const int ft = bid % tilesF; bid /= tilesF;
    const int tg = bid % groupsT; const int b = bid / groupsT;
    const int f0 = ft * C2_FT;
    const int tile0 = tg * C3_TPW, ntile = min(C3_TPW, tilesT - tile0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int ncgs = (a.Cin + 7) / 8, nchunks = (ncgs + 1) / 2;
    const int nstage = ntile * nchunks;

    f32x4 acc[4][NT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float st_s[NT], st_s2[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) { st_s[j] = 0.f; st_s2[j] = 0.f; }
    if (tid < 48) {
        lsc[tid] = (a.in_scale && tid < a.Cin) ? a.in_scale[tid] : 0.f;
        lsh[tid] = (a.in_scale && tid < a.Cin) ? a.in_shift[tid] : 0.f;
    }
    float xscale = 1.f, unscale = 1.f;                   // TERMS == 2: exact power-of-two operand scale and its inverse (times the weights')
    if (TERMS == 2) {
        const int kx = a.x_absmax ? pow2_scale_exp(*a.x_absmax, 12) : 0;
        const int kw = pow2_scale_exp(*a.w_absmax, 13);
        xscale = ldexpf(1.f, kx);
        unscale = ldexpf(1.f, -(kx + kw));
    }

    // per-lane fragment offsets: pair p = 4 s + lk of the chunk (clamped: the padded slots carry zero weights)
    int aoff2[5], aoff1[3];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int p = min(4 * s + lk, 17), tap = p >> 1;
        aoff2[s] = ((wave + tap / 3) * C4_POS + tap % 3 + li) * C4_PSTR + (p & 1) * 16;
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int tap = min(4 * s + lk, 8);
        aoff1[s] = ((wave + tap / 3) * C4_POS + tap % 3 + li) * C4_PSTR;
    }
    const int boff = (lk & 1) * c4_odd_base(COUT) + ((lk >> 1) * COUT + li) * 16;

    auto stage_tile = [&](int q) { return q / nchunks; };
    auto stage_chunk = [&](int q) { const int i = q / nchunks, c = q % nchunks; return (i & 1) ? nchunks - 1 - c : c; };

    float xreg[C4_XIT][8];
    // packed weight chunk -> LDS by LDS-DMA (global_load_lds_dwordx4: a wave copies 1 KB, lane-linear, no registers, no ds_write):
    // issued right after the barrier that retires the previous stage, in flight under the commit's BatchNorm / split arithmetic
    auto load_weights = [&](int ch) {
        const unsigned char* wsrc = wpack + (long)ch * WCH;
#pragma unroll
        for (int it = 0; it < (WLDS / 1024 + 3) / 4; ++it) {
            const int off = (it * 4 + wave) * 1024;
            if (off < WLDS)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc + off + lane * 16),
                                                 (__attribute__((address_space(3))) void*)(lw + off), 16, 0, 0);
        }
    };
    // Staging items of this thread, decoded ONCE: (row, position, group) packed in one register + the element offset relative to
    // the stage's (t0, first channel, f0) corner.  Inside the stage loop only "laundered" copies are used, so that nothing derived
    // from them is hoisted (the compiler otherwise keeps ~100 loop-invariant addresses in registers and spills around the multiply).
    int it_desc[C4_XIT], it_goff[C4_XIT];
#pragma unroll
    for (int it = 0; it < C4_XIT; ++it) {
        const int e = tid + 256 * it;
        const int cgl = e / C4_ITEMS, rp = e % C4_ITEMS;
        const int r = rp / C4_POS, pos = rp % C4_POS;
        it_desc[it] = r | (pos << 4) | (cgl << 12);
        it_goff[it] = ((r - 1) * a.Cin + cgl * 8) * a.F + pos - 1;
    }
    const int clip_elems = a.T * a.Cin * a.F;
    const float* __restrict__ xclip = a.x + (long)b * clip_elems;
    // raw buffer over this clip's input: a load whose byte offset falls outside [0, 4 clip_elems) returns 0 -- rows above / below the
    // clip, columns left of f = 0 on the first row -- so the addresses need no clamping (the clamped-index version spent ~6 VALU
    // instructions per scalar load, a third of the staging arithmetic); everything outside the tile's valid region is masked at commit
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xclip), 0, clip_elems * 4, 0x00020000);
    auto issue = [&](int q) {
        const int ch = stage_chunk(q), t0 = (tile0 + stage_tile(q)) * CV_TR;
        const int ncg = min(2, ncgs - 2 * ch);
        const int corner = (t0 * a.Cin + ch * 16) * a.F + f0;
#pragma unroll
        for (int it = 0; it < C4_XIT; ++it) {
            if (256 * it >= ncg * C4_ITEMS) break;                 // uniform: the one-group chunk has 396 items
            int g = it_goff[it];
            asm volatile("" : "+v"(g));
            g = (g + corner) * 4;
            const int plane = a.F * 4;
#pragma unroll
            for (int k = 0; k < 8; ++k) xreg[it][k] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(xrsrc, g + k * plane, 0, 0));
        }
    };
    auto commit = [&](int q) {     // registers -> LDS; BN+ReLU of the producer folded in; zero = padding (of the ACTIVATED tensor)
        const int ch = stage_chunk(q), t0 = (tile0 + stage_tile(q)) * CV_TR;
        const int ncg = min(2, ncgs - 2 * ch);
        const unsigned sgn = (q & 1) ? 0x80000000u : 0u;
#pragma unroll
        for (int it = 0; it < C4_XIT; ++it) {
            if (256 * it >= ncg * C4_ITEMS) break;
            int d = it_desc[it];
            asm volatile("" : "+v"(d));
            const int r = d & 15, pos = (d >> 4) & 255, cgl = d >> 12, rp = r * C4_POS + pos;
            if (cgl >= ncg) continue;
            const int t = t0 + r - 1, f = f0 + pos - 1, c0 = (ch * 2 + cgl) * 8;
            const bool ok = t >= 0 && t < a.T && f >= 0 && f < a.F;
            float v[8];
            if (a.in_scale) {                                     // lsc / lsh are zero beyond Cin: padded channels come out as 0
                const f32x4 sc0 = *reinterpret_cast<const f32x4*>(lsc + c0), sc1 = *reinterpret_cast<const f32x4*>(lsc + c0 + 4);
                const f32x4 sh0 = *reinterpret_cast<const f32x4*>(lsh + c0), sh1 = *reinterpret_cast<const f32x4*>(lsh + c0 + 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[k] = ok ? fmaxf(xreg[it][k] * sc0[k] + sh0[k], 0.f) : 0.f;
                    v[4 + k] = ok ? fmaxf(xreg[it][4 + k] * sc1[k] + sh1[k], 0.f) : 0.f;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (ok && c0 + k < a.Cin) ? xreg[it][k] : 0.f;
            }
            uint4 o[TERMS];
            if (TERMS == 3) {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = __uint_as_float(__float_as_uint(v[k]) ^ sgn);      // odd stages multiply -x (see the stage loop)
                split3_pair(v[0], v[1], o[0].x, o[1].x, o[TERMS - 1].x);
                split3_pair(v[2], v[3], o[0].y, o[1].y, o[TERMS - 1].y);
                split3_pair(v[4], v[5], o[0].z, o[1].z, o[TERMS - 1].z);
                split3_pair(v[6], v[7], o[0].w, o[1].w, o[TERMS - 1].w);
            } else {
                // the odd stages' sign rides on the power-of-two scale; activations are clamped to fp16's range in one v_med3 (with the
                // launcher's bound in x_absmax it never bites), a gradient operand is already inside it by construction of its scale
                const float xs = sgn ? -xscale : xscale;
                if (a.in_scale) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = __builtin_amdgcn_fmed3f(v[k] * xs, -65000.f, 65000.f);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] *= xs;
                }
                split2_pair_f16(v[0], v[1], o[0].x, o[1].x);
                split2_pair_f16(v[2], v[3], o[0].y, o[1].y);
                split2_pair_f16(v[4], v[5], o[0].z, o[1].z);
                split2_pair_f16(v[6], v[7], o[0].w, o[1].w);
            }
#pragma unroll
            for (int sp = 0; sp < TERMS; ++sp) *reinterpret_cast<uint4*>(lin + sp * C4_INPL + rp * C4_PSTR + cgl * 16) = o[sp];
        }
    };

    int resident = -1;
    bool acc_neg = false;
    const int nh = (f0 + C4_MH * 16 >= a.F) ? 1 : 4 / C4_MH;      // m-tile passes that hold any valid column (F = 480: 7.5 tiles of 64)
    const bool half_tile = f0 + 32 >= a.F;                        // two-term kernel: two m-tiles instead of four
    auto flip_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = -acc[i][j][r];
    };
#ifdef C4_TRACE
    const int trace_first = (int)gridDim.x / 2;
    const int trace_wg = ((int)blockIdx.x >= trace_first && (int)blockIdx.x < trace_first + C4_TRACE_WGS) ? (int)blockIdx.x - trace_first : -1;
#endif
    // the next stage's input loads are issued before this stage's multiply (with three products per k-step the multiply no
    // longer covers the other workgroup's load round trip; round 1, six products: no gain)
    if (nstage > 0) issue(0);
    for (int q = 0; q < nstage; ++q) {
        C4_STAMP(0);
        __syncthreads();                      // previous stage fully consumed
        C4_STAMP(1);
        if (stage_chunk(q) != resident) load_weights(stage_chunk(q));
        commit(q);
        resident = stage_chunk(q);
        C4_STAMP(2);
        __syncthreads();
        C4_STAMP(3);
        if (q + 1 < nstage) issue(q + 1);
        C4_STAMP(4);
        // The bf16 matrix pipe truncates its internal sum toward -infinity (measured: mean error -3e-9 sum|a||b|, always negative, against
        // a random part of 5e-8) -- nothing for one output, but the BatchNorm sums over 10^6 positions see 70x their random error.  Odd
        // stages therefore accumulate the NEGATED sum (input negated while staging, accumulators flipped): the truncation then pushes
        // the value the other way, and a tile's stages / neighbouring tiles cancel.
        if (acc_neg != bool(q & 1)) { flip_acc(); acc_neg = !acc_neg; }
        if (TERMS == 3) {
            if (ncgs - 2 * resident >= 2) c4_multiply<5, NT, COUT>(lin, lw, aoff2, boff, acc, nh);
            else c4_multiply<3, NT, COUT>(lin, lw, aoff1, boff, acc, nh);
        } else {
            if (half_tile) {
                if (ncgs - 2 * resident >= 2) c4_multiply_f16x2<5, 2, NT, COUT>(lin, lw, aoff2, boff, acc);
                else c4_multiply_f16x2<3, 2, NT, COUT>(lin, lw, aoff1, boff, acc);
            } else {
                if (ncgs - 2 * resident >= 2) c4_multiply_f16x2<5, 4, NT, COUT>(lin, lw, aoff2, boff, acc);
                else c4_multiply_f16x2<3, 4, NT, COUT>(lin, lw, aoff1, boff, acc);
            }
        }
        C4_STAMP(5);
        if ((q + 1) % nchunks != 0) continue;
        if (acc_neg) { flip_acc(); acc_neg = false; }
        if (TERMS == 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][j][r] *= unscale;
        }
        // ---- tile epilogue.  C/D map: lane holds column n = li (channel), rows lk*4+r (f positions) of each m-tile.
        const int t = (tile0 + stage_tile(q)) * CV_TR + wave;
        const bool row_ok = t < a.T;
        int li_ = li, lk_ = lk;
        asm volatile("" : "+v"(li_), "+v"(lk_));
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int co = j * 16 + li_;
            float bm = 0.f, bi = 0.f, bsc = 0.f, bsh = 0.f;
            f32x4 yv[4];
            if (BNRED && row_ok && co < COUT) {
                bm = a.yl_mean[co]; bi = a.yl_invstd[co]; bsc = a.yl_scale[co]; bsh = a.yl_shift[co];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int f = f0 + i * 16 + lk_ * 4;
                    const float* src = a.yl + (((long)b * a.T + t) * COUT + co) * a.F + f;
                    if (f + 3 < a.F && (a.F % 4 == 0)) yv[i] = *reinterpret_cast<const f32x4*>(src);
                    else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) yv[i][r] = (f + r < a.F) ? src[r] : 0.f;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = f0 + i * 16 + lk_ * 4;
                if (row_ok && co < COUT) {
                    float* dst = a.y + (((long)b * a.T + t) * COUT + co) * a.F + f;
                    const bool full = f + 3 < a.F && (a.F % 4 == 0);
                    if (full) *reinterpret_cast<f32x4*>(dst) = acc[i][j];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (!full && f + r >= a.F) continue;
                        const float v = acc[i][j][r];
                        if (!full) dst[r] = v;
                        if (BNRED) {
                            const float xv = yv[i][r];
                            const float gm = (xv * bsc + bsh > 0.f) ? v : 0.f;
                            st_s[j] += gm; st_s2[j] += gm * (xv - bm) * bi;
                        } else { st_s[j] += v; st_s2[j] += v * v; }
                    }
                }
                acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            __builtin_amdgcn_sched_barrier(0);        // one n-tile at a time: hoisting every yl load spills the prefetched input
        }
        C4_STAMP(6);
    }
    if (a.stat_partial) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            float s = st_s[j], s2 = st_s2[j];
            s += __shfl_xor(s, 16, 64); s2 += __shfl_xor(s2, 16, 64);
            s += __shfl_xor(s, 32, 64); s2 += __shfl_xor(s2, 32, 64);
            if (lk == 0) { red[wave][j * 16 + li][0] = s; red[wave][j * 16 + li][1] = s2; }
        }
        __syncthreads();
        if (tid < COUT) {
            float s = 0.f, s2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { s += red[w][tid][0]; s2 += red[w][tid][1]; }
            a.stat_partial[((long)blockIdx.x * COUT + tid) * 2 + 0] = s;
            a.stat_partial[((long)blockIdx.x * COUT + tid) * 2 + 1] = s2;
        }
    }
}

// First layer: Cin = 1.  A streaming kernel (53 GFLOP at B = 256 against 12 GB written): a thread owns 4 consecutive f positions of a
// row (16-byte stores of every output channel), walks the rows grid-stride, and keeps its per-channel sum / sum of squares in
// registers -- the batch-statistics partials are reduced ONCE per workgroup at the end (the first version reduced 40 values across the
// wave for every position and wrote 92 MB of partials).  C1_BLOCKS workgroups = that many partial rows.
#define C1_BLOCKS 2048
__global__ __launch_bounds__(256) void conv3x3_c1(ConvArgs a) {
    __shared__ float lw[20 * 9];
    __shared__ float red[4][20][2];
    for (int e = threadIdx.x; e < a.Cout * 9; e += 256) lw[e] = a.w[e];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qpr = (a.F + 3) / 4;                               // quads per row
    const long nquads = (long)a.B * a.T * qpr;
    const bool vec = (a.F % 4 == 0) && (((uintptr_t)a.y & 15) == 0);
    float s1[20], s2[20], m1[20];
#pragma unroll
    for (int co = 0; co < 20; ++co) { s1[co] = 0.f; s2[co] = 0.f; m1[co] = 0.f; }
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nquads; q += (long)gridDim.x * 256) {
        const int f0 = (int)(q % qpr) * 4;
        const long row = q / qpr;                                // b * T + t
        const int t = (int)(row % a.T);
        float v[3][6];                                           // input window: rows t-1..t+1, columns f0-1..f0+4
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
            const int tt = t + dt - 1;
            const float* xr = a.x + (row + dt - 1) * a.F;
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const int ff = f0 + c - 1;
                v[dt][c] = (tt >= 0 && tt < a.T && ff >= 0 && ff < a.F) ? xr[ff] : 0.f;
            }
        }
#pragma unroll
        for (int co = 0; co < 20; ++co) {
            if (co >= a.Cout) break;
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dt = 0; dt < 3; ++dt)
#pragma unroll
                for (int df = 0; df < 3; ++df) {
                    const float w = lw[co * 9 + dt * 3 + df];
#pragma unroll
                    for (int p = 0; p < 4; ++p) o[p] = fmaf(v[dt][p + df], w, o[p]);
                }
            float* dst = a.y + (row * a.Cout + co) * a.F + f0;
            if (vec) {
                *reinterpret_cast<f32x4*>(dst) = o;
#pragma unroll
                for (int p = 0; p < 4; ++p) { s1[co] += o[p]; s2[co] = fmaf(o[p], o[p], s2[co]); }
                m1[co] = fmaxf(fmaxf(m1[co], fmaxf(fabsf(o[0]), fabsf(o[1]))), fmaxf(fabsf(o[2]), fabsf(o[3])));
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) if (f0 + p < a.F) { dst[p] = o[p]; s1[co] += o[p]; s2[co] = fmaf(o[p], o[p], s2[co]); m1[co] = fmaxf(m1[co], fabsf(o[p])); }
            }
        }
    }
    if (a.out_absmax) {          // per-channel max |y|: the next layer derives its operand scale from it (a2s_conv_rows.hip)
#pragma unroll
        for (int co = 0; co < 20; ++co) {
            if (co >= a.Cout) break;
            const float m = wave_max(m1[co]);
            if (lane == 0) {
                const unsigned bits = __float_as_uint(m);
                if (bits > __hip_atomic_load(reinterpret_cast<unsigned*>(a.out_absmax + co), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    atomicMax(reinterpret_cast<unsigned*>(a.out_absmax + co), bits);
            }
        }
    }
    if (a.stat_partial) {
#pragma unroll
        for (int co = 0; co < 20; ++co) {
            if (co >= a.Cout) break;
            const float w1 = wave_sum(s1[co]), w2 = wave_sum(s2[co]);
            if (lane == 0) { red[wave][co][0] = w1; red[wave][co][1] = w2; }
        }
        __syncthreads();
        if (threadIdx.x < a.Cout) {
            float s = 0.f, q2 = 0.f;
            for (int w = 0; w < 4; ++w) { s += red[w][threadIdx.x][0]; q2 += red[w][threadIdx.x][1]; }
            a.stat_partial[((long)blockIdx.x * a.Cout + threadIdx.x) * 2 + 0] = s;
            a.stat_partial[((long)blockIdx.x * a.Cout + threadIdx.x) * 2 + 1] = q2;
        }
    }
}

// The same kernel with the channel count fixed at compile time and F a multiple of 4 (the model's 20 x 480): with a run-time Cout the
// per-channel accumulators above are indexed dynamically (s_set_gpr_idx and ~50 register moves per channel: 3070 VALU instructions per
// quad, the kernel ran at the VALU's pace, 4.4 ms at B = 256 against 2.1 ms of HBM time).  Here everything unrolls: one aligned 16-byte
// load and two edge scalars per window row, packed fp32 FMAs, the same order of operations per output -- results are bit-identical.
template <int COUT>
__global__ __launch_bounds__(256, 4) void conv3x3_c1_fixed(ConvArgs a) {
    __shared__ __attribute__((aligned(16))) float lw[COUT * 12];             // 9 taps per channel, padded to 12 for 16-byte reads
    __shared__ float red[4][COUT][2];
    for (int e = threadIdx.x; e < COUT * 12; e += 256) lw[e] = (e % 12 < 9) ? a.w[(e / 12) * 9 + e % 12] : 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qpr = a.F / 4;
    const long nquads = (long)a.B * a.T * qpr;
    float s1[COUT], s2[COUT], m1[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) { s1[co] = 0.f; s2[co] = 0.f; m1[co] = 0.f; }
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nquads; q += (long)gridDim.x * 256) {
        const int f0 = (int)(q % qpr) * 4;
        const long row = q / qpr;
        const int t = (int)(row % a.T);
        float v[3][6];
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
            const int tt = t + dt - 1;
            const bool in = tt >= 0 && tt < a.T;
            const float* xr = a.x + (row + dt - 1) * a.F + f0;
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            float l = 0.f, r = 0.f;
            if (in) {
                c = *reinterpret_cast<const f32x4*>(xr);
                if (f0 > 0) l = xr[-1];
                if (f0 + 4 < a.F) r = xr[4];
            }
            v[dt][0] = l; v[dt][1] = c[0]; v[dt][2] = c[1]; v[dt][3] = c[2]; v[dt][4] = c[3]; v[dt][5] = r;
        }
        float* dst = a.y + row * COUT * a.F + f0;
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
            asm volatile("" ::: "memory");            // the taps are re-read from LDS per channel: hoisted out of the loop they cost 180 registers
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(&lw[co * 12]), w1 = *reinterpret_cast<const f32x4*>(&lw[co * 12 + 4]);
            const float w8 = lw[co * 12 + 8];
            const float w[9] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3], w8};
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dt = 0; dt < 3; ++dt)
#pragma unroll
                for (int df = 0; df < 3; ++df)
#pragma unroll
                    for (int p = 0; p < 4; ++p) o[p] = fmaf(v[dt][p + df], w[dt * 3 + df], o[p]);
            __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(dst + (long)co * a.F));
#pragma unroll
            for (int p = 0; p < 4; ++p) { s1[co] += o[p]; s2[co] = fmaf(o[p], o[p], s2[co]); }
            m1[co] = fmaxf(fmaxf(m1[co], fmaxf(fabsf(o[0]), fabsf(o[1]))), fmaxf(fabsf(o[2]), fabsf(o[3])));
        }
    }
    if (a.out_absmax) {
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
            const float m = wave_max(m1[co]);
            if (lane == 0) {
                const unsigned bits = __float_as_uint(m);
                if (bits > __hip_atomic_load(reinterpret_cast<unsigned*>(a.out_absmax + co), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    atomicMax(reinterpret_cast<unsigned*>(a.out_absmax + co), bits);
            }
        }
    }
    if (a.stat_partial) {
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
            const float w1 = wave_sum(s1[co]), w2 = wave_sum(s2[co]);
            if (lane == 0) { red[wave][co][0] = w1; red[wave][co][1] = w2; }
        }
        __syncthreads();
        if (threadIdx.x < COUT) {
            float s = 0.f, q2 = 0.f;
            for (int w = 0; w < 4; ++w) { s += red[w][threadIdx.x][0]; q2 += red[w][threadIdx.x][1]; }
            a.stat_partial[((long)blockIdx.x * COUT + threadIdx.x) * 2 + 0] = s;
            a.stat_partial[((long)blockIdx.x * COUT + threadIdx.x) * 2 + 1] = q2;
        }
    }
}

// out[0] = max_c (|scale_c| absmax_c + |shift_c|): a hard bound of relu(x scale_c + shift_c) over the tensor, given the per-channel
// max |x_c| its producer wrote (a2s_conv3x3_ranged) -- the operand range of the kernels that read the activated tensor on the fly
__global__ void act_bound_kernel(const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ absmax, int C, float* __restrict__ out) {
    float m = 0.f;
    for (int c = threadIdx.x; c < C; c += 64) m = fmaxf(m, fabsf(scale[c]) * absmax[c] + fabsf(shift[c]));
    m = wave_max(m);
    if (threadIdx.x == 0) *out = m;
}
int a2s_act_bound_impl(hipStream_t st, const float* scale, const float* shift, const float* absmax, int C, float* out) {
    A2S_REQUIRE(scale && shift && absmax && out && C > 0, "act_bound: null tensor");
    hipLaunchKernelGGL(act_bound_kernel, dim3(1), dim3(64), 0, st, scale, shift, absmax, C, out);
    A2S_CHECK_LAUNCH("act_bound");
    return A2S_OK;
}

// ------------------------------------------------------------------------------------------- launchers
// Switches (a2s_switches.h): "conv_c1_fast", "conv_bf16x3" and, of the latter's launches, "conv_f16x2" -- a data-gradient launch additionally
// needs the max |dy| scalar of its operand (a2s_conv3x3_dgrad_bnstats_scaled) and stays on three terms without it

// the row-streaming kernel of a2s_conv_rows.hip (forward and data-gradient launches with F % 4 == 0, 20 / 40 channels)

size_t a2s_conv3x3_workspace_floats_impl(int Cin) {
    if (Cin == 1) return 0;
    const size_t f32_image = (size_t)(Cin / CV_CK) * C2_WCHUNK, split_image = (size_t)c4_chunks(Cin) * c4_chunk_bytes(40) / 4;
    // + the per-channel max |x| scratch, the max |w| scalar and the activation bound of the two-term path
    const size_t tiled = (f32_image > split_image ? f32_image : split_image) + 64 + 4;
    const size_t rows = a2s_conv_rows_workspace_floats(Cin);
    return tiled > rows ? tiled : rows;
}

int a2s_conv3x3_impl(hipStream_t st, const float* x, const float* w, float* y, const float* in_scale,
                     const float* in_shift, float* stat_partial, int B, int T, int F, int Cin, int Cout, int flip, float* ws,
                     const float* yl, const float* yl_mean, const float* yl_invstd, const float* yl_scale, const float* yl_shift,
                     const float* x_absmax, const float* in_absmax, float* out_absmax) {
    A2S_REQUIRE(x && w && y, "conv3x3: null tensor");
    A2S_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "conv3x3: scale/shift must come together");
    A2S_REQUIRE(!yl || (yl_mean && yl_invstd && yl_scale && yl_shift && stat_partial && Cin != 1), "conv3x3: the fused BatchNorm-backward statistics need all of their tensors");
    ConvArgs a{x, w, y, in_scale, in_shift, stat_partial, B, T, F, Cin, Cout, flip, yl, yl_mean, yl_invstd, yl_scale, yl_shift, x_absmax, nullptr, out_absmax};
    if (Cin != 1 && a2s_conv_rows_eligible(F, Cin) && (Cout == 20 || Cout == 40)) {
        A2S_REQUIRE(ws, "conv3x3: needs a workspace of a2s_conv3x3_workspace_floats(Cin) floats for the packed weights");
        return a2s_conv3x3_rows_impl(st, x, w, y, in_scale, in_shift, in_absmax, stat_partial, out_absmax, B, T, F, Cin, Cout, flip, ws,
                                     yl, yl_mean, yl_invstd, yl_scale, yl_shift, x_absmax);
    }
    if (out_absmax && Cin == 1) {       // accumulated by atomic max in the first-layer kernel
        const hipError_t me = hipMemsetAsync(out_absmax, 0, sizeof(float) * Cout, st);
        A2S_REQUIRE(me == hipSuccess, "conv3x3: hipMemsetAsync(out_absmax): %s", hipGetErrorString(me));
    }
    if (out_absmax && Cin != 1) {       // the tiled kernels do not track it (A/B switch, odd shapes): one extra pass over y afterwards
        const int rc = a2s_conv3x3_impl(st, x, w, y, in_scale, in_shift, stat_partial, B, T, F, Cin, Cout, flip, ws, yl, yl_mean, yl_invstd, yl_scale, yl_shift,
                                        x_absmax, in_absmax, nullptr);
        return rc != A2S_OK ? rc : a2s_channel_absmax_impl(st, y, (long)B * T, Cout, F, out_absmax);
    }
    if (Cin == 1) {
        A2S_REQUIRE(Cout <= 20 && !flip && !in_scale, "conv3x3: Cin=1 path supports Cout<=20, no flip, no input affine");
        const bool fixed = a2s_sw(A2S_SW_conv_c1_fast) && Cout == 20 && F % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;
        if (fixed) hipLaunchKernelGGL(conv3x3_c1_fixed<20>, dim3(a2s_conv3x3_stat_blocks_impl(B, T, F, 1)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(conv3x3_c1, dim3(a2s_conv3x3_stat_blocks_impl(B, T, F, 1)), dim3(256), 0, st, a);
    } else {
        A2S_REQUIRE(Cin % 4 == 0 && Cin % CV_CK == 0, "conv3x3: Cin must be a multiple of %d", CV_CK);
        A2S_REQUIRE(ws, "conv3x3: needs a workspace of a2s_conv3x3_workspace_floats(Cin) floats for the packed weights");
        A2S_REQUIRE(Cout == 20 || Cout == 40, "conv3x3: Cout must be 20 or 40 (got %d)", Cout);
        // the kernels below come in four instances, Cout 20 / 40 x plain / fused statistics of the layer below (yl): launch(co, red) gets the pair
        // as compile-time constants
        auto with_instance = [&](auto launch) {
            if (Cout == 20 && !yl) launch(std::integral_constant<int, 20>{}, std::false_type{});
            else if (Cout == 20) launch(std::integral_constant<int, 20>{}, std::true_type{});
            else if (!yl) launch(std::integral_constant<int, 40>{}, std::false_type{});
            else launch(std::integral_constant<int, 40>{}, std::true_type{});
        };
        const int nblk4 = B * a2s_cdiv(a2s_cdiv(T, CV_TR), C3_TPW) * a2s_cdiv(F, C2_FT);
        if (a2s_sw(A2S_SW_conv_bf16x3) & (flip ? 2 : 1)) {
            // two fp16 terms when enabled -- a gradient operand (flip) only with its max |x| scalar: fp16 has no exponent range to spare
            const bool two = (a2s_sw(A2S_SW_conv_f16x2) & (flip ? 2 : 1)) && (!flip || x_absmax);
            const int terms = two ? 2 : 3;
            const int n = c4_chunks(Cin) * C4_SLOTS * Cout * 8;
            const size_t image = c4_chunks(Cin) * c4_chunk_bytes(Cout, terms);
            const hipError_t me = hipMemsetAsync(ws, 0, image, st);
            A2S_REQUIRE(me == hipSuccess, "conv3x3: hipMemsetAsync(packed weights): %s", hipGetErrorString(me));
            float* wmax = ws + a2s_conv3x3_workspace_floats_impl(Cin) - 4;
            const unsigned char* wp = (const unsigned char*)ws;
            if (two) {
                a2s_absmax_small_launch(st, w, Cout * Cin * 9, wmax);
                hipLaunchKernelGGL(conv_pack_weights_split<2>, dim3(a2s_cdiv(n, 256)), dim3(256), 0, st, w, (unsigned short*)ws, Cin, Cout, flip, (const float*)wmax);
                A2S_CHECK_LAUNCH("conv_pack_weights_split<2>");
                a.w_absmax = wmax;
                if (!flip && in_scale) {
                    // An ACTIVATED forward operand relu(x scale_c + shift_c) is scaled like a gradient operand, by the power of two that brings its bound
                    // (a2s_act_bound of the per-channel max |x| its producer wrote; measured here for a caller without it) to 2^12: BatchNorm's gamma is
                    // a free parameter, unscaled activations of order 1e5 saturate fp16 (finite, wrong outputs), those of order 1e-3 lose the second term.
                    if (!in_absmax) {
                        float* scratch = wmax - 64;
                        const int rc = a2s_channel_absmax_impl(st, x, (long)B * T, Cin, F, scratch);
                        if (rc != A2S_OK) return rc;
                        in_absmax = scratch;
                    }
                    hipLaunchKernelGGL(act_bound_kernel, dim3(1), dim3(64), 0, st, in_scale, in_shift, in_absmax, Cin, wmax + 1);
                    A2S_CHECK_LAUNCH("act_bound (tiled forward)");
                    a.x_absmax = wmax + 1;
                }
                with_instance([&](auto co, auto red) { hipLaunchKernelGGL((conv3x3_split<co(), red(), 2>), dim3(nblk4), dim3(256), 0, st, a, wp); });
                A2S_CHECK_LAUNCH("conv3x3_split<2>");
                return A2S_OK;
            }
            hipLaunchKernelGGL(conv_pack_weights_split<3>, dim3(a2s_cdiv(n, 256)), dim3(256), 0, st, w, (unsigned short*)ws, Cin, Cout, flip, (const float*)nullptr);
            A2S_CHECK_LAUNCH("conv_pack_weights_split<3>");
            with_instance([&](auto co, auto red) { hipLaunchKernelGGL((conv3x3_split<co(), red(), 3>), dim3(nblk4), dim3(256), 0, st, a, wp); });
            A2S_CHECK_LAUNCH("conv3x3_split<3>");
            return A2S_OK;
        }
        const int chunks = Cin / CV_CK;
        hipLaunchKernelGGL(conv_pack_weights, dim3(a2s_cdiv(chunks * C2_WCHUNK, 256)), dim3(256), 0, st, w, ws, Cin, Cout, flip, chunks);
        A2S_CHECK_LAUNCH("conv_pack_weights");
        const int nblk = B * a2s_cdiv(a2s_cdiv(T, CV_TR), C3_TPW) * a2s_cdiv(F, C2_FT);
        with_instance([&](auto co, auto red) { hipLaunchKernelGGL((conv3x3_mfma<co(), red()>), dim3(nblk), dim3(256), 0, st, a, (const float*)ws); });
    }
    A2S_CHECK_LAUNCH("conv3x3");
    return A2S_OK;
}

int a2s_conv3x3_stat_blocks_impl(int B, int T, int F, int Cin) {
    if (Cin == 1) {       // the streaming first-layer kernel: at most C1_BLOCKS grid-stride workgroups
        const long want = a2s_cdiv((long)B * T * ((F + 3) / 4), 256);
        return (int)(want < C1_BLOCKS ? want : C1_BLOCKS);
    }
    if (a2s_conv_rows_eligible(F, Cin)) return a2s_conv_rows_blocks(B, T, F);
    return B * a2s_cdiv(a2s_cdiv(T, CV_TR), C3_TPW) * a2s_cdiv(F, C2_FT);
}
