// BatchNorm with batch statistics, forward and backward, for the (rows, C, F) activations of the ConvStack and the (rows, C) output of its
// Linear.  The statistics partials [nblocks][C][2] come from the epilogues of the kernels that produce the tensor (convolutions, GEMM) or
// from the column / plane reductions here; everything is reduced in a fixed order (deterministic).
#include "a2s_internal.h"

// ------------------------------------------------------------------------------------------- BatchNorm
// Fixed-order reduction of the per-workgroup partials in double (the reference's CPU kernel accumulates
// batch statistics in double: at::acc_type<float> on CPU), then the affine the consumer applies on load.
struct BnFinalizeArgs {
    const float* partial; int nblocks; int C; double count;
    const float* gamma; const float* beta;
    float* running_mean; float* running_var; long long* num_batches_tracked;   // updated when training
    float* mean; float* invstd;          // saved for backward
    float* scale; float* shift;          // y = x*scale + shift
    float eps, momentum; int training;
};

__global__ __launch_bounds__(256) void bn_finalize(BnFinalizeArgs a) {
    const int c = blockIdx.x;
    __shared__ double rs[256], rs2[256];
    double s = 0.0, s2 = 0.0;
    if (a.training) {
        for (int i = threadIdx.x; i < a.nblocks; i += 256) {
            s += (double)a.partial[((long)i * a.C + c) * 2 + 0];
            s2 += (double)a.partial[((long)i * a.C + c) * 2 + 1];
        }
    }
    rs[threadIdx.x] = s; rs2[threadIdx.x] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { rs[threadIdx.x] += rs[threadIdx.x + o]; rs2[threadIdx.x] += rs2[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double mean, var;
        if (a.training) {
            mean = rs[0] / a.count;
            var = rs2[0] / a.count - mean * mean;          // biased; double keeps the cancellation harmless
            if (var < 0.0) var = 0.0;
            const double unb = a.count > 1.0 ? var * a.count / (a.count - 1.0) : var;
            a.running_mean[c] = (float)((1.0 - a.momentum) * a.running_mean[c] + a.momentum * mean);
            a.running_var[c] = (float)((1.0 - a.momentum) * a.running_var[c] + a.momentum * unb);
            if (c == 0 && a.num_batches_tracked) *a.num_batches_tracked += 1;
        } else {
            mean = a.running_mean[c]; var = a.running_var[c];
        }
        const double inv = 1.0 / sqrt(var + (double)a.eps);
        a.mean[c] = (float)mean; a.invstd[c] = (float)inv;
        const double sc = (double)a.gamma[c] * inv;
        a.scale[c] = (float)sc;
        a.shift[c] = (float)((double)a.beta[c] - mean * sc);
    }
}

// y = relu(x*scale[c] + shift[c]) over (rows, C, F) planes -- materialises the last ConvStack activation as
// the (B*T, C*F) operand of the 19200->256 GEMM.
__global__ void bn_relu_apply(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ scale,
                              const float* __restrict__ shift, long n, int C, int F) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int c = (int)((i / F) % C);
        y[i] = fmaxf(x[i] * scale[c] + shift[c], 0.f);
    }
}

// Column statistics of a (rows, C) matrix (BatchNorm1d of the Linear output, reference models.py:505,539):
// partial sums per row block, same [nblocks][C][2] format as the conv epilogue.
__global__ __launch_bounds__(256) void col_stats_partial(const float* __restrict__ x, float* __restrict__ partial,
                                                         long rows, int C, int rows_per_block) {
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = min(rows, r0 + rows_per_block);
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f, s2 = 0.f;
        for (long r = r0; r < r1; ++r) { const float v = x[r * C + c]; s += v; s2 += v * v; }
        partial[((long)blockIdx.x * C + c) * 2 + 0] = s;
        partial[((long)blockIdx.x * C + c) * 2 + 1] = s2;
    }
}

// The same sums kept in double and written as TWO fp32 terms: entry blockIdx.x holds the fp32 heads of the block's sums, entry nblocks + blockIdx.x
// what the heads left over.  bn_finalize adds the 2 * nblocks entries in double and gets the sums to ~48 bits, so var = E[x^2] - mean^2 stays exact
// where the variance is far below mean^2 (few rows with nearly equal values: an fp32 sum of squares is off by 2^-24 mean^2 there, which against
// var + eps = 1e-5 was 0.7 % of invstd in a two-row call).
__global__ __launch_bounds__(256) void col_stats_partial_split(const float* __restrict__ x, float* __restrict__ partial,
                                                               long rows, int C, int rows_per_block) {
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = min(rows, r0 + rows_per_block);
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0, s2 = 0.0;
        for (long r = r0; r < r1; ++r) { const double v = (double)x[r * C + c]; s += v; s2 += v * v; }
        const float sh = (float)s, s2h = (float)s2;
        float* head = partial + ((long)blockIdx.x * C + c) * 2;
        float* rest = partial + (((long)gridDim.x + blockIdx.x) * C + c) * 2;
        head[0] = sh; head[1] = s2h;
        rest[0] = (float)(s - (double)sh); rest[1] = (float)(s2 - (double)s2h);
    }
}

// y[r,c] = relu(x[r,c]*scale[c]+shift[c]) (* dropout mask/keep when mask != null)
__global__ void bn1d_relu_dropout(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ scale,
                                  const float* __restrict__ shift, const uint8_t* __restrict__ mask, float inv_keep,
                                  long n, int C) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int c = (int)(i % C);
        float v = fmaxf(x[i] * scale[c] + shift[c], 0.f);
        if (mask) v = mask[i] ? v * inv_keep : 0.f;
        y[i] = v;
    }
}

int a2s_bn_finalize_impl(hipStream_t st, const float* partial, int nblocks, int C, double count, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, long long* nbt, float* mean,
                         float* invstd, float* scale, float* shift, float eps, float momentum, int training) {
    A2S_REQUIRE(gamma && beta && running_mean && running_var && mean && invstd && scale && shift, "bn_finalize: null tensor");
    A2S_REQUIRE(!training || partial, "bn_finalize: training needs the statistics partials");
    BnFinalizeArgs a{partial, nblocks, C, count, gamma, beta, running_mean, running_var, nbt, mean, invstd, scale, shift, eps, momentum, training};
    hipLaunchKernelGGL(bn_finalize, dim3(C), dim3(256), 0, st, a);
    A2S_CHECK_LAUNCH("bn_finalize");
    return A2S_OK;
}

int a2s_bn_relu_apply_impl(hipStream_t st, const float* x, float* y, const float* scale, const float* shift, long n, int C, int F) {
    hipLaunchKernelGGL(bn_relu_apply, dim3(min((long)4096, (n + 255) / 256)), dim3(256), 0, st, x, y, scale, shift, n, C, F);
    A2S_CHECK_LAUNCH("bn_relu_apply");
    return A2S_OK;
}

int a2s_col_stats_split_impl(hipStream_t st, const float* x, float* partial, long rows, int C, int rows_per_block) {
    A2S_REQUIRE(x && partial && rows > 0 && C > 0 && rows_per_block > 0, "col_stats_split: null tensor or empty shape");
    hipLaunchKernelGGL(col_stats_partial_split, dim3(a2s_cdiv(rows, rows_per_block)), dim3(256), 0, st, x, partial, rows, C, rows_per_block);
    A2S_CHECK_LAUNCH("col_stats_partial_split");
    return A2S_OK;
}
int a2s_col_stats_impl(hipStream_t st, const float* x, float* partial, long rows, int C, int rows_per_block) {
    hipLaunchKernelGGL(col_stats_partial, dim3(a2s_cdiv(rows, rows_per_block)), dim3(256), 0, st, x, partial, rows, C, rows_per_block);
    A2S_CHECK_LAUNCH("col_stats_partial");
    return A2S_OK;
}

int a2s_bn1d_relu_dropout_impl(hipStream_t st, const float* x, float* y, const float* scale, const float* shift,
                               const uint8_t* mask, float inv_keep, long n, int C) {
    hipLaunchKernelGGL(bn1d_relu_dropout, dim3(min((long)4096, (n + 255) / 256)), dim3(256), 0, st, x, y, scale, shift, mask, inv_keep, n, C);
    A2S_CHECK_LAUNCH("bn1d_relu_dropout");
    return A2S_OK;
}

// =========================================================================================== backward
// BatchNorm (+ReLU, + optional dropout) backward in three steps, with y = x*scale + shift, xh = (x-mean)*invstd:
//   g' = g * [y > 0] (* keep*inv_keep);  s1 = sum g', s2 = sum g' xh  (per channel, fixed-order reduction);
//   dbeta += s1, dgamma += s2;  dx = gamma*invstd * (g' - s1/N - xh * s2/N).
// Plane layout (rows, C, F): block = one row, wave per channel plane.  Matrix layout (rows, C): see *_cols.
__global__ __launch_bounds__(256) void bn_bwd_reduce_planes(const float* __restrict__ g, const float* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            float* __restrict__ partial, int C, int F) {
    const long row = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < C; c += 4) {
        const float* gp = g + (row * C + c) * F;
        const float* xp = x + (row * C + c) * F;
        const float m = mean[c], is = invstd[c], sc = scale[c], sh = shift[c];
        float s1 = 0.f, s2 = 0.f;
        for (int f = lane; f < F; f += 64) {
            const float xv = xp[f];
            const float gv = (xv * sc + sh > 0.f) ? gp[f] : 0.f;
            s1 += gv; s2 += gv * (xv - m) * is;
        }
        s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane == 0) { partial[(row * C + c) * 2 + 0] = s1; partial[(row * C + c) * 2 + 1] = s2; }
    }
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_cols(const float* __restrict__ g, const float* __restrict__ x,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                                          const uint8_t* __restrict__ mask, float inv_keep,
                                                          float* __restrict__ partial, long rows, int C, int rows_per_block) {
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    for (int c = threadIdx.x; c < C; c += 256) {
        const float m = mean[c], is = invstd[c], sc = scale[c], sh = shift[c];
        float s1 = 0.f, s2 = 0.f;
        for (long r = r0; r < r1; ++r) {
            const float xv = x[r * C + c];
            float gv = (xv * sc + sh > 0.f) ? g[r * C + c] : 0.f;
            if (mask) gv = mask[r * C + c] ? gv * inv_keep : 0.f;
            s1 += gv; s2 += gv * (xv - m) * is;
        }
        partial[((long)blockIdx.x * C + c) * 2 + 0] = s1;
        partial[((long)blockIdx.x * C + c) * 2 + 1] = s2;
    }
}

// one block per channel: fixed-order double reduction of the partials -> dgamma/dbeta (+=) and c1 = s1/N, c2 = s2/N
__global__ __launch_bounds__(256) void bn_bwd_finalize(const float* __restrict__ partial, int nblocks, int C, double count,
                                                       float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ c12) {
    const int c = blockIdx.x;
    __shared__ double r1[256], r2[256];
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        s1 += (double)partial[((long)i * C + c) * 2 + 0];
        s2 += (double)partial[((long)i * C + c) * 2 + 1];
    }
    r1[threadIdx.x] = s1; r2[threadIdx.x] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        dbeta[c] += (float)r1[0];
        dgamma[c] += (float)r2[0];
        c12[2 * c + 0] = (float)(r1[0] / count);
        c12[2 * c + 1] = (float)(r2[0] / count);
    }
}

// dx = scale_c * (g' - c1 - xh*c2), element i has channel (i / F) % C; may run in place (dx == g)
__global__ void bn_bwd_apply(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ mean,
                             const float* __restrict__ invstd, const float* __restrict__ scale, const float* __restrict__ shift,
                             const float* __restrict__ c12, const uint8_t* __restrict__ mask, float inv_keep,
                             float* __restrict__ dx, long n, int C, int F, float* __restrict__ absmax) {
    const long stride = (long)gridDim.x * blockDim.x;
    float am = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int c = (int)((i / F) % C);
        const float xv = x[i];
        float gv = (xv * scale[c] + shift[c] > 0.f) ? g[i] : 0.f;
        if (mask) gv = mask[i] ? gv * inv_keep : 0.f;
        const float o = scale[c] * (gv - c12[2 * c] - (xv - mean[c]) * invstd[c] * c12[2 * c + 1]);
        dx[i] = o;
        am = fmaxf(am, fabsf(o));
    }
    if (absmax) {           // max |dx| for the consumer's power-of-two operand scale
        __shared__ float red[16];
        block_absmax_to(absmax, am, red);
    }
}

// The same for the (rows, C, F) activation layout with F % 4 == 0: one workgroup per (b,t) row, 16-byte accesses, the channel of a
// quad computed once (the generic kernel above spends two integer divisions per element and moves 4 bytes per access).
__global__ __launch_bounds__(256) void bn_bwd_apply_planes(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ c12,
                                                           float* __restrict__ dx, int C, int F, float* __restrict__ absmax) {
    __shared__ float k[64 * 6];
    float am = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
        k[c * 6 + 0] = mean[c]; k[c * 6 + 1] = invstd[c]; k[c * 6 + 2] = scale[c]; k[c * 6 + 3] = shift[c];
        k[c * 6 + 4] = c12[2 * c]; k[c * 6 + 5] = c12[2 * c + 1];
    }
    __syncthreads();
    const int qpp = F / 4, nq = C * qpp;                       // quads per plane, per row
    const long base = (long)blockIdx.x * C * F;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g + base);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x + base);
    f32x4* d4 = reinterpret_cast<f32x4*>(dx + base);
    for (int q0 = threadIdx.x; q0 < nq; q0 += 4 * 256) {        // 4 quads in flight per thread
        f32x4 gv[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = q0 + u * 256;
            if (q < nq) { gv[u] = g4[q]; xv[u] = x4[q]; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = q0 + u * 256;
            if (q >= nq) continue;
            const float* kc = k + (q / qpp) * 6;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gm = (xv[u][e] * kc[2] + kc[3] > 0.f) ? gv[u][e] : 0.f;
                o[e] = kc[2] * (gm - kc[4] - (xv[u][e] - kc[0]) * kc[1] * kc[5]);
                am = fmaxf(am, fabsf(o[e]));
            }
            d4[q] = o;
        }
    }
    if (absmax) {
        __shared__ float red[16];
        block_absmax_to(absmax, am, red);
    }
}

int a2s_bn_bwd_impl(hipStream_t st, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
                    const float* shift, const uint8_t* mask, float inv_keep, float* dgamma, float* dbeta, float* dx, float* partial,
                    float* c12, long rows, int C, int F, float* dx_absmax) {
    A2S_REQUIRE(g && x && mean && invstd && scale && shift && dgamma && dbeta && partial && c12, "bn_bwd: null tensor");
    if (dx_absmax && dx) {
        const hipError_t me = hipMemsetAsync(dx_absmax, 0, sizeof(float), st);
        A2S_REQUIRE(me == hipSuccess, "bn_bwd: hipMemsetAsync: %s", hipGetErrorString(me));
    }
    int nblocks;
    if (F > 1) {
        A2S_REQUIRE(!mask, "bn_bwd: dropout mask only supported on the (rows, C) layout");
        nblocks = (int)rows;
        hipLaunchKernelGGL(bn_bwd_reduce_planes, dim3(nblocks), dim3(256), 0, st, g, x, mean, invstd, scale, shift, partial, C, F);
    } else {
        const int rpb = 64;
        nblocks = a2s_cdiv(rows, rpb);
        hipLaunchKernelGGL(bn_bwd_reduce_cols, dim3(nblocks), dim3(256), 0, st, g, x, mean, invstd, scale, shift, mask, inv_keep, partial, rows, C, rpb);
    }
    A2S_CHECK_LAUNCH("bn_bwd_reduce");
    hipLaunchKernelGGL(bn_bwd_finalize, dim3(C), dim3(256), 0, st, partial, nblocks, C, (double)rows * F, dgamma, dbeta, c12);
    A2S_CHECK_LAUNCH("bn_bwd_finalize");
    if (!dx) return A2S_OK;            // statistics only: the input gradient is formed by the consumer (a2s_conv3x3_wgrad_bn)
    const long n = rows * C * F;
    if (F > 1 && F % 4 == 0 && C <= 64 && !mask && ((((uintptr_t)g | (uintptr_t)x | (uintptr_t)dx) & 15) == 0)) {
        hipLaunchKernelGGL(bn_bwd_apply_planes, dim3((unsigned)rows), dim3(256), 0, st, g, x, mean, invstd, scale, shift, c12, dx, C, F, dx_absmax);
        A2S_CHECK_LAUNCH("bn_bwd_apply_planes");
        return A2S_OK;
    }
    hipLaunchKernelGGL(bn_bwd_apply, dim3(min((long)4096, (n + 255) / 256)), dim3(256), 0, st, g, x, mean, invstd, scale, shift, c12, mask,
                       inv_keep, dx, n, C, F, dx_absmax);
    A2S_CHECK_LAUNCH("bn_bwd_apply");
    return A2S_OK;
}

// BatchNorm backward whose statistics partials were produced elsewhere (the data-gradient convolution's epilogue,
// a2s_conv3x3_dgrad_bnstats): finalize (dgamma, dbeta, c12) + apply.  (rows, C, F) layout only.
int a2s_bn_bwd_from_partial_impl(hipStream_t st, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
                                 const float* shift, float* dgamma, float* dbeta, float* dx, const float* partial, int nblocks, float* c12,
                                 long rows, int C, int F, float* dx_absmax) {
    A2S_REQUIRE(g && x && mean && invstd && scale && shift && dgamma && dbeta && partial && c12 && nblocks > 0, "bn_bwd_from_partial: null tensor");
    if (dx_absmax && dx) {
        const hipError_t me = hipMemsetAsync(dx_absmax, 0, sizeof(float), st);
        A2S_REQUIRE(me == hipSuccess, "bn_bwd_from_partial: hipMemsetAsync: %s", hipGetErrorString(me));
    }
    hipLaunchKernelGGL(bn_bwd_finalize, dim3(C), dim3(256), 0, st, partial, nblocks, C, (double)rows * F, dgamma, dbeta, c12);
    A2S_CHECK_LAUNCH("bn_bwd_finalize");
    if (!dx) return A2S_OK;
    const long n = rows * C * F;
    if (F > 1 && F % 4 == 0 && C <= 64 && ((((uintptr_t)g | (uintptr_t)x | (uintptr_t)dx) & 15) == 0)) {
        hipLaunchKernelGGL(bn_bwd_apply_planes, dim3((unsigned)rows), dim3(256), 0, st, g, x, mean, invstd, scale, shift, c12, dx, C, F, dx_absmax);
        A2S_CHECK_LAUNCH("bn_bwd_apply_planes");
        return A2S_OK;
    }
    hipLaunchKernelGGL(bn_bwd_apply, dim3(min((long)4096, (n + 255) / 256)), dim3(256), 0, st, g, x, mean, invstd, scale, shift, c12,
                       (const uint8_t*)nullptr, 1.f, dx, n, C, F, dx_absmax);
    A2S_CHECK_LAUNCH("bn_bwd_apply");
    return A2S_OK;
}

// ---- split form for synchronised BatchNorm (statistics exchanged between ranks by the host between the two calls)
// sums[c] = {s1, s2} of THIS rank (fixed-order double reduction of the partials)
__global__ __launch_bounds__(256) void bn_bwd_finalize_sums(const float* __restrict__ partial, int nblocks, int C, float* __restrict__ sums) {
    const int c = blockIdx.x;
    __shared__ double r1[256], r2[256];
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        s1 += (double)partial[((long)i * C + c) * 2 + 0];
        s2 += (double)partial[((long)i * C + c) * 2 + 1];
    }
    r1[threadIdx.x] = s1; r2[threadIdx.x] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { sums[2 * c] = (float)r1[0]; sums[2 * c + 1] = (float)r2[0]; }
}
// dgamma/dbeta += LOCAL sums (what torch.nn.SyncBatchNorm does: parameter gradients are rank-local, DDP averages them);
// c12 = GLOBAL sums / global count (the input gradient sees the statistics of the whole global batch)
__global__ void bn_bwd_c12_from_sums(const float* __restrict__ local, const float* __restrict__ global, double count, float* __restrict__ dgamma,
                                     float* __restrict__ dbeta, float* __restrict__ c12, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    dbeta[c] += local[2 * c]; dgamma[c] += local[2 * c + 1];
    c12[2 * c] = (float)((double)global[2 * c] / count); c12[2 * c + 1] = (float)((double)global[2 * c + 1] / count);
}

int a2s_bn_bwd_stats_impl(hipStream_t st, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
                          const float* shift, const uint8_t* mask, float inv_keep, float* partial, float* sums, long rows, int C, int F) {
    A2S_REQUIRE(g && x && mean && invstd && scale && shift && partial && sums, "bn_bwd_stats: null tensor");
    int nblocks;
    if (F > 1) {
        A2S_REQUIRE(!mask, "bn_bwd_stats: dropout mask only supported on the (rows, C) layout");
        nblocks = (int)rows;
        hipLaunchKernelGGL(bn_bwd_reduce_planes, dim3(nblocks), dim3(256), 0, st, g, x, mean, invstd, scale, shift, partial, C, F);
    } else {
        const int rpb = 64;
        nblocks = a2s_cdiv(rows, rpb);
        hipLaunchKernelGGL(bn_bwd_reduce_cols, dim3(nblocks), dim3(256), 0, st, g, x, mean, invstd, scale, shift, mask, inv_keep, partial, rows, C, rpb);
    }
    A2S_CHECK_LAUNCH("bn_bwd_reduce");
    hipLaunchKernelGGL(bn_bwd_finalize_sums, dim3(C), dim3(256), 0, st, partial, nblocks, C, sums);
    A2S_CHECK_LAUNCH("bn_bwd_finalize_sums");
    return A2S_OK;
}

int a2s_bn_bwd_apply_impl(hipStream_t st, const float* g, const float* x, const float* mean, const float* invstd, const float* scale,
                          const float* shift, const uint8_t* mask, float inv_keep, const float* sums_local, const float* sums_global,
                          double count_global, float* dgamma, float* dbeta, float* dx, float* c12, long rows, int C, int F) {
    A2S_REQUIRE(g && x && sums_local && sums_global && dgamma && dbeta && dx && c12, "bn_bwd_apply: null tensor");
    hipLaunchKernelGGL(bn_bwd_c12_from_sums, dim3(a2s_cdiv(C, 256)), dim3(256), 0, st, sums_local, sums_global, count_global, dgamma, dbeta, c12, C);
    A2S_CHECK_LAUNCH("bn_bwd_c12_from_sums");
    const long n = rows * C * F;
    hipLaunchKernelGGL(bn_bwd_apply, dim3(min((long)4096, (n + 255) / 256)), dim3(256), 0, st, g, x, mean, invstd, scale, shift, c12, mask,
                       inv_keep, dx, n, C, F, (float*)nullptr);
    A2S_CHECK_LAUNCH("bn_bwd_apply");
    return A2S_OK;
}

// The two halves again for statistics that were already reduced into per-block partials by the kernel that produced g (the data-gradient
// convolutions' and the Linear data gradient's epilogues): (1) partials -> this rank's sums; [host: all-reduce]; (2) dgamma / dbeta += local sums,
// c12 from the global sums -- no pass over (g, x) at all, the input gradient is then formed by the fused consumer (a2s_conv3x3_wgrad_bn_ranged).
int a2s_bn_bwd_sums_from_partial_impl(hipStream_t st, const float* partial, int nblocks, int C, float* sums) {
    A2S_REQUIRE(partial && sums && nblocks > 0 && C > 0, "bn_bwd_sums_from_partial: null tensor");
    hipLaunchKernelGGL(bn_bwd_finalize_sums, dim3(C), dim3(256), 0, st, partial, nblocks, C, sums);
    A2S_CHECK_LAUNCH("bn_bwd_finalize_sums");
    return A2S_OK;
}
int a2s_bn_bwd_c12_from_sums_impl(hipStream_t st, const float* sums_local, const float* sums_global, double count_global, float* dgamma, float* dbeta,
                                  float* c12, int C) {
    A2S_REQUIRE(sums_local && sums_global && dgamma && dbeta && c12 && count_global > 0, "bn_bwd_c12_from_sums: null tensor");
    hipLaunchKernelGGL(bn_bwd_c12_from_sums, dim3(a2s_cdiv(C, 256)), dim3(256), 0, st, sums_local, sums_global, count_global, dgamma, dbeta, c12, C);
    A2S_CHECK_LAUNCH("bn_bwd_c12_from_sums");
    return A2S_OK;
}

size_t a2s_bn_bwd_partial_floats_impl(long rows, int C, int F) {
    const long nblocks = F > 1 ? rows : (rows + 63) / 64;
    return (size_t)nblocks * C * 2;
}

// ---- not BatchNorm, but kept in this file: the weight scale of the tiled two-term convolution (a2s_conv3x3_impl).  As the only user of block_max
// in its translation unit the kernel compiles to a differently scheduled reduction loop (hipcc inlines a helper's last call by moving it, the
// others by cloning); beside the block_absmax_to users above it keeps the code it has always had.
// max |w| of a small tensor by ONE workgroup (the fp16 two-term path scales the weights by a power of two: their second term would
// otherwise sit in fp16's subnormal range)
__global__ __launch_bounds__(256) void absmax_small(const float* __restrict__ w, int n, float* __restrict__ out) {
    __shared__ float red[16];
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(w[i]));
    m = block_max(m, red);
    if (threadIdx.x == 0) *out = m;
}
void a2s_absmax_small_launch(hipStream_t st, const float* w, int n, float* out) {      // the caller checks the launch with its next one
    hipLaunchKernelGGL(absmax_small, dim3(1), dim3(256), 0, st, w, n, out);
}
