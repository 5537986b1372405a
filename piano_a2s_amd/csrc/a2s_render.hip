// Note synthesiser of the rendered synthetic corpus: the 16 kHz waveforms of a batch of clips from their render programs.
// One program = rows_per_clip rows of 8 int32 (floats bit-cast):
//     row 0      [n_samples, n_rows, attack, rel_len, rel_rate f32, gain f32, noise_level f32, noise_seed u32]
//     rows 1 ..  [onset, length, inc1 u32, amp f32, decay f32, g f32, n_harm, 0];  length <= 0, onset >= n_samples or onset < 0: padding, skipped
//     wave[n] = gain * sum_rows(ascending) amp * env(m) * sum_{h = 1 .. n_harm, h * inc1 < 2^31} g^(h-1) * sin(2 pi x_h(m))  +  noise_level * u(n)
//     m = n - onset in [0, length + rel_len);  x_h(m) = ((uint32)(m * h * inc1) >> 8) * 2^-24  (a wrapping 32-bit product: exact whatever the tiling)
//     env(m) = min(1, (m + 1) / attack) * exp(-m * decay) * (m >= length ? exp(-(m - length) * rel_rate) : 1)
//     u(n) = (hash32(noise_seed + n * 0x9E3779B9) >> 8) * 2^-23 - 1
// Grid (ceil(n_samples / 1024), B), 256 threads, four consecutive samples per thread.  The workgroup scans the clip's rows 256 at a time; the rows
// that overlap its 1024 samples go into an LDS list IN ROW ORDER (ballot + prefix count), every thread then walks the list with broadcast reads and
// adds each row's contribution to its four samples: rows ascending, harmonics ascending, the noise last.  One thread forms a sample's whole sum, so
// the result is the same bit for bit whatever the grid, the batch or the run.  No atomics, no waits between workgroups, plain stores only.
// Bounds: rows are read at [1, min(n_rows, rows_per_clip - 1)] of the clip's program; samples are written at [0, n_samples) of the clip's row of `wave`.
#include "a2s_internal.h"

#define RN_THREADS 256
#define RN_TILE (RN_THREADS * 4)

static long long rn_launches = 0;

__device__ __forceinline__ unsigned rn_hash32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__global__ __launch_bounds__(RN_THREADS) void render_notes(const int* __restrict__ programs, int rows_per_clip, int n_samples, float* __restrict__ wave,
                                                           long wave_bstride, int vec_ok) {
    __shared__ int4 list[RN_THREADS * 2];          // the tile's rows of one chunk, 32 bytes each, in row order
    __shared__ int wave_count[RN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int4* prog = reinterpret_cast<const int4*>(programs + (long)blockIdx.y * rows_per_clip * 8);
    const int4 h0 = prog[0], h1 = prog[1];
    const int clip_n = min(max(h0.x, 0), n_samples);                       // the clip's own length: samples behind it are zero
    const float inv_attack = 1.0f / (float)max(h0.z, 1);
    const int rel_len = max(h0.w, 0);
    const float rel_rate = __int_as_float(h1.x), gain = __int_as_float(h1.y), noise_level = __int_as_float(h1.z);
    const unsigned noise_seed = (unsigned)h1.w;
    const int t0 = blockIdx.x * RN_TILE, t1 = min(t0 + RN_TILE, clip_n);
    const int n0 = t0 + tid * 4;
    const int n_rows = t0 < clip_n ? min(max(h0.y, 0), rows_per_clip - 1) : 0;      // a tile behind the clip's own length scans nothing and writes zeros
    float acc[4] = {0.f, 0.f, 0.f, 0.f};

    for (int base = 1; base <= n_rows; base += RN_THREADS) {
        // ---- stage 1: which of this chunk's rows sound inside [t0, t1)
        const int r = base + tid;
        int4 a = {0, 0, 0, 0};
        bool live = false;
        if (r <= n_rows) {
            a = prog[2 * r];
            live = a.y > 0 && a.x >= 0 && a.x < clip_n && a.x < t1 && (long)a.x + a.y + rel_len > (long)t0;
        }
        const unsigned long long mask = __ballot(live);
        if (lane == 0) wave_count[wv] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < RN_THREADS / 64; ++w) {
            const int c = wave_count[w];
            before += w < wv ? c : 0;
            total += c;
        }
        if (live) {
            const int slot = before + __popcll(mask & ((1ull << lane) - 1ull));
            list[2 * slot] = a;
            list[2 * slot + 1] = prog[2 * r + 1];
        }
        __syncthreads();
        // ---- stage 2: every thread adds the listed rows to its four samples
        for (int i = 0; i < total; ++i) {
            const int4 ra = list[2 * i], rb = list[2 * i + 1];
            const int onset = ra.x, length = ra.y;
            const int span = (int)min((long)length + rel_len, (long)0x7fffffff - onset);       // m < span; never past what an int sample index can hold
            const int m0 = n0 - onset;
            if (m0 + 3 < 0 || m0 >= span) continue;
            const unsigned inc = (unsigned)ra.z;
            const float amp = __int_as_float(ra.w), decay = __int_as_float(rb.x), g = __int_as_float(rb.y);
            const int n_harm = min(rb.z, 16);
            float e[4], s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int m = m0 + j;
                float v = fminf(1.0f, (float)(m + 1) * inv_attack) * __expf(-(float)m * decay);
                if (m >= length) v *= __expf(-(float)(m - length) * rel_rate);
                e[j] = (m >= 0 && m < span) ? amp * v : 0.f;
            }
            unsigned hinc = 0;
            float gh = 1.0f;
            for (int h = 1; h <= n_harm; ++h) {
                hinc += inc;                                               // h * inc1: below 2^32 while the previous one was below 2^31 and so is inc1
                if (hinc >= 0x80000000u) break;                            // the partial would lie above the Nyquist frequency
                unsigned ph = (unsigned)m0 * hinc;                         // wrapping product = the phase in 2^-32 revolutions
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s[j] = fmaf(gh, __builtin_amdgcn_sinf((float)(ph >> 8) * 0x1p-24f), s[j]);      // the hardware sine takes revolutions
                    ph += hinc;
                }
                gh *= g;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(e[j], s[j], acc[j]);
        }
        __syncthreads();
    }

    if (n0 >= n_samples) return;
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + j;
        const unsigned hsh = rn_hash32(noise_seed + (unsigned)n * 0x9E3779B9u);
        const float u = (float)(hsh >> 8) * 0x1p-23f - 1.0f;
        out[j] = n < clip_n ? gain * acc[j] + noise_level * u : 0.f;
    }
    float* dst = wave + (long)blockIdx.y * wave_bstride + n0;
    if (vec_ok && n0 + 4 <= n_samples) {
        *reinterpret_cast<f32x4*>(dst) = f32x4{out[0], out[1], out[2], out[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n0 + j < n_samples) dst[j] = out[j];
    }
}

int a2s_render_notes_impl(hipStream_t st, const int* programs, int rows_per_clip, int n_samples, float* wave, long wave_bstride, int B) {
    A2S_REQUIRE(programs && wave, "render_notes: null programs or wave");
    A2S_REQUIRE(B >= 0 && rows_per_clip >= 1 && n_samples >= 1 && wave_bstride >= n_samples,
                "render_notes: needs B >= 0, rows_per_clip >= 1, n_samples >= 1 and a wave stride >= n_samples (got B = %d, rows_per_clip = %d, n_samples = %d, stride = %ld)",
                B, rows_per_clip, n_samples, wave_bstride);
    A2S_REQUIRE(B <= 65535, "render_notes: at most 65535 clips per call (got %d)", B);
    A2S_REQUIRE(((uintptr_t)programs & 15) == 0, "render_notes: the programs need 16-byte alignment");
    if (B == 0) return A2S_OK;
    const int vec_ok = (((uintptr_t)wave & 15) == 0 && wave_bstride % 4 == 0) ? 1 : 0;
    hipLaunchKernelGGL(render_notes, dim3(a2s_cdiv(n_samples, RN_TILE), B), dim3(RN_THREADS), 0, st, programs, rows_per_clip, n_samples, wave, wave_bstride, vec_ok);
    A2S_CHECK_LAUNCH("render_notes");
    __atomic_fetch_add(&rn_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}

int a2s_render_launches_impl(void) { return (int)__atomic_load_n(&rn_launches, __ATOMIC_RELAXED); }
