// Note-level scoring on the device (piano_a2s_amd/metrics.py: note_events is the definition this file restates): per pair of bar
// rows (target, prediction) the note counts of the two sides and the sizes of four multiset intersections.  Integers only: the host definition and
// this kernel agree exactly.
//
// note_match_pairs: one workgroup of 256 threads per pair; thread t owns the four consecutive token positions 4 t .. 4 t + 3 of a row of up to
// NM_CAP = 1024 tokens.  A side is parsed by the whole workgroup (parse_side), first the target, then the prediction:
//   1. the row is cut before its first <eos> (a block minimum over the positions of EOS-class ids);
//   2. ignored tokens (<pad>, <sos>, ids outside [0, V): never used as an index) are squeezed out by a block prefix sum of the keep flags;
//   3. ONE block prefix sum of the packed flags (NL | TAB << 11 | event << 22, unsigned: the totals are at most 1024, 1024 and 512, and 512 << 22 = 2^31) gives every token its
//      line, its count of TABs and its event number.  The NL that ends line l - 1 leaves the TAB count at the start of line l in line_tab[l],
//      and every separator (NL or TAB) leaves the event count at the start of the field it opens in field_ev[]: so the field index is a
//      difference of two prefix values and "first event of its field" is an equality -- every slot has one writer, no LDS atomics;
//   4. the line-time recurrence t = max(t_prev, min end[field]) is walked by thread 0 over the events, which lie in (line, field) order already;
//      the eight end[] values are its own words of LDS (indexed registers would be spilled to scratch memory);
//   5. every event that is a note (no rest, no continuation, field < 8) leaves key = onset << 25 | midi << 18 | ticks and its token id, every other
//      event the key NM_NONE.  Onset < 512 events x 221760 ticks < 2^27, midi < 2^7, ticks <= 221760 < 2^18.
// The intersections are then counted without a sort: with the notes of a bar in the tens, the target's note i is matched at a level iff
//   #{j < i : key_ref[j] == key_ref[i]}  <  #{j : key_hyp[j] == key_ref[i]}       (its rank among its equals is below the other side's count),
// which handles duplicates exactly; one loop over the two lists serves the four levels (the three coarser keys are shifts of the first, the
// spelled one adds the token id), every read of it a broadcast.  A bar at capacity (512 notes a side) costs 2048 LDS reads per thread.
// Output: 8 int32 per pair = n_ref, n_hyp, tp_pitch, tp_onset, tp_value, tp_spelled, flags (bit 0: the target row had events beyond the eighth
// spine, bit 1: the prediction row had), 0.  A pair with a row longer than NM_CAP (or with offsets that run backwards) is not read: its six counts
// are -1.  Bounds: ids at [off[p], off[p + 1]) of its side only, the three tables at ids checked against [0, V) only, out at [8 p, 8 p + 8).
#include "a2s_internal.h"

#define NM_THREADS 256
#define NM_CAP 1024
#define NM_PER 4                       // tokens per thread
#define NM_EVENTS (NM_CAP / 2)         // an event follows a DUR token: no two are adjacent
#define NM_FIELDS 8
#define NM_NONE 0xffffffffffffffffULL
#define NM_BIG 0x7fffffff
// class codes of the cls table (include/a2s.h: A2S_NOTE_CLS_*)
#define NM_TAB 1
#define NM_NL 2
#define NM_FERM 3
#define NM_CLOSE 4
#define NM_EOS 5
#define NM_IGNORE 6
// per compacted token: the class code above, or
#define NM_DUR 7
#define NM_PITCH 8
#define NM_REST (-2)                   // value of the midi table for the rest

static long long nm_launches = 0;

struct NmShared {
    int tok[NM_CAP];                   // the compacted row
    unsigned char cls[NM_CAP];
    int line_tab[NM_CAP + 1];          // TAB count at the start of line l
    int field_ev[NM_CAP + 1];          // event count at the start of the field behind the s-th separator (s = 0: the row's first field)
    int line_t[NM_CAP + 1];            // onset of line l (written for lines with events only)
    int ev_meta[NM_EVENTS];            // line | min(field, 8) << 11 | first-of-field << 15
    int ev_dur[NM_EVENTS];
    int end[NM_FIELDS];                // thread 0's: when the spine of field j is free again
    unsigned wave_part[NM_THREADS / 64];
    unsigned long long key[2][NM_EVENTS];
    int ntok[2][NM_EVENTS];
};

// sum of v over the lanes below this one in its wave (exclusive), and the wave's total.  Unsigned: the packed flags of step 3 reach 2^31.
__device__ __forceinline__ unsigned nm_wave_exclusive(unsigned v, int lane, unsigned* total) {
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    *total = __shfl(inc, 63, 64);
    return inc - v;
}

// exclusive prefix sum over the workgroup in thread order; *total: the sum over all threads.  Two barriers; part: one slot per wave.
__device__ __forceinline__ unsigned nm_block_exclusive(unsigned v, int tid, unsigned* part, unsigned* total) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned wtotal;
    const unsigned ex = nm_wave_exclusive(v, lane, &wtotal);
    __syncthreads();                   // (the previous use of part has been read)
    if (lane == 0) part[wave] = wtotal;
    __syncthreads();
    unsigned base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NM_THREADS / 64; ++w) {
        const unsigned p = part[w];
        base += w < wave ? p : 0u;
        all += p;
    }
    *total = all;
    return base + ex;
}

__device__ __forceinline__ int nm_block_min(int v, int tid, unsigned* part) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    __syncthreads();
    if ((tid & 63) == 0) part[tid >> 6] = (unsigned)v;
    __syncthreads();
    int m = (int)part[0];
#pragma unroll
    for (int w = 1; w < NM_THREADS / 64; ++w) m = min(m, (int)part[w]);
    return m;
}

// Parse the row ids[0 .. len) (len <= NM_CAP) into sh.key[side] / sh.ntok[side][0 .. n_events); returns n_events (uniform), *n_notes, *overflow.
__device__ __forceinline__ int nm_parse_side(NmShared& sh, int side, const int* __restrict__ ids, int len, const int* __restrict__ dur_ticks,
                             const int* __restrict__ midi, const int* __restrict__ cls, int V, int tid, int* n_notes, int* overflow) {
    const int p0 = tid * NM_PER;
    int id[NM_PER], c[NM_PER];
    int eos_at = NM_BIG;
#pragma unroll
    for (int e = 0; e < NM_PER; ++e) {
        const int p = p0 + e;
        id[e] = p < len ? ids[p] : -1;
        c[e] = NM_IGNORE;
        if (id[e] >= 0 && id[e] < V) {
            c[e] = cls[id[e]];
            if (dur_ticks[id[e]] > 0) c[e] = NM_DUR;
            else if (midi[id[e]] != -1) c[e] = NM_PITCH;
            if (c[e] == NM_EOS) eos_at = min(eos_at, p);
        }
    }
    eos_at = nm_block_min(eos_at, tid, sh.wave_part);
    // 2. squeeze the ignored tokens out
    int keep = 0;
#pragma unroll
    for (int e = 0; e < NM_PER; ++e) {
        if (p0 + e >= eos_at || c[e] == NM_IGNORE) c[e] = -1;
        keep += c[e] >= 0;
    }
    unsigned kept;
    int at = (int)nm_block_exclusive((unsigned)keep, tid, sh.wave_part, &kept);
    const int n = (int)kept;
#pragma unroll
    for (int e = 0; e < NM_PER; ++e)
        if (c[e] >= 0) {
            sh.tok[at] = id[e];
            sh.cls[at] = (unsigned char)c[e];
            ++at;
        }
    __syncthreads();
    // 3. lines, fields, events of the compacted row
    unsigned packed = 0;                                           // a row of 512 events makes the total 2^31: unsigned throughout
    int ev_flag[NM_PER];
#pragma unroll
    for (int e = 0; e < NM_PER; ++e) {
        const int q = p0 + e;
        c[e] = q < n ? sh.cls[q] : -1;
        ev_flag[e] = c[e] == NM_PITCH && q > 0 && sh.cls[q - 1] == NM_DUR;
        packed += (unsigned)(c[e] == NM_NL) | (unsigned)(c[e] == NM_TAB) << 11 | (unsigned)ev_flag[e] << 22;
    }
    unsigned total;
    unsigned run = nm_block_exclusive(packed, tid, sh.wave_part, &total);
    const int n_events = (int)(total >> 22);
    if (tid == 0) sh.line_tab[0] = sh.field_ev[0] = 0;
    unsigned pre[NM_PER];                                              // the exclusive prefix of every token of this thread
#pragma unroll
    for (int e = 0; e < NM_PER; ++e) {
        pre[e] = run;
        run += (unsigned)(c[e] == NM_NL) | (unsigned)(c[e] == NM_TAB) << 11 | (unsigned)ev_flag[e] << 22;
        const int nl = (int)(run & 0x7ff), tab = (int)((run >> 11) & 0x7ff), ev = (int)(run >> 22);          // inclusive
        if (c[e] == NM_NL) sh.line_tab[nl] = tab;
        if (c[e] == NM_NL || c[e] == NM_TAB) sh.field_ev[nl + tab] = ev;
    }
    __syncthreads();
    int over = 0;
#pragma unroll
    for (int e = 0; e < NM_PER; ++e) {
        if (!ev_flag[e]) continue;
        const int q = p0 + e;
        const int line = (int)(pre[e] & 0x7ff), tab = (int)((pre[e] >> 11) & 0x7ff), ev = (int)(pre[e] >> 22);
        const int field = tab - sh.line_tab[line];
        const int first = ev == sh.field_ev[line + tab];
        int nx = q + 1 < n ? sh.cls[q + 1] : -1;
        if (nx == NM_FERM) nx = q + 2 < n ? sh.cls[q + 2] : -1;
        const int tk = sh.tok[q], m = midi[tk];
        const bool note = m != NM_REST && nx != NM_CLOSE && field < NM_FIELDS;
        over |= field >= NM_FIELDS;
        const int ticks = dur_ticks[sh.tok[q - 1]];
        sh.ev_meta[ev] = line | min(field, NM_FIELDS) << 11 | first << 15;
        sh.ev_dur[ev] = ticks;
        // the onset is added once the line times are known
        sh.key[side][ev] = note ? ((unsigned long long)(m & 0x7f) << 18 | (unsigned long long)(ticks & 0x3ffff)) : NM_NONE;
        sh.ntok[side][ev] = tk;
    }
    *overflow = __syncthreads_or(over);                            // (also: the events are in LDS)
    // 4. the line times
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < NM_FIELDS; ++j) sh.end[j] = 0;
        int t = 0, e = 0;
        while (e < n_events) {
            const int line = sh.ev_meta[e] & 0x7ff;
            int m = NM_BIG, e1 = e;
            for (; e1 < n_events; ++e1) {
                const int meta = sh.ev_meta[e1];
                if ((meta & 0x7ff) != line) break;
                const int f = (meta >> 11) & 0xf;
                if ((meta >> 15) && f < NM_FIELDS) m = min(m, sh.end[f]);
            }
            if (m != NM_BIG) {
                t = max(t, m);
                for (int k = e; k < e1; ++k) {
                    const int meta = sh.ev_meta[k], f = (meta >> 11) & 0xf;
                    if ((meta >> 15) && f < NM_FIELDS) sh.end[f] = t + sh.ev_dur[k];
                }
            }
            sh.line_t[line] = t;
            e = e1;
        }
    }
    __syncthreads();
    // 5. onsets into the keys
    int notes = 0;
    for (int e = tid; e < n_events; e += NM_THREADS) {
        const unsigned long long k = sh.key[side][e];
        if (k != NM_NONE) {
            sh.key[side][e] = k | (unsigned long long)sh.line_t[sh.ev_meta[e] & 0x7ff] << 25;
            ++notes;
        }
    }
    unsigned n_all;
    nm_block_exclusive((unsigned)notes, tid, sh.wave_part, &n_all);
    *n_notes = (int)n_all;
    __syncthreads();
    return n_events;
}

__global__ __launch_bounds__(NM_THREADS) void note_match_pairs(const int* __restrict__ ref, const long long* __restrict__ ref_off,
                                                               const int* __restrict__ hyp, const long long* __restrict__ hyp_off,
                                                               const int* __restrict__ dur_ticks, const int* __restrict__ midi,
                                                               const int* __restrict__ cls, int V, int* __restrict__ out) {
    __shared__ NmShared sh;
    const int tid = threadIdx.x;
    const long p = blockIdx.x;
    const long long r0 = ref_off[p], h0 = hyp_off[p];
    const long long nr = ref_off[p + 1] - r0, nh = hyp_off[p + 1] - h0;
    int* o = out + p * 8;
    if (nr < 0 || nh < 0 || nr > NM_CAP || nh > NM_CAP || r0 < 0 || h0 < 0) {          // uniform: the rows are not read
        if (tid < 8) o[tid] = tid < 6 ? -1 : 0;
        return;
    }
    int n_ref, n_hyp, over_ref, over_hyp;
    const int er = nm_parse_side(sh, 0, ref + r0, (int)nr, dur_ticks, midi, cls, V, tid, &n_ref, &over_ref);
    const int eh = nm_parse_side(sh, 1, hyp + h0, (int)nh, dur_ticks, midi, cls, V, tid, &n_hyp, &over_hyp);
    // the target's note i is matched iff its rank among its equals is below the prediction's count of them
    int tp_pitch = 0, tp_onset = 0, tp_value = 0, tp_spelled = 0;
    for (int i = tid; i < er; i += NM_THREADS) {
        const unsigned long long k = sh.key[0][i];
        if (k == NM_NONE) continue;
        const int tk = sh.ntok[0][i];
        const unsigned long long k_on = k >> 18;
        const int k_pitch = (int)(k_on & 0x7f);
        int d_pitch = 0, d_onset = 0, d_value = 0, d_spelled = 0;             // (count on the other side) - (equals in front on this side)
        for (int j = 0; j < eh; ++j) {
            const unsigned long long q = sh.key[1][j];
            if (q == NM_NONE) continue;
            const bool on = (q >> 18) == k_on;
            d_pitch += (int)((q >> 18) & 0x7f) == k_pitch;
            d_onset += on;
            d_value += q == k;
            d_spelled += on && sh.ntok[1][j] == tk;
        }
        for (int j = 0; j < i; ++j) {
            const unsigned long long q = sh.key[0][j];
            if (q == NM_NONE) continue;
            const bool on = (q >> 18) == k_on;
            d_pitch -= (int)((q >> 18) & 0x7f) == k_pitch;
            d_onset -= on;
            d_value -= q == k;
            d_spelled -= on && sh.ntok[0][j] == tk;
        }
        tp_pitch += d_pitch > 0;
        tp_onset += d_onset > 0;
        tp_value += d_value > 0;
        tp_spelled += d_spelled > 0;
    }
    // four totals of at most 512 each in one sum: 10 bits would do, 16 are used
    unsigned lo, hi;
    nm_block_exclusive((unsigned)(tp_pitch | tp_onset << 16), tid, sh.wave_part, &lo);
    nm_block_exclusive((unsigned)(tp_value | tp_spelled << 16), tid, sh.wave_part, &hi);
    if (tid < 8) {
        int v = 0;
        if (tid == 0) v = n_ref;
        if (tid == 1) v = n_hyp;
        if (tid == 2) v = (int)(lo & 0xffff);
        if (tid == 3) v = (int)(lo >> 16);
        if (tid == 4) v = (int)(hi & 0xffff);
        if (tid == 5) v = (int)(hi >> 16);
        if (tid == 6) v = (over_ref ? 1 : 0) | (over_hyp ? 2 : 0);
        o[tid] = v;
    }
}

int a2s_note_match_max_len_impl(void) { return NM_CAP; }
long a2s_note_match_launches_impl(void) { return (long)__atomic_load_n(&nm_launches, __ATOMIC_RELAXED); }

int a2s_note_match_impl(hipStream_t st, const int* ref, const long long* ref_off, const int* hyp, const long long* hyp_off, int n_pairs,
                        const int* dur_ticks, const int* midi, const int* cls, int V, int* out) {
    A2S_REQUIRE(n_pairs >= 0, "note_match: n_pairs = %d", n_pairs);
    A2S_REQUIRE(V >= 1, "note_match: a vocabulary of %d symbols", V);
    A2S_REQUIRE(ref && hyp && ref_off && hyp_off && out, "note_match: null ids, offsets or result");
    A2S_REQUIRE(dur_ticks && midi && cls, "note_match: null vocabulary table");
    if (n_pairs == 0) return A2S_OK;
    hipLaunchKernelGGL(note_match_pairs, dim3(n_pairs), dim3(NM_THREADS), 0, st, ref, ref_off, hyp, hyp_off, dur_ticks, midi, cls, V, out);
    A2S_CHECK_LAUNCH("note_match_pairs");
    __atomic_fetch_add(&nm_launches, 1LL, __ATOMIC_RELAXED);
    return A2S_OK;
}
