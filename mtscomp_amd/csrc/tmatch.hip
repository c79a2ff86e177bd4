// Template-matching events on a slab of template scores (mts_match_templates, mts_dev_match_templates).
//
// launch_correlate (correlate.hip) has written score[t, k] of the file rows [sc_row0, sc_row0 + sc_rows) x n_out into a device slab --
// every row of the recording within exclude_rows of the rows [s0, s1) that the slab owns (reduce.hip: tmatch_run).  The kernels here
// pick the events of the owned rows where the scores lie:
//   k_tmatch_best   one wave per score row: lanes stride over the n_out scores 64 at a time (coalesced 256-byte reads), each keeps
//                   (max, first index) over its ascending indices with a strict >, NaN skipped; the wave combines by __shfl_xor on
//                   (value descending, index ascending).  best[row] = the row's largest score that is not a NaN (its own bits: of
//                   -0 and +0 the first), arg[row] = the first template that attains it; a row of NaNs gets NaN and -1.
//   k_tmatch_mask   one lane per owned row, 64 consecutive rows per wave: a lane whose best > threshold[arg] walks d = 1 .. R, nearest
//                   first, the earlier row before the later one, and leaves at the first neighbour that beats it: best' >= best
//                   earlier, best' > best later (a row of NaNs beats nothing: its NaN compares false).  Rows outside the slab do
//                   not exist: the slab holds every row of the recording within R.  A ballot gives the wave's 64-bit word of a
//                   row-ordered bitmap.
//   k_tmatch_emit   after k_detect_count / k_detect_scan (detect.hip, bitmap-generic: launch_bitmap_offsets): every block of
//                   DETECT_BLOCK_WORDS words writes (row, arg[row], best[row]) of its set bits in bit order from its offset on.  Events
//                   at positions >= max_events are counted and not written.
// The bitmap's order is the output's order: no sort, no atomics -- the same bytes whatever ran when.
#include "common.h"

namespace mts {

namespace {

constexpr int TM_WAVES = 4;
constexpr int TM_THREADS = 64 * TM_WAVES;
constexpr int TM_WORDS_PER_THREAD = DETECT_BLOCK_WORDS / TM_THREADS;
static_assert(TM_WORDS_PER_THREAD * TM_THREADS == DETECT_BLOCK_WORDS, "a block of the bitmap is a whole number of words per thread");
constexpr u32 TM_NAN = 0x7fc00000u;

}  // namespace

__global__ __launch_bounds__(TM_THREADS) void k_tmatch_best(const float *__restrict__ score, long n_rows, int n_out, float *__restrict__ best,
                                                           int *__restrict__ arg)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * TM_WAVES + (threadIdx.x >> 6);
    if (row >= n_rows) return;                                     // (wave-uniform)
    const float *s = score + (u64)row * (u64)n_out;
    float v = 0.f;
    int k = -1;
    for (int i = lane; i < n_out; i += 64) {
        const float x = s[i];
        if (x == x && (k < 0 || x > v)) { v = x; k = i; }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int ok = __shfl_xor(k, d, 64);
        if (ok >= 0 && (k < 0 || ov > v || (ov == v && ok < k))) { v = ov; k = ok; }
    }
    if (lane == 0) {
        best[row] = k >= 0 ? v : __uint_as_float(TM_NAN);
        arg[row] = k;
    }
}

// wave g of the launch: rows s0 + 64 g .. s0 + 64 g + 63 of [s0, s1); bitmap[g].  best / arg: of file rows [sc_row0, sc_row0 + sc_rows)
__global__ __launch_bounds__(TM_THREADS) void k_tmatch_mask(const float *__restrict__ best, const int *__restrict__ arg, long sc_row0, long sc_rows,
                                                           const float *__restrict__ thr, int R, long s0, long s1, u64 n_words,
                                                           u64 *__restrict__ bitmap)
{
    const int lane = threadIdx.x & 63;
    const u64 g = (u64)blockIdx.x * TM_WAVES + (threadIdx.x >> 6);
    if (g >= n_words) return;                                      // (wave-uniform)
    const long t = s0 + (long)(g * 64) + lane;
    bool ev = false;
    if (t < s1) {
        const long i = t - sc_row0;
        const int k = arg[i];
        const float v = best[i];
        if (k >= 0 && v > thr[k]) {
            ev = true;
            for (int d = 1; d <= R && ev; d++) {
                if (i - d >= 0 && best[i - d] >= v) ev = false;           // an earlier row: an equal value wins
                else if (i + d < sc_rows && best[i + d] > v) ev = false;
            }
        }
    }
    const u64 m = ballot64(ev);
    if (lane == 0) bitmap[g] = m;
}

__global__ __launch_bounds__(TM_THREADS) void k_tmatch_emit(const u64 *__restrict__ bitmap, u64 n_words, const u64 *__restrict__ offsets,
                                                           const float *__restrict__ best, const int *__restrict__ arg, long sc_row0, long s0,
                                                           u64 max_events, long *__restrict__ out_row, int *__restrict__ out_tpl,
                                                           float *__restrict__ out_score)
{
    __shared__ u32 wave_sums[TM_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 w0 = (u64)blockIdx.x * DETECT_BLOCK_WORDS + (u64)threadIdx.x * TM_WORDS_PER_THREAD;
    u64 words[TM_WORDS_PER_THREAD];
    u32 mine = 0;
#pragma unroll
    for (int e = 0; e < TM_WORDS_PER_THREAD; e++) {
        words[e] = w0 + e < n_words ? bitmap[w0 + e] : 0;
        mine += (u32)__popcll(words[e]);
    }
    // the exclusive prefix of the thread's popcount in the workgroup
    u32 inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sums[w] = inc;
    __syncthreads();
    u32 base = 0;
#pragma unroll
    for (int i = 0; i < TM_WAVES; i++) if (i < w) base += wave_sums[i];
    u64 pos = offsets[blockIdx.x] + base + inc - mine;
#pragma unroll
    for (int e = 0; e < TM_WORDS_PER_THREAD; e++) {
        u64 m = words[e];
        while (m) {
            const long t = s0 + (long)((w0 + e) * 64) + __builtin_ctzll(m);
            m &= m - 1;
            if (pos < max_events) {
                out_row[pos] = t;
                out_tpl[pos] = arg[t - sc_row0];
                out_score[pos] = best[t - sc_row0];
            }
            pos++;
        }
    }
}

long tmatch_bitmap_words(long n_rows) { return (n_rows + 63) / 64; }

int launch_tmatch_best(hipStream_t st, const float *d_score, long n_rows, int n_out, float *d_best, int *d_arg)
{
    if (n_rows <= 0) return MTS_OK;
    if (n_out < 1 || n_out > CORRELATE_MAX_OUT) { set_error("match_templates: %d templates (1 .. %d)", n_out, CORRELATE_MAX_OUT); return MTS_E_ARG; }
    const long nb = (n_rows + TM_WAVES - 1) / TM_WAVES;
    if (nb > 0x7fffffffl) { set_error("match_templates: too many rows in one launch"); return MTS_E_ARG; }
    hipLaunchKernelGGL(k_tmatch_best, dim3((unsigned)nb), dim3(TM_THREADS), 0, st, d_score, n_rows, n_out, d_best, d_arg);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

int launch_tmatch_mask(hipStream_t st, const float *d_best, const int *d_arg, long sc_row0, long sc_rows, const float *d_thr, int exclude_rows,
                       long s0, long s1, u64 *d_bitmap)
{
    if (s1 <= s0) return MTS_OK;
    if (s0 < sc_row0 || s1 > sc_row0 + sc_rows || exclude_rows < 0) { set_error("match_templates: rows outside the score slab"); return MTS_E_ARG; }
    const long n_words = tmatch_bitmap_words(s1 - s0);
    const long nb = (n_words + TM_WAVES - 1) / TM_WAVES;
    if (nb > 0x7fffffffl) { set_error("match_templates: too many rows in one launch"); return MTS_E_ARG; }
    hipLaunchKernelGGL(k_tmatch_mask, dim3((unsigned)nb), dim3(TM_THREADS), 0, st, d_best, d_arg, sc_row0, sc_rows, d_thr, exclude_rows, s0, s1,
                       (u64)n_words, d_bitmap);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

int launch_tmatch_emit(hipStream_t st, const u64 *d_bitmap, long n_words, u32 *d_counts, u64 *d_offsets, u64 *d_total, const float *d_best,
                       const int *d_arg, long sc_row0, long s0, long max_events, long *d_row, int *d_tpl, float *d_score)
{
    if (n_words <= 0) return MTS_OK;
    const int rc = launch_bitmap_offsets(st, d_bitmap, n_words, d_counts, d_offsets, d_total);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tmatch_emit, dim3((unsigned)detect_blocks(n_words)), dim3(TM_THREADS), 0, st, d_bitmap, (u64)n_words, d_offsets, d_best,
                       d_arg, sc_row0, s0, (u64)max_events, d_row, d_tpl, d_score);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace mts
