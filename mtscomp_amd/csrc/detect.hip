// Threshold-crossing peak detection on filtered rows (mts_detect, mts_dev_detect).
//
// The filter is k_decimate with q = 1 (decimate.hip) into a float32 workspace z of file rows [ws_row0, ws_row0 + ws_rows) x n_cols;
// the kernels here work on that workspace, slab after slab (api.hip: detect_run):
//   k_row_median    reference = 1: the exact median of every row (np.sort's order, NaN last; the mean 0.5f * (a + b) of the two middle
//                   values for an even n; NaN when the row holds one) subtracted in place, one rounding per value.  One wave per
//                   row: the row's order keys are sorted by a bitonic network in LDS (padded with the key of a NaN, which is last).
//   k_detect_mask   one wave per (row, 64 column positions): v = -z, z or |z|; a lane whose v > threshold walks its neighbourhood
//                   (|dt| <= R rows, |dj| <= S positions, inside the workspace = inside the recording), nearest rows first, and
//                   leaves at the first neighbour that beats it: v' > v, or v' == v at an earlier (t, j).  A ballot gives the
//                   64-bit word of the event bitmap, stored by lane 0.
//   k_detect_count / k_detect_scan / k_detect_emit   the bitmap is row-major, which is the (t, j) order of the output: popcounts per
//                   block of DET_BLOCK_WORDS words, an exclusive scan of the blocks by one workgroup that continues from the events
//                   counted so far (*total), then every block writes its events in bit order.  Events at positions >= max_events
//                   are counted and not written.  No atomics: the same bytes whatever ran when.
#include "common.h"

namespace mts {

namespace {

constexpr int DET_WAVES = 4;
constexpr int DET_THREADS = 64 * DET_WAVES;
constexpr int DET_WORDS_PER_THREAD = 4;
constexpr int DET_BLOCK_WORDS = DET_THREADS * DET_WORDS_PER_THREAD;
constexpr u32 KEY_NAN = 0xffffffffu;

// a key whose unsigned order is np.sort's order of floats: NaN (either sign) last, above +inf
__device__ __forceinline__ u32 order_key(float x)
{
    const u32 b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return KEY_NAN;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(u32 k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float det_value(float z, int sign) { return sign == 0 ? -z : sign == 1 ? z : fabsf(z); }

}  // namespace

// P: the power of two >= max(n, 2) the network sorts (uniform); rows past n_rows sort padding and write nothing
__global__ __launch_bounds__(DET_THREADS) void k_row_median(float *__restrict__ y, long n_rows, int n, int P)
{
#pragma clang fp contract(off)
    __shared__ u32 keys[DET_WAVES][MTS_DETECT_MAX_REF_COLS];
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * DET_WAVES + w;
    const bool live = row < n_rows;
    float *p = y + (u64)(live ? row : 0) * (u64)n;
    u32 *s = keys[w];
    for (int i = lane; i < P; i += 64) s[i] = (live && i < n) ? order_key(p[i]) : KEY_NAN;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < (P >> 1); i += 64) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const u32 a = s[lo], b = s[hi];
                const bool up = (lo & k) == 0;
                if ((a > b) == up) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
    }
    if (!live) return;
    float m;
    if (s[n - 1] == KEY_NAN) m = __builtin_nanf("");
    else {
        const float a = key_value(s[(n - 1) >> 1]);
        if (n & 1) m = a;
        else {
            const float sum = a + key_value(s[n >> 1]);
            m = 0.5f * sum;
        }
    }
    for (int i = lane; i < n; i += 64) p[i] = p[i] - m;
}

// wave g of the launch: word g % W of row s0 + g / W; bitmap[g]
__global__ __launch_bounds__(DET_THREADS) void k_detect_mask(const float *__restrict__ z, long ws_row0, long ws_rows, int n,
                                                            const float *__restrict__ thr, int sign, int R, int S, long s0, u64 n_words,
                                                            int W, u64 *__restrict__ bitmap)
{
    const int lane = threadIdx.x & 63;
    const u64 g = (u64)blockIdx.x * DET_WAVES + (threadIdx.x >> 6);
    if (g >= n_words) return;                                      // (wave-uniform)
    const long t = s0 + (long)(g / (u64)W);
    const int j = (int)(g % (u64)W) * 64 + lane;
    bool ev = false;
    if (j < n) {
        const float *zr = z + (u64)(t - ws_row0) * (u64)n;
        const float v = det_value(zr[j], sign);
        if (v > thr[j]) {
            ev = true;
            const int j_lo = j - S > 0 ? j - S : 0, j_hi = j + S < n - 1 ? j + S : n - 1;
            for (int jj = j_lo; jj <= j_hi; jj++) {                // the row itself: an equal value at a lower position wins
                const float v2 = det_value(zr[jj], sign);
                if (v2 > v || (v2 == v && jj < j)) { ev = false; break; }
            }
            for (int d = 1; d <= R && ev; d++) {
                if (t - d >= ws_row0) {                            // an earlier row: an equal value wins
                    const float *q = zr - (u64)d * (u64)n;
                    for (int jj = j_lo; jj <= j_hi; jj++)
                        if (det_value(q[jj], sign) >= v) { ev = false; break; }
                }
                if (ev && t + d < ws_row0 + ws_rows) {
                    const float *q = zr + (u64)d * (u64)n;
                    for (int jj = j_lo; jj <= j_hi; jj++)
                        if (det_value(q[jj], sign) > v) { ev = false; break; }
                }
            }
        }
    }
    const u64 m = ballot64(ev);
    if (lane == 0) bitmap[g] = m;
}

namespace {

// the popcount of the thread's words and its exclusive prefix in the workgroup; -> the workgroup's sum
__device__ __forceinline__ u32 block_prefix(u32 mine, u32 *wave_sums, u32 *before)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u32 inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sums[w] = inc;
    __syncthreads();
    u32 base = 0, all = 0;
#pragma unroll
    for (int i = 0; i < DET_WAVES; i++) { if (i < w) base += wave_sums[i]; all += wave_sums[i]; }
    *before = base + inc - mine;
    return all;
}

}  // namespace

__global__ __launch_bounds__(DET_THREADS) void k_detect_count(const u64 *__restrict__ bitmap, u64 n_words, u32 *__restrict__ counts)
{
    __shared__ u32 wave_sums[DET_WAVES];
    const u64 w0 = (u64)blockIdx.x * DET_BLOCK_WORDS + (u64)threadIdx.x * DET_WORDS_PER_THREAD;
    u32 mine = 0;
#pragma unroll
    for (int e = 0; e < DET_WORDS_PER_THREAD; e++)
        if (w0 + e < n_words) mine += (u32)__popcll(bitmap[w0 + e]);
    u32 before;
    const u32 all = block_prefix(mine, wave_sums, &before);
    if (threadIdx.x == 0) counts[blockIdx.x] = all;
}

// one workgroup: offsets[b] = *total + the counts of the blocks before b; *total += all of them
__global__ __launch_bounds__(DET_THREADS) void k_detect_scan(const u32 *__restrict__ counts, long n_blocks, u64 *__restrict__ offsets,
                                                            u64 *__restrict__ total)
{
    __shared__ u64 part[DET_THREADS];
    __shared__ u64 base;
    const long per = (n_blocks + DET_THREADS - 1) / DET_THREADS;
    const long b0 = (long)threadIdx.x * per, b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    u64 sum = 0;
    for (long b = b0; b < b1; b++) sum += counts[b];
    part[threadIdx.x] = sum;
    if (threadIdx.x == 0) base = *total;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 run = base;
        for (int i = 0; i < DET_THREADS; i++) { const u64 c = part[i]; part[i] = run; run += c; }
        *total = run;
    }
    __syncthreads();
    u64 run = part[threadIdx.x];
    for (long b = b0; b < b1; b++) { offsets[b] = run; run += counts[b]; }
}

__global__ __launch_bounds__(DET_THREADS) void k_detect_emit(const u64 *__restrict__ bitmap, u64 n_words, const u64 *__restrict__ offsets,
                                                            const float *__restrict__ z, long ws_row0, int n, int W, long s0, u64 max_events,
                                                            long *__restrict__ out_row, int *__restrict__ out_pos, float *__restrict__ out_amp)
{
    __shared__ u32 wave_sums[DET_WAVES];
    const u64 w0 = (u64)blockIdx.x * DET_BLOCK_WORDS + (u64)threadIdx.x * DET_WORDS_PER_THREAD;
    u64 words[DET_WORDS_PER_THREAD];
    u32 mine = 0;
#pragma unroll
    for (int e = 0; e < DET_WORDS_PER_THREAD; e++) {
        words[e] = w0 + e < n_words ? bitmap[w0 + e] : 0;
        mine += (u32)__popcll(words[e]);
    }
    u32 before;
    block_prefix(mine, wave_sums, &before);
    u64 pos = offsets[blockIdx.x] + before;
#pragma unroll
    for (int e = 0; e < DET_WORDS_PER_THREAD; e++) {
        u64 m = words[e];
        if (!m) continue;
        const long t = s0 + (long)((w0 + e) / (u64)W);
        const int j0 = (int)((w0 + e) % (u64)W) * 64;
        while (m) {
            const int j = j0 + __builtin_ctzll(m);
            m &= m - 1;
            if (pos < max_events) {
                out_row[pos] = t;
                out_pos[pos] = j;
                out_amp[pos] = z[(u64)(t - ws_row0) * (u64)n + (u64)j];
            }
            pos++;
        }
    }
}

int launch_row_median(hipStream_t st, float *d_y, long n_rows, int n_cols)
{
    if (n_rows <= 0) return MTS_OK;
    if (n_cols < 1 || n_cols > MTS_DETECT_MAX_REF_COLS) { set_error("detect: a median over %d columns (1 .. %d)", n_cols, MTS_DETECT_MAX_REF_COLS); return MTS_E_ARG; }
    int P = 2;
    while (P < n_cols) P <<= 1;
    const long nb = (n_rows + DET_WAVES - 1) / DET_WAVES;
    if (nb > 0x7fffffffl) { set_error("detect: too many rows in one launch"); return MTS_E_ARG; }
    hipLaunchKernelGGL(k_row_median, dim3((unsigned)nb), dim3(DET_THREADS), 0, st, d_y, n_rows, n_cols, P);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

long detect_bitmap_words(long n_rows, int n_cols) { return n_rows * (long)((n_cols + 63) / 64); }
long detect_blocks(long n_words) { return (n_words + DET_BLOCK_WORDS - 1) / DET_BLOCK_WORDS; }

int launch_detect_mask(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, const float *d_thr, int sign, int exclude_rows,
                       int exclude_cols, long s0, long s1, u64 *d_bitmap)
{
    if (s1 <= s0) return MTS_OK;
    if (s0 < ws_row0 || s1 > ws_row0 + ws_rows) { set_error("detect: rows outside the workspace"); return MTS_E_ARG; }
    const long n_words = detect_bitmap_words(s1 - s0, n_cols);
    const long nb = (n_words + DET_WAVES - 1) / DET_WAVES;
    if (nb > 0x7fffffffl) { set_error("detect: too many rows in one launch"); return MTS_E_ARG; }
    hipLaunchKernelGGL(k_detect_mask, dim3((unsigned)nb), dim3(DET_THREADS), 0, st, d_z, ws_row0, ws_rows, n_cols, d_thr, sign, exclude_rows,
                       exclude_cols, s0, (u64)n_words, (n_cols + 63) / 64, d_bitmap);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

// k_detect_count and k_detect_scan know nothing of what a bit stands for: the offsets of any bitmap's blocks (tmatch.hip emits by them)
int launch_bitmap_offsets(hipStream_t st, const u64 *d_bitmap, long n_words, u32 *d_counts, u64 *d_offsets, u64 *d_total)
{
    static_assert(DETECT_BLOCK_WORDS == DET_BLOCK_WORDS, "common.h states the block of the bitmap kernels");
    if (n_words <= 0) return MTS_OK;
    const long nb = detect_blocks(n_words);
    if (nb > 0x7fffffffl) { set_error("detect: too many rows in one launch"); return MTS_E_ARG; }
    hipLaunchKernelGGL(k_detect_count, dim3((unsigned)nb), dim3(DET_THREADS), 0, st, d_bitmap, (u64)n_words, d_counts);
    hipLaunchKernelGGL(k_detect_scan, dim3(1), dim3(DET_THREADS), 0, st, d_counts, nb, d_offsets, d_total);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

int launch_detect_emit(hipStream_t st, const u64 *d_bitmap, long n_words, u32 *d_counts, u64 *d_offsets, u64 *d_total, const float *d_z,
                       long ws_row0, int n_cols, long s0, long max_events, long *d_row, int *d_pos, float *d_amp)
{
    if (n_words <= 0) return MTS_OK;
    const long nb = detect_blocks(n_words);
    if (nb > 0x7fffffffl) { set_error("detect: too many rows in one launch"); return MTS_E_ARG; }
    hipLaunchKernelGGL(k_detect_count, dim3((unsigned)nb), dim3(DET_THREADS), 0, st, d_bitmap, (u64)n_words, d_counts);
    hipLaunchKernelGGL(k_detect_scan, dim3(1), dim3(DET_THREADS), 0, st, d_counts, nb, d_offsets, d_total);
    hipLaunchKernelGGL(k_detect_emit, dim3((unsigned)nb), dim3(DET_THREADS), 0, st, d_bitmap, (u64)n_words, d_offsets, d_z, ws_row0, n_cols,
                       (n_cols + 63) / 64, s0, (u64)max_events, d_row, d_pos, d_amp);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace mts
