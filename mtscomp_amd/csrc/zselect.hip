// One round of a most-significant-digit radix select over a dense float32 slab of the filtered signal z (mts_filtered_rank_hist,
// mts_dev_filtered_rank_hist).
//
// Input: d_y, the rows [s0, s1) of z as the filter stage left them (C order, n_cols items per row, slab row 0 = file row s0).  The
// order keys, the selectors and the outputs are mts_rank_hist's for a float32 recording (include/mtscomp_hip.h).
//   k_zrank_hist  needs no table: workgroup (b, g) owns the rows [s0 + b * H, min(s1, s0 + (b + 1) * H)) (H: ZSEL_BLOCK_ROWS unless the
//                 caller says otherwise) of the columns [64 g, 64 g + 64), and walks the rows in segments that end at the window
//                 boundaries of the grid (zrank_block_rows, zrank_segment: reduce_plan.h, swept on the CPU).  A slab of 256 MiB is some
//                 tens of row blocks: the column groups in the grid's y are what fills the CUs.  Per segment the 64 lanes of a wave take
//                 their 64 consecutive columns of a row -- one 256-byte load, no gather --, the ZSEL_WAVES waves every ZSEL_WAVES-th row.
//                 The counting is k_rank_hist's (select.hip): a candidate increments the 32-bit LDS counter
//                 hist[selector][digit][lane], lane l on bank l mod 32 whatever the digit, so neither random data nor a constant column
//                 gives a bank conflict; 2 x 256 x 64 x 4 B = 128 KiB of the CU's 160, one workgroup of 1024 threads per CU.  At the end of the segment the non-zero counters go to the cell's histogram in HBM
//                 with integer atomicAdd and the smallest / largest candidate key with integer atomicMin / atomicMax.  Integers only:
//                 the outputs do not depend on the order of blocks, slabs, pieces or calls.
#include "common.h"
#include "reduce_plan.h"

namespace mts {

namespace {

constexpr int ZSEL_WAVES = 16;           // one workgroup of 1024 threads per CU (the LDS allows no second one)
constexpr int ZSEL_UNROLL = 4;           // rows of one wave in flight
constexpr int ZSEL_S = MTS_RANK_SELECTORS;
constexpr int ZSEL_BINS = 1 << MTS_RANK_BITS;
constexpr int ZSEL_LDS_HIST = ZSEL_S * ZSEL_BINS * 64 * 4;
constexpr int ZSEL_LDS = ZSEL_LDS_HIST + 2 * ZSEL_S * 64 * 8;
static_assert(MTS_RANK_BITS == 8 && ZSEL_S == 2, "the LDS budget and the flush are written for two selectors of 8-bit digits");

// the key maps of select.hip for float32 items (that file keeps its own): -0 is +0, every NaN is all ones, negative numbers reversed
// below the positive ones
__device__ __forceinline__ u32 zkey32(float x)
{
    if (x != x) return ~0u;
    if (x == 0.0f) return 0x80000000u;
    const u32 b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ u64 zkey64(double x)
{
    if (x != x) return ~0ull;
    if (x == 0.0) return 0x8000000000000000ull;
    const u64 b = (u64)__double_as_longlong(x);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}

// MODE 0: the float32 item.  MODE 1: double(x) - c.  MODE 2: |double(x) - c|.
template <typename K, int MODE> __device__ __forceinline__ K zrank_key(float x, double c)
{
    if constexpr (MODE == 0) return zkey32(x);
    else {
        const double d = (double)x - c;
        return zkey64(MODE == 2 ? __builtin_fabs(d) : d);
    }
}

}  // namespace

template <typename K, int MODE>
__global__ __launch_bounds__(64 * ZSEL_WAVES) void k_zrank_hist(const float *__restrict__ y, long s0, long s1, long H, int n_cols, long row_begin,
                                                                long window_rows, const double *__restrict__ center,
                                                                const u64 *__restrict__ sel_prefix, const int *__restrict__ sel_shift,
                                                                u32 *__restrict__ hist, unsigned long long *__restrict__ kmin,
                                                                unsigned long long *__restrict__ kmax)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    u32 *lh = (u32 *)smem;                                     // [selector][digit][lane]
    K *lmin = (K *)(smem + ZSEL_LDS_HIST), *lmax = lmin + ZSEL_S * 64;
    constexpr int KB = 8 * (int)sizeof(K);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const ZrankSeg blk = zrank_block_rows(s0, s1, H, (long)blockIdx.x);
    const int g0 = 64 * (int)blockIdx.y;
    for (long r0 = blk.r0; r0 < blk.r1;) {                     // (uniform: every thread walks the same segments)
        const ZrankSeg seg = zrank_segment(r0, blk.r1, row_begin, window_rows);
        const u64 win = (u64)seg.win;
        const float *base = y + (u64)(seg.r0 - s0) * (u64)n_cols;
        const long n = seg.r1 - seg.r0;
        for (int e = threadIdx.x; e < ZSEL_S * ZSEL_BINS * 64; e += 64 * ZSEL_WAVES) lh[e] = 0;
        if (threadIdx.x < ZSEL_S * 64) { lmin[threadIdx.x] = (K)~(K)0; lmax[threadIdx.x] = 0; }
        __syncthreads();
        const int j = g0 + lane;
        if (j < n_cols) {
            bool act[ZSEL_S];
            int sh[ZSEL_S], hs[ZSEL_S];
            K pf[ZSEL_S], mn[ZSEL_S], mx[ZSEL_S];
            double c = 0.0;
            if constexpr (MODE != 0) c = center[win * (u64)n_cols + (u64)j];
#pragma unroll
            for (int s = 0; s < ZSEL_S; s++) {
                const u64 o = (win * ZSEL_S + s) * (u64)n_cols + (u64)j;
                const int v = sel_shift[o];
                mn[s] = (K)~(K)0; mx[s] = 0;
                act[s] = v >= 0;
                sh[s] = act[s] ? v : 0;
                // every bit above the digit is prefix; a digit that reaches the top of the key has none (prefix 0, nothing to shift by)
                if (sh[s] + MTS_RANK_BITS >= KB) { hs[s] = KB - 1; pf[s] = 0; }
                else { hs[s] = sh[s] + MTS_RANK_BITS; pf[s] = (K)sel_prefix[o]; }
            }
            auto count = [&](float x) {
                const K key = zrank_key<K, MODE>(x, c);
#pragma unroll
                for (int s = 0; s < ZSEL_S; s++) {
                    const K top = sh[s] + MTS_RANK_BITS >= KB ? (K)0 : (K)(key >> hs[s]);
                    if (act[s] && top == pf[s]) {
                        atomicAdd(&lh[(s * ZSEL_BINS + (int)((key >> sh[s]) & (ZSEL_BINS - 1))) * 64 + lane], 1u);
                        mn[s] = key < mn[s] ? key : mn[s];
                        mx[s] = key > mx[s] ? key : mx[s];
                    }
                }
            };
            const float *p = base + j;
            long r = w;
            for (; r + (ZSEL_UNROLL - 1) * ZSEL_WAVES < n; r += ZSEL_UNROLL * ZSEL_WAVES) {
                float x[ZSEL_UNROLL];
#pragma unroll
                for (int u = 0; u < ZSEL_UNROLL; u++) x[u] = p[(u64)(r + u * ZSEL_WAVES) * (u64)n_cols];
#pragma unroll
                for (int u = 0; u < ZSEL_UNROLL; u++) count(x[u]);
            }
            for (; r < n; r += ZSEL_WAVES) count(p[(u64)r * (u64)n_cols]);
#pragma unroll
            for (int s = 0; s < ZSEL_S; s++)
                if (act[s] && mn[s] <= mx[s]) { atomicMin(&lmin[s * 64 + lane], mn[s]); atomicMax(&lmax[s * 64 + lane], mx[s]); }
        }
        __syncthreads();
        // flush: lanes are consecutive columns of one (window, selector, digit) row of the histogram
        for (int e = threadIdx.x; e < ZSEL_S * ZSEL_BINS * 64; e += 64 * ZSEL_WAVES) {
            const u32 v = lh[e];
            const int l = e & 63, sb = e >> 6;              // sb = selector * 256 + digit
            if (v && g0 + l < n_cols) atomicAdd(&hist[(win * (ZSEL_S * ZSEL_BINS) + (u64)sb) * (u64)n_cols + (u64)(g0 + l)], v);
        }
        if (threadIdx.x < ZSEL_S * 64) {
            const int l = threadIdx.x & 63, s = threadIdx.x >> 6;
            const K a = lmin[threadIdx.x], b = lmax[threadIdx.x];
            if (g0 + l < n_cols && a <= b) {
                const u64 o = (win * ZSEL_S + s) * (u64)n_cols + (u64)(g0 + l);
                atomicMin(&kmin[o], (unsigned long long)a);
                atomicMax(&kmax[o], (unsigned long long)b);
            }
        }
        __syncthreads();
        r0 = seg.r1;
    }
}

namespace {

template <typename K, int MODE>
int launch_mode(hipStream_t st, const float *d_y, long s0, long s1, long H, int n_cols, long row_begin, long window_rows, const double *d_center,
                const u64 *d_prefix, const int *d_shift, u32 *d_hist, u64 *d_kmin, u64 *d_kmax)
{
    MTS_LDS_ATTR((k_zrank_hist<K, MODE>), ZSEL_LDS);
    hipLaunchKernelGGL((k_zrank_hist<K, MODE>), dim3((unsigned)zrank_blocks(s0, s1, H), (unsigned)((n_cols + 63) / 64)), dim3(64 * ZSEL_WAVES),
                       ZSEL_LDS, st, d_y, s0, s1, H, n_cols, row_begin, window_rows, d_center, d_prefix, d_shift, d_hist,
                       (unsigned long long *)d_kmin, (unsigned long long *)d_kmax);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace

int launch_zrank_hist(hipStream_t st, int mode, const float *d_y, long s0, long s1, long H, int n_cols, long row_begin, long window_rows,
                      const double *d_center, const u64 *d_prefix, const int *d_shift, u32 *d_hist, u64 *d_kmin, u64 *d_kmax)
{
    if (s1 <= s0) return MTS_OK;
    if (H < 1 || zrank_blocks(s0, s1, H) >= (1l << 31) || n_cols < 1 || (n_cols + 63) / 64 > 65535) {
        set_error("filtered rank hist: a slab of %ld rows x %d columns in blocks of %ld rows", s1 - s0, n_cols, H); return MTS_E_ARG;
    }
#define MTS_ZSEL_ARGS st, d_y, s0, s1, H, n_cols, row_begin, window_rows, d_center, d_prefix, d_shift, d_hist, d_kmin, d_kmax
    if (mode == 0) return launch_mode<u32, 0>(MTS_ZSEL_ARGS);
    if (mode == 1) return launch_mode<u64, 1>(MTS_ZSEL_ARGS);
    if (mode == 2) return launch_mode<u64, 2>(MTS_ZSEL_ARGS);
#undef MTS_ZSEL_ARGS
    return MTS_E_ARG;
}

}  // namespace mts
