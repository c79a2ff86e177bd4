// One round of a most-significant-digit radix select over decoded chunks (mts_rank_hist, mts_dev_rank_hist).
//
// Input: decoded C-order (rows, n_channels) chunks in HBM, as stats.hip reads them.  The rows of every (chunk ∩ window) segment are cut
// into tiles of at most SEL_TILE_ROWS rows (api.hip).  Every item is mapped to its order key (an unsigned integer whose order is
// np.sort's order of the items: include/mtscomp_hip.h spells the maps out); a (window, column) cell has MTS_RANK_SELECTORS selectors
// (prefix, shift), and an item is a candidate of a selector when key >> (shift + 8) == prefix.
//   k_rank_hist   one workgroup per tile: the 64 lanes of a wave take 64 consecutive entries of `cols`, the SEL_WAVES waves take every
//                 SEL_WAVES-th row.  A candidate increments the 32-bit LDS counter hist[selector][digit][lane]: lane l is bank l mod 32
//                 whatever the digit, and a 4-byte access is served in two groups of 32 lanes, so neither random data nor a constant
//                 column gives a bank conflict (the waves of the workgroup still meet on one address for a constant column: that is
//                 what the LDS atomic is for).  2 x 256 x 64 x 4 B = 128 KiB of the CU's 160.  At the end of the tile the non-zero
//                 counters go to the cell's histogram in HBM with integer atomicAdd and the smallest / largest candidate key with
//                 integer atomicMin / atomicMax.  Integers only: the outputs do not depend on the order of tiles, launches or calls.
#include <type_traits>

#include "common.h"

namespace mts {

namespace {

constexpr int SEL_WAVES = 16;            // one workgroup of 1024 threads per CU (the LDS allows no second one)
constexpr int SEL_UNROLL = 4;            // rows of one wave in flight
constexpr int SEL_S = MTS_RANK_SELECTORS;
constexpr int SEL_BINS = 1 << MTS_RANK_BITS;
constexpr int SEL_LDS_HIST = SEL_S * SEL_BINS * 64 * 4;
constexpr int SEL_LDS = SEL_LDS_HIST + 2 * SEL_S * 64 * 8;
static_assert(MTS_RANK_BITS == 8 && SEL_S == 2, "the LDS budget and the flush are written for two selectors of 8-bit digits");

// float bit pattern -> key: -0 is +0, every NaN is all ones, negative numbers reversed below the positive ones
__device__ __forceinline__ u32 fkey(float x)
{
    if (x != x) return ~0u;
    if (x == 0.0f) return 0x80000000u;
    const u32 b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ u64 dkey(double x)
{
    if (x != x) return ~0ull;
    if (x == 0.0) return 0x8000000000000000ull;
    const u64 b = (u64)__double_as_longlong(x);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}

// MODE 0: the item in its own type.  MODE 1: double(x) - c.  MODE 2: |double(x) - c|.
template <typename T, typename K, int MODE> __device__ __forceinline__ K make_key(T x, double c)
{
    if constexpr (MODE == 0) {
        if constexpr (std::is_same<T, float>::value) return fkey(x);
        else if constexpr (std::is_same<T, double>::value) return dkey(x);
        else if constexpr (std::is_signed<T>::value) return (K)(std::make_unsigned_t<T>)x ^ ((K)1 << (8 * sizeof(T) - 1));
        else return (K)x;
    } else {
        const double d = (double)x - c;
        return dkey(MODE == 2 ? __builtin_fabs(d) : d);
    }
}

template <typename K> __device__ __forceinline__ K lds_min(K *p, K v) { return atomicMin(p, v); }
template <typename K> __device__ __forceinline__ K lds_max(K *p, K v) { return atomicMax(p, v); }

}  // namespace

template <typename T, typename K, int MODE>
__global__ __launch_bounds__(64 * SEL_WAVES) void k_rank_hist(const StatTile *__restrict__ tiles, const long *__restrict__ tile_win,
                                                              const int *__restrict__ ids, const int *__restrict__ ok,
                                                              const int *__restrict__ cols, int n_cols, int pitch,
                                                              const double *__restrict__ center, const u64 *__restrict__ sel_prefix,
                                                              const int *__restrict__ sel_shift, u32 *__restrict__ hist,
                                                              unsigned long long *__restrict__ kmin, unsigned long long *__restrict__ kmax)
{
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    u32 *lh = (u32 *)smem;                                     // [selector][digit][lane]
    K *lmin = (K *)(smem + SEL_LDS_HIST), *lmax = lmin + SEL_S * 64;
    constexpr int KB = 8 * (int)sizeof(K);
    const int tid = ids[blockIdx.x];
    const StatTile t = tiles[tid];
    if (!ok[t.chunk]) return;                                  // (a chunk that failed to decode counts nothing; uniform)
    const u64 win = (u64)tile_win[tid];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T *base = (const T *)t.base + (u64)t.row_lo * (u64)pitch;
    const long n = t.n_rows;
    for (int g0 = 0; g0 < n_cols; g0 += 64) {
        for (int e = threadIdx.x; e < SEL_S * SEL_BINS * 64; e += 64 * SEL_WAVES) lh[e] = 0;
        if (threadIdx.x < SEL_S * 64) { lmin[threadIdx.x] = (K)~(K)0; lmax[threadIdx.x] = 0; }
        __syncthreads();
        const int j = g0 + lane;
        bool act[SEL_S];
        int sh[SEL_S], hs[SEL_S];
        K pf[SEL_S], mn[SEL_S], mx[SEL_S];
#pragma unroll
        for (int s = 0; s < SEL_S; s++) { act[s] = false; sh[s] = 0; hs[s] = 0; pf[s] = 0; mn[s] = (K)~(K)0; mx[s] = 0; }
        if (j < n_cols) {
            double c = 0.0;
            if constexpr (MODE != 0) c = center[win * (u64)n_cols + (u64)j];
#pragma unroll
            for (int s = 0; s < SEL_S; s++) {
                const u64 o = (win * SEL_S + s) * (u64)n_cols + (u64)j;
                const int v = sel_shift[o];
                act[s] = v >= 0;
                sh[s] = act[s] ? v : 0;
                // every bit above the digit is prefix; a digit that reaches the top of the key has none (prefix 0, nothing to shift by)
                if (sh[s] + MTS_RANK_BITS >= KB) { hs[s] = KB - 1; pf[s] = 0; }
                else { hs[s] = sh[s] + MTS_RANK_BITS; pf[s] = (K)sel_prefix[o]; }
            }
            auto count = [&](T x) {
                const K key = make_key<T, K, MODE>(x, c);
#pragma unroll
                for (int s = 0; s < SEL_S; s++) {
                    const K top = sh[s] + MTS_RANK_BITS >= KB ? (K)0 : (K)(key >> hs[s]);
                    if (act[s] && top == pf[s]) {
                        atomicAdd(&lh[(s * SEL_BINS + (int)((key >> sh[s]) & (SEL_BINS - 1))) * 64 + lane], 1u);
                        mn[s] = key < mn[s] ? key : mn[s];
                        mx[s] = key > mx[s] ? key : mx[s];
                    }
                }
            };
            const T *p = base + cols[j];
            long r = w;
            for (; r + (SEL_UNROLL - 1) * SEL_WAVES < n; r += SEL_UNROLL * SEL_WAVES) {
                T x[SEL_UNROLL];
#pragma unroll
                for (int u = 0; u < SEL_UNROLL; u++) x[u] = p[(u64)(r + u * SEL_WAVES) * (u64)pitch];
#pragma unroll
                for (int u = 0; u < SEL_UNROLL; u++) count(x[u]);
            }
            for (; r < n; r += SEL_WAVES) count(p[(u64)r * (u64)pitch]);
#pragma unroll
            for (int s = 0; s < SEL_S; s++)
                if (act[s] && mn[s] <= mx[s]) { lds_min(&lmin[s * 64 + lane], mn[s]); lds_max(&lmax[s * 64 + lane], mx[s]); }
        }
        __syncthreads();
        // flush: lanes are consecutive columns of one (window, selector, digit) row of the histogram
        for (int e = threadIdx.x; e < SEL_S * SEL_BINS * 64; e += 64 * SEL_WAVES) {
            const u32 v = lh[e];
            const int l = e & 63, sb = e >> 6;                  // sb = selector * 256 + digit
            if (v && g0 + l < n_cols) atomicAdd(&hist[(win * (SEL_S * SEL_BINS) + (u64)sb) * (u64)n_cols + (u64)(g0 + l)], v);
        }
        if (threadIdx.x < SEL_S * 64) {
            const int l = threadIdx.x & 63, s = threadIdx.x >> 6;
            const K a = lmin[threadIdx.x], b = lmax[threadIdx.x];
            if (g0 + l < n_cols && a <= b) {
                const u64 o = (win * SEL_S + s) * (u64)n_cols + (u64)(g0 + l);
                atomicMin(&kmin[o], (unsigned long long)a);
                atomicMax(&kmax[o], (unsigned long long)b);
            }
        }
        __syncthreads();
    }
}

namespace {

template <typename T, typename K, int MODE>
int launch_mode(hipStream_t st, const StatTile *d_tiles, const long *d_tile_win, const int *d_ids, int n_launch, const int *d_ok,
                const int *d_cols, int n_cols, int n_channels, const double *d_center, const u64 *d_prefix, const int *d_shift, u32 *d_hist,
                u64 *d_kmin, u64 *d_kmax)
{
    MTS_LDS_ATTR((k_rank_hist<T, K, MODE>), SEL_LDS);
    hipLaunchKernelGGL((k_rank_hist<T, K, MODE>), dim3((unsigned)n_launch), dim3(64 * SEL_WAVES), SEL_LDS, st, d_tiles, d_tile_win, d_ids, d_ok,
                       d_cols, n_cols, n_channels, d_center, d_prefix, d_shift, d_hist, (unsigned long long *)d_kmin,
                       (unsigned long long *)d_kmax);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

template <typename T>
int launch_typed(hipStream_t st, int mode, const StatTile *d_tiles, const long *d_tile_win, const int *d_ids, int n_launch, const int *d_ok,
                 const int *d_cols, int n_cols, int n_channels, const double *d_center, const u64 *d_prefix, const int *d_shift, u32 *d_hist,
                 u64 *d_kmin, u64 *d_kmax)
{
    using K0 = std::conditional_t<(sizeof(T) <= 4), u32, u64>;
#define MTS_SEL_ARGS st, d_tiles, d_tile_win, d_ids, n_launch, d_ok, d_cols, n_cols, n_channels, d_center, d_prefix, d_shift, d_hist, d_kmin, d_kmax
    if (mode == 0) return launch_mode<T, K0, 0>(MTS_SEL_ARGS);
    if (mode == 1) return launch_mode<T, u64, 1>(MTS_SEL_ARGS);
    if (mode == 2) return launch_mode<T, u64, 2>(MTS_SEL_ARGS);
#undef MTS_SEL_ARGS
    return MTS_E_ARG;
}

}  // namespace

int launch_rank_hist(hipStream_t st, int itemsize, int flags, int mode, const StatTile *d_tiles, const long *d_tile_win, const int *d_ids,
                     int n_launch, const int *d_ok, const int *d_cols, int n_cols, int n_channels, const double *d_center, const u64 *d_prefix,
                     const int *d_shift, u32 *d_hist, u64 *d_kmin, u64 *d_kmax)
{
    if (n_launch <= 0) return MTS_OK;
#define MTS_SEL_CASE(T) \
    return launch_typed<T>(st, mode, d_tiles, d_tile_win, d_ids, n_launch, d_ok, d_cols, n_cols, n_channels, d_center, d_prefix, d_shift, d_hist, d_kmin, d_kmax)
    if (flags & MTS_FLAG_FLOAT) {
        if (itemsize == 4) MTS_SEL_CASE(float);
        if (itemsize == 8) MTS_SEL_CASE(double);
    } else if (flags & MTS_FLAG_UNSIGNED) {
        if (itemsize == 1) MTS_SEL_CASE(uint8_t);
        if (itemsize == 2) MTS_SEL_CASE(uint16_t);
        if (itemsize == 4) MTS_SEL_CASE(uint32_t);
        if (itemsize == 8) MTS_SEL_CASE(uint64_t);
    } else {
        if (itemsize == 1) MTS_SEL_CASE(int8_t);
        if (itemsize == 2) MTS_SEL_CASE(int16_t);
        if (itemsize == 4) MTS_SEL_CASE(int32_t);
        if (itemsize == 8) MTS_SEL_CASE(int64_t);
    }
#undef MTS_SEL_CASE
    return MTS_E_ARG;
}

}  // namespace mts
