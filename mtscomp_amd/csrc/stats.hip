// Per-window, per-channel min / max / sum / sum of squares of decoded chunks (mts_window_stats, mts_dev_window_stats).
//
// Input: decoded C-order (rows, n_channels) chunks in HBM -- entries of the decoded-chunk cache, or the workspace decompress_batch
// wrote.  The rows of every (chunk ∩ window) segment are cut into tiles of at most STAT_TILE_ROWS rows (api.hip); a window that
// covers the whole file still gives thousands of workgroups.
//   k_stats_tiles    one workgroup per tile: the 64 lanes of a wave take 64 consecutive entries of `cols` (for all channels: 64
//                    consecutive items of a row, one contiguous segment), the 4 waves of the workgroup take every 4th row and keep
//                    their accumulators in registers; the waves are combined through LDS in wave order and one partial per
//                    (tile, column) goes to the slab.  The decoded bytes are read once.
//   k_stats_combine  one thread per (window, column): the window's tiles in tile (= row) order.  No atomics anywhere: the float
//                    sums are the same from run to run.
#include <type_traits>

#include "common.h"

namespace mts {

namespace {

template <typename T> __device__ __forceinline__ T type_max()
{
    if constexpr (std::is_floating_point<T>::value) return (T)__builtin_huge_val();
    else if constexpr (std::is_signed<T>::value) return (T)((std::make_unsigned_t<T>)(~(std::make_unsigned_t<T>)0) >> 1);
    else return (T)~(T)0;
}
template <typename T> __device__ __forceinline__ T type_min()
{
    if constexpr (std::is_floating_point<T>::value) return -(T)__builtin_huge_val();
    else if constexpr (std::is_signed<T>::value) return (T)(-type_max<T>() - 1);
    else return (T)0;
}
// np.min / np.max: a NaN wins over everything and stays (once m is NaN, neither comparison holds)
template <typename T> __device__ __forceinline__ T min_nan(T m, T x) { return (x < m || x != x) ? x : m; }
template <typename T> __device__ __forceinline__ T max_nan(T m, T x) { return (x > m || x != x) ? x : m; }

// sum: x.astype(int64) with two's-complement wrap (as u64), or float64 for float items
template <typename T, typename S> __device__ __forceinline__ S to_sum(T x)
{
    if constexpr (std::is_floating_point<S>::value) return (S)x;
    else if constexpr (std::is_signed<T>::value) return (S)(long long)x;
    else return (S)x;
}
// sum of squares: exact u64 for 1- and 2-byte integers (|x|^2 < 2^32: 2^31 rows fit), float64 otherwise
template <typename T, typename Q> __device__ __forceinline__ Q to_sq(T x)
{
    if constexpr (std::is_floating_point<Q>::value) { const double d = (double)x; return d * d; }
    else { const long long v = (long long)x; return (Q)(v * v); }
}

template <typename T, typename S, typename Q>
struct Acc {
    T mn, mx; S sm; Q sq;
    __device__ __forceinline__ void init() { mn = type_max<T>(); mx = type_min<T>(); sm = 0; sq = 0; }
    __device__ __forceinline__ void add(T x) { mn = min_nan(mn, x); mx = max_nan(mx, x); sm += to_sum<T, S>(x); sq += to_sq<T, Q>(x); }
    __device__ __forceinline__ void merge(T a, T b, S s, Q q) { mn = min_nan(mn, a); mx = max_nan(mx, b); sm += s; sq += q; }
};

constexpr int STAT_WAVES = 4;
constexpr int STAT_UNROLL = 8;           // rows of one wave in flight (8 independent loads per lane)

}  // namespace

template <typename T, typename S, typename Q>
__global__ __launch_bounds__(64 * STAT_WAVES) void k_stats_tiles(const StatTile *__restrict__ tiles, const int *__restrict__ ids,
                                                                 const int *__restrict__ ok, const int *__restrict__ cols, int n_cols,
                                                                 int pitch, T *__restrict__ smin, T *__restrict__ smax,
                                                                 S *__restrict__ ssum, Q *__restrict__ ssq)
{
    __shared__ T lmin[STAT_WAVES][64], lmax[STAT_WAVES][64];
    __shared__ S lsum[STAT_WAVES][64];
    __shared__ Q lsq[STAT_WAVES][64];
    const int tid = ids[blockIdx.x];
    const StatTile t = tiles[tid];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool live = ok[t.chunk] != 0;                  // (a chunk that failed to decode: its tiles are identities)
    const T *base = (const T *)t.base + (u64)t.row_lo * (u64)pitch;
    const long n = t.n_rows;
    for (int g0 = 0; g0 < n_cols; g0 += 64) {
        const int j = g0 + lane;
        Acc<T, S, Q> a;
        a.init();
        if (live && j < n_cols) {
            const T *p = base + cols[j];
            long r = w;
            for (; r + (STAT_UNROLL - 1) * STAT_WAVES < n; r += STAT_UNROLL * STAT_WAVES) {
                T x[STAT_UNROLL];
#pragma unroll
                for (int u = 0; u < STAT_UNROLL; u++) x[u] = p[(u64)(r + u * STAT_WAVES) * (u64)pitch];
#pragma unroll
                for (int u = 0; u < STAT_UNROLL; u++) a.add(x[u]);
            }
            for (; r < n; r += STAT_WAVES) a.add(p[(u64)r * (u64)pitch]);
        }
        lmin[w][lane] = a.mn; lmax[w][lane] = a.mx; lsum[w][lane] = a.sm; lsq[w][lane] = a.sq;
        __syncthreads();
        if (w == 0 && j < n_cols) {
            Acc<T, S, Q> c;
            c.init();
#pragma unroll
            for (int k = 0; k < STAT_WAVES; k++) c.merge(lmin[k][lane], lmax[k][lane], lsum[k][lane], lsq[k][lane]);      // (wave order: deterministic)
            const u64 o = (u64)tid * (u64)n_cols + (u64)j;
            smin[o] = c.mn; smax[o] = c.mx; ssum[o] = c.sm; ssq[o] = c.sq;
        }
        __syncthreads();
    }
}

template <typename T, typename S, typename Q>
__global__ __launch_bounds__(256) void k_stats_combine(const T *__restrict__ smin, const T *__restrict__ smax, const S *__restrict__ ssum,
                                                       const Q *__restrict__ ssq, const long *__restrict__ win_tiles, long n_windows, int n_cols,
                                                       T *__restrict__ omin, T *__restrict__ omax, S *__restrict__ osum, Q *__restrict__ osq)
{
    const u64 items = (u64)n_windows * (u64)n_cols, stride = (u64)gridDim.x * 256;
    for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < items; e += stride) {
        const long w = (long)(e / (u64)n_cols);
        const u64 j = e % (u64)n_cols;
        Acc<T, S, Q> c;
        c.init();
        for (long t = win_tiles[w]; t < win_tiles[w + 1]; t++) {            // the window's tiles in row order
            const u64 o = (u64)t * (u64)n_cols + j;
            c.merge(smin[o], smax[o], ssum[o], ssq[o]);
        }
        omin[e] = c.mn; omax[e] = c.mx; osum[e] = c.sm; osq[e] = c.sq;
    }
}

namespace {

template <typename T, typename S, typename Q>
int launch_typed(hipStream_t st, const StatTile *d_tiles, const int *d_ids, int n_launch, const int *d_ok, const int *d_cols, int n_cols,
                 int n_channels, u8 *d_slab, long n_tiles, const long *d_win_tiles, long n_windows, void *o_min, void *o_max, void *o_sum,
                 void *o_sq, bool combine)
{
    const u64 plane = (u64)n_tiles * (u64)n_cols * 8;      // four planes of 8-byte entries (the item type is at most 8 bytes)
    T *smin = (T *)d_slab, *smax = (T *)(d_slab + plane);
    S *ssum = (S *)(d_slab + 2 * plane);
    Q *ssq = (Q *)(d_slab + 3 * plane);
    if (!combine) {
        if (n_launch > 0)
            hipLaunchKernelGGL((k_stats_tiles<T, S, Q>), dim3((unsigned)n_launch), dim3(64 * STAT_WAVES), 0, st, d_tiles, d_ids, d_ok, d_cols,
                               n_cols, n_channels, smin, smax, ssum, ssq);
    } else if (n_windows > 0) {
        const u64 items = (u64)n_windows * (u64)n_cols, nb = (items + 255) / 256;
        hipLaunchKernelGGL((k_stats_combine<T, S, Q>), dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, st, smin, smax, ssum, ssq,
                           d_win_tiles, n_windows, n_cols, (T *)o_min, (T *)o_max, (S *)o_sum, (Q *)o_sq);
    }
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

int launch_stats(hipStream_t st, int itemsize, int flags, const StatTile *d_tiles, const int *d_ids, int n_launch, const int *d_ok, const int *d_cols,
                 int n_cols, int n_channels, u8 *d_slab, long n_tiles, const long *d_win_tiles, long n_windows, void *o_min, void *o_max,
                 void *o_sum, void *o_sq, bool combine)
{
#define MTS_STATS_CASE(T, S, Q) \
    return launch_typed<T, S, Q>(st, d_tiles, d_ids, n_launch, d_ok, d_cols, n_cols, n_channels, d_slab, n_tiles, d_win_tiles, n_windows, o_min, o_max, o_sum, o_sq, combine)
    if (flags & MTS_FLAG_FLOAT) {
        if (itemsize == 4) MTS_STATS_CASE(float, double, double);
        if (itemsize == 8) MTS_STATS_CASE(double, double, double);
    } else if (flags & MTS_FLAG_UNSIGNED) {
        if (itemsize == 1) MTS_STATS_CASE(uint8_t, u64, u64);
        if (itemsize == 2) MTS_STATS_CASE(uint16_t, u64, u64);
        if (itemsize == 4) MTS_STATS_CASE(uint32_t, u64, double);
        if (itemsize == 8) MTS_STATS_CASE(uint64_t, u64, double);
    } else {
        if (itemsize == 1) MTS_STATS_CASE(int8_t, u64, u64);
        if (itemsize == 2) MTS_STATS_CASE(int16_t, u64, u64);
        if (itemsize == 4) MTS_STATS_CASE(int32_t, u64, double);
        if (itemsize == 8) MTS_STATS_CASE(int64_t, u64, double);
    }
#undef MTS_STATS_CASE
    return MTS_E_ARG;
}

}  // namespace

int launch_stats_tiles(hipStream_t st, int itemsize, int flags, const StatTile *d_tiles, const int *d_ids, int n_launch, const int *d_ok,
                       const int *d_cols, int n_cols, int n_channels, u8 *d_slab, long n_tiles)
{
    return launch_stats(st, itemsize, flags, d_tiles, d_ids, n_launch, d_ok, d_cols, n_cols, n_channels, d_slab, n_tiles, nullptr, 0, nullptr,
                        nullptr, nullptr, nullptr, false);
}

int launch_stats_combine(hipStream_t st, int itemsize, int flags, const u8 *d_slab, long n_tiles, const long *d_win_tiles, long n_windows,
                         int n_cols, void *d_min, void *d_max, void *d_sum, void *d_sumsq)
{
    return launch_stats(st, itemsize, flags, nullptr, nullptr, 0, nullptr, nullptr, n_cols, 0, (u8 *)d_slab, n_tiles, d_win_tiles, n_windows,
                        d_min, d_max, d_sum, d_sumsq, true);
}

}  // namespace mts
