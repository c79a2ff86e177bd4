// Per-channel power spectral density of decoded chunks, Welch's method (mts_welch, mts_dev_welch).
//
// Segment s of a call covers file rows [row_seg0 + s * step, row_seg0 + s * step + N), N = nperseg = 2^LOG2N.  For a segment and
// a column: m = the segment's mean in float64 (integers: the exact sum rounded once; floats: the pairwise tree v = v[0::2] + v[1::2]),
// y[n] = F(double(x[n]) - m) * F(taper[n]) in the compute type F (no detrend: m = 0), X = the real FFT of y in F, and
// P[k] = double(Re X[k])^2 + double(Im X[k])^2 for k = 0 .. N/2.  Input: a segment table, as for k_decimate: chunk s of the table
// holds file rows [seg_row0[s], seg_row0[s + 1]) at seg_base[s] (n_channels items per row).
//   k_welch    one workgroup of 512 threads per (block of WELCH_BLOCK_SEGMENTS segments) x (tile of C columns).  Thread t works on
//              column c = t % C and rows / points / bins p = t / C (mod P = 512 / C); the tile of a segment is N / 2 complex points
//              per column in LDS, interleaved [point][column] (C * N * sizeof(F) <= 64 KiB; 128 KiB for float64 at N = 16384).
//              Per segment: stream the thread's K = N / P contiguous rows, reduce the mean (a pairwise stack in registers, then
//              a tree over p in LDS), stream them again and write y as z[n / 2] = y[n & ~1] + i y[n | 1], run the N / 2-point complex FFT (Stockham, radix-4 passes and one radix-2
//              pass when log2(N / 2) is odd; every pass reads all its inputs, waits at a barrier, and writes its outputs in
//              place), split it into the N / 2 + 1 bins of the real FFT, and add P to the thread's float64 accumulators (fixed
//              bins).  After the block's last segment each thread writes its bins: one partial per (block, bin, column).
//   k_welch_combine  adds a launch's block partials to the group accumulators, block by block in order.
// Twiddles: tw[q] = exp(-2 pi i q / N), q < N, computed on the host in extended precision and rounded once to F (tw[0] = 1).
// Nothing depends on the piece, launch, call or device: the same bits everywhere.
#include <type_traits>

#include "common.h"

namespace mts {

namespace {

constexpr int WT = 512;                                           // threads per workgroup (8 waves: 2 per SIMD)
constexpr long WELCH_TILE_BYTES = 65536;                           // LDS for a tile's points (at least one column)

template <typename F> struct Cx { typedef F type __attribute__((ext_vector_type(2))); };

template <typename F, int LOG2N>
struct WPlan {
    static constexpr int N = 1 << LOG2N, M = N / 2, LOG2M = LOG2N - 1;
    static constexpr long C0 = WELCH_TILE_BYTES / ((long)N * (long)sizeof(F));
    static constexpr int C = C0 < 1 ? 1 : C0 > 64 ? 64 : (int)C0;  // columns per tile (a power of two)
    static constexpr int P = WT / C;                                // threads per column
    static constexpr int K = N / P;                                 // rows per thread and segment
    static constexpr int MC = M * C;                                // complex points in LDS
    static constexpr int BINS = MC / WT;                            // bins per thread (+ bin N / 2 for p == 0)
    // one workgroup per CU (8 waves); 256 VGPRs per thread hold K rows' stream, a pass's PER x R points and BINS float64 sums
    // with at most a few spilled (the float64 tile at N = 16384 spills more; with 256 threads every float32 N >= 256 spilled 170-250)
    static constexpr int WAVES_PER_SIMD = 2;
    static_assert(P <= N && K >= 1 && BINS >= 1, "plan");
};

template <typename F>
__device__ __forceinline__ typename Cx<F>::type cmul(typename Cx<F>::type a, typename Cx<F>::type w)
{
    typedef typename Cx<F>::type F2;
    F2 r;
    r.x = a.x * w.x - a.y * w.y;
    r.y = a.x * w.y + a.y * w.x;
    return r;
}

// one Stockham pass of radix R on the N / 2-point transforms of the C columns (Ns: the length of the sub-transforms done so far)
template <typename F, int LOG2N, int R>
__device__ __forceinline__ void fft_pass(typename Cx<F>::type *z, const typename Cx<F>::type *__restrict__ tw, int lns, int t)
{
    typedef WPlan<F, LOG2N> W;
    typedef typename Cx<F>::type F2;
    constexpr int LR = R == 4 ? 2 : 1;
    constexpr int NB = W::M / R * W::C;                            // butterflies of the pass
    constexpr int PER = (NB + WT - 1) / WT;
    F2 v[PER][R];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int bf = t + WT * i;
        if (NB % WT == 0 || bf < NB) {
            const int c = bf & (W::C - 1), j = bf / W::C;
#pragma unroll
            for (int r = 0; r < R; r++) v[i][r] = z[(j + r * (W::M / R)) * W::C + c];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int bf = t + WT * i;
        if (NB % WT == 0 || bf < NB) {
            const int c = bf & (W::C - 1), j = bf / W::C;
            const int k = j & ((1 << lns) - 1);
            if (lns > 0) {
                const int sh = LOG2N - lns - LR;                   // tw index of r * k / (Ns * R) of a turn
#pragma unroll
                for (int r = 1; r < R; r++) v[i][r] = cmul<F>(v[i][r], tw[(k * r) << sh]);
            }
            if (R == 4) {
                const F2 a = v[i][0] + v[i][2], b = v[i][0] - v[i][2], cc = v[i][1] + v[i][3], d = v[i][1] - v[i][3];
                v[i][0] = a + cc;
                v[i][2] = a - cc;
                v[i][1].x = b.x + d.y; v[i][1].y = b.y - d.x;     // b - i d
                v[i][3].x = b.x - d.y; v[i][3].y = b.y + d.x;     // b + i d
            } else {
                const F2 a = v[i][0];
                v[i][0] = a + v[i][1];
                v[i][1] = a - v[i][1];
            }
            const int d0 = ((j >> lns) << (lns + LR)) + k;
#pragma unroll
            for (int r = 0; r < R; r++) z[(d0 + (r << lns)) * W::C + c] = v[i][r];
        }
    }
    __syncthreads();
}

// the rows of one thread, ascending, one column: the chunk of the current row and a pointer to its item; rows outside the chunks
// (none when the host's checks hold) and columns past the tile's read as 0
template <typename T>
struct RowWalk {
    int ci;
    long row, c_hi;
    const T *q;
    bool ok;
    __device__ __forceinline__ void start(const u8 *const *seg_base, const long *seg_row0, int n_segs, int pitch, int col, bool col_ok, long r)
    {
        int lo = 0, hi = n_segs - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg_row0[mid] <= r) lo = mid; else hi = mid - 1; }
        ci = lo;
        row = r;
        c_hi = seg_row0[ci + 1];
        ok = col_ok && r >= seg_row0[ci];
        q = (const T *)seg_base[ci] + (u64)(r - seg_row0[ci]) * (u64)pitch + col;
    }
    __device__ __forceinline__ T next(const u8 *const *seg_base, const long *seg_row0, int n_segs, int pitch, int col)
    {
        if (row >= c_hi) {
            if (ci + 1 < n_segs) {
                ci++;
                c_hi = seg_row0[ci + 1];
                q = (const T *)seg_base[ci] + col;
            } else {
                ok = false;
            }
        }
        const T v = ok ? *q : (T)0;
        q += pitch;
        row++;
        return v;
    }
};

}  // namespace

template <typename T, typename F, int LOG2N>
__global__ __launch_bounds__(WT, (WPlan<F, LOG2N>::WAVES_PER_SIMD)) void k_welch(
    const u8 *const *__restrict__ seg_base, const long *__restrict__ seg_row0, int n_segs, int pitch, const int *__restrict__ cols, int n_cols,
    const F *__restrict__ taper, const typename Cx<F>::type *__restrict__ tw, long row_seg0, long step, long seg_end, long block0, int detrend,
    double *__restrict__ out)
{
    typedef WPlan<F, LOG2N> W;
    typedef typename Cx<F>::type F2;
    constexpr int N = W::N, M = W::M, C = W::C, P = W::P, K = W::K, LOG2K = __builtin_ctz(K);
    __shared__ __attribute__((aligned(16))) F2 z[W::MC];
    __shared__ __attribute__((aligned(16))) long red[2 * WT];      // the mean's partial sums: a double, or (hi, lo) for integers
    const int t = threadIdx.x;
    const int c = t & (C - 1), p = t / C;
    const int c0 = blockIdx.x * C;
    const bool col_ok = c0 + c < n_cols;
    const int col = col_ok ? cols[c0 + c] : 0;
    const long blk = block0 + blockIdx.y;
    const long s0 = blk * WELCH_BLOCK_SEGMENTS;
    const long s1 = s0 + WELCH_BLOCK_SEGMENTS < seg_end ? s0 + WELCH_BLOCK_SEGMENTS : seg_end;

    double acc[W::BINS], acc_m = 0.0;
#pragma unroll
    for (int i = 0; i < W::BINS; i++) acc[i] = 0.0;

    for (long s = s0; s < s1; s++) {
        // the thread's rows: [a, a + K) of the segment starting at r0, column col; the chunk of row a found by bisection
        const long r0 = row_seg0 + s * step, a = r0 + (long)p * K;
        RowWalk<T> rw;
        rw.start(seg_base, seg_row0, n_segs, pitch, col, col_ok, a);
        double m = 0.0;
        if (detrend) {
            if constexpr (std::is_floating_point<T>::value) {
                // pairwise over the thread's K rows (v = v[0::2] + v[1::2] until one is left), streamed: st[l] holds a finished
                // sum of 2^l rows waiting for its right neighbour
                double st[LOG2K + 1];
#pragma unroll
                for (int k = 0; k < K; k++) {
                    double cur = (double)rw.next(seg_base, seg_row0, n_segs, pitch, col);
#pragma unroll
                    for (int l = 0; l < LOG2K && (((k + 1) >> l) & 1) == 0; l++) cur = st[l] + cur;
                    st[__builtin_ctz(k + 1) < LOG2K ? __builtin_ctz(k + 1) : LOG2K] = cur;
                }
                ((double *)red)[t] = st[LOG2K];
                for (int h = 1; h < P; h <<= 1) {                  // then across the threads of the column: p, p + h for p % 2h == 0
                    __syncthreads();
                    if ((p & (2 * h - 1)) == 0) ((double *)red)[t] = ((double *)red)[t] + ((double *)red)[t + C * h];
                }
                __syncthreads();
                m = ((double *)red)[c] * (1.0 / N);
            } else {
                // exact: sum(x >> 32) and sum(x & 0xffffffff) fit in 64 bits (N <= 2^14), S = hi * 2^32 + lo rounded once
                long shi = 0, slo = 0;
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const T v = rw.next(seg_base, seg_row0, n_segs, pitch, col);
                    if constexpr (std::is_signed<T>::value) {
                        const long x = (long)v;
                        shi += x >> 32; slo += (long)(x & 0xffffffffl);
                    } else {
                        const u64 x = (u64)v;
                        shi += (long)(x >> 32); slo += (long)(x & 0xffffffffull);
                    }
                }
                red[2 * t] = shi; red[2 * t + 1] = slo;
                for (int h = 1; h < P; h <<= 1) {
                    __syncthreads();
                    if ((p & (2 * h - 1)) == 0) { red[2 * t] += red[2 * (t + C * h)]; red[2 * t + 1] += red[2 * (t + C * h) + 1]; }
                }
                __syncthreads();
                m = ((double)red[2 * c] * 4294967296.0 + (double)red[2 * c + 1]) * (1.0 / N);
            }
            rw.start(seg_base, seg_row0, n_segs, pitch, col, col_ok, a);
        }
        // y into the tile: rows n, n + 1 (n = p * K + k, k even) are point n / 2 of the column
#pragma unroll
        for (int k = 0; k < K; k += 2) {
            const int n = p * K + k;
            const double x0 = (double)rw.next(seg_base, seg_row0, n_segs, pitch, col);
            const double x1 = (double)rw.next(seg_base, seg_row0, n_segs, pitch, col);
            F2 y;
            y.x = (F)(x0 - m) * taper[n];
            y.y = (F)(x1 - m) * taper[n + 1];
            z[(n >> 1) * C + c] = y;
        }
        __syncthreads();
        int lns = 0;
#pragma unroll 1
        for (; lns + 2 <= W::LOG2M; lns += 2) fft_pass<F, LOG2N, 4>(z, tw, lns, t);
        if (lns < W::LOG2M) fft_pass<F, LOG2N, 2>(z, tw, lns, t);
        // split: X[k] = E[k] + W^k O[k], E = (Z[k] + conj Z[M - k]) / 2, O = (Z[k] - conj Z[M - k]) / 2i; X[0], X[M] from Z[0]
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int i = 0; i < W::BINS; i++) {
                const int k = p + P * i;
                const F2 a = z[k * C + c];
                if (k == 0) {
                    const double x0 = (double)(a.x + a.y), xm = (double)(a.x - a.y);
                    acc[i] = acc[i] + x0 * x0;
                    acc_m = acc_m + xm * xm;
                } else {
                    const F2 b = z[(M - k) * C + c];
                    const F half = (F)0.5;
                    F2 e, o;
                    e.x = (a.x + b.x) * half; e.y = (a.y - b.y) * half;
                    o.x = (a.y + b.y) * half; o.y = (b.x - a.x) * half;
                    const F2 w = tw[k];
                    const F xr = e.x + (w.x * o.x - w.y * o.y), xi = e.y + (w.x * o.y + w.y * o.x);
                    const double dr = (double)xr, di = (double)xi;
                    acc[i] = acc[i] + (dr * dr + di * di);
                }
            }
        }
        __syncthreads();                                           // (the next segment overwrites the tile and the sums)
    }
    if (!col_ok) return;
    double *o = out + (u64)(blk - block0) * (u64)(M + 1) * (u64)n_cols + (u64)(c0 + c);
#pragma unroll
    for (int i = 0; i < W::BINS; i++) o[(u64)(p + P * i) * (u64)n_cols] = acc[i];
    if (p == 0) o[(u64)M * (u64)n_cols] = acc_m;
}

// acc[g][e] = acc[g][e] + part[b][e] for the launch's blocks b of group g, in block order (blocks lb0 .. lb1 - 1 of the call)
__global__ void k_welch_combine(const double *__restrict__ part, long lb0, long lb1, long group_blocks, long n_elems, double *__restrict__ acc)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_elems) return;
    const long g = lb0 / group_blocks + blockIdx.y;
    const long b0 = g * group_blocks > lb0 ? g * group_blocks : lb0;
    const long b1 = (g + 1) * group_blocks < lb1 ? (g + 1) * group_blocks : lb1;
    double a = acc[(u64)g * (u64)n_elems + (u64)e];
    for (long b = b0; b < b1; b++) a = a + part[(u64)(b - lb0) * (u64)n_elems + (u64)e];
    acc[(u64)g * (u64)n_elems + (u64)e] = a;
}

namespace {

template <typename T, typename F, int LOG2N>
int launch_n(hipStream_t st, const u8 *const *b, const long *r0, int ns, int nc, const int *cols, int n_cols, const void *taper, const void *tw,
             long row_seg0, long step, long seg_end, long block0, long n_blocks, int detrend, double *out)
{
    typedef WPlan<F, LOG2N> W;
    const dim3 grid((unsigned)((n_cols + W::C - 1) / W::C), (unsigned)n_blocks);
    hipLaunchKernelGGL((k_welch<T, F, LOG2N>), grid, dim3(WT), 0, st, b, r0, ns, nc, cols, n_cols, (const F *)taper,
                       (const typename Cx<F>::type *)tw, row_seg0, step, seg_end, block0, detrend, out);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

template <typename T, typename F>
int launch_f(hipStream_t st, int log2n, const u8 *const *b, const long *r0, int ns, int nc, const int *cols, int n_cols, const void *taper,
             const void *tw, long row_seg0, long step, long seg_end, long block0, long n_blocks, int detrend, double *out)
{
    switch (log2n) {
#define MTS_WELCH_N(L) \
    case L: return launch_n<T, F, L>(st, b, r0, ns, nc, cols, n_cols, taper, tw, row_seg0, step, seg_end, block0, n_blocks, detrend, out)
    MTS_WELCH_N(4); MTS_WELCH_N(5); MTS_WELCH_N(6); MTS_WELCH_N(7); MTS_WELCH_N(8); MTS_WELCH_N(9);
    MTS_WELCH_N(10); MTS_WELCH_N(11); MTS_WELCH_N(12); MTS_WELCH_N(13); MTS_WELCH_N(14);
#undef MTS_WELCH_N
    }
    return MTS_E_ARG;
}

template <typename T>
int launch_t(hipStream_t st, int csize, int log2n, const u8 *const *b, const long *r0, int ns, int nc, const int *cols, int n_cols,
             const void *taper, const void *tw, long row_seg0, long step, long seg_end, long block0, long n_blocks, int detrend, double *out)
{
    if (csize == 4) return launch_f<T, float>(st, log2n, b, r0, ns, nc, cols, n_cols, taper, tw, row_seg0, step, seg_end, block0, n_blocks, detrend, out);
    if (csize == 8) return launch_f<T, double>(st, log2n, b, r0, ns, nc, cols, n_cols, taper, tw, row_seg0, step, seg_end, block0, n_blocks, detrend, out);
    return MTS_E_ARG;
}

}  // namespace

int welch_tile_columns(int csize, int log2n)
{
    const long c = WELCH_TILE_BYTES / ((1l << log2n) * (long)csize);
    return c < 1 ? 1 : c > 64 ? 64 : (int)c;
}

int launch_welch(hipStream_t st, int itemsize, int flags, int csize, int log2n, const u8 *const *d_seg_base, const long *d_seg_row0, int n_segs,
                 int n_channels, const int *d_cols, int n_cols, const void *d_taper, const void *d_tw, long row_seg0, long step, long seg_end,
                 long block0, long n_blocks, int detrend, double *d_part)
{
    if (n_blocks <= 0) return MTS_OK;
    if (n_blocks > 65535) { set_error("welch: too many blocks in one launch"); return MTS_E_ARG; }
#define MTS_WELCH_CASE(T) \
    return launch_t<T>(st, csize, log2n, d_seg_base, d_seg_row0, n_segs, n_channels, d_cols, n_cols, d_taper, d_tw, row_seg0, step, seg_end, block0, n_blocks, detrend, d_part)
    if (flags & MTS_FLAG_FLOAT) {
        if (itemsize == 4) MTS_WELCH_CASE(float);
        if (itemsize == 8) MTS_WELCH_CASE(double);
    } else if (flags & MTS_FLAG_UNSIGNED) {
        if (itemsize == 1) MTS_WELCH_CASE(uint8_t);
        if (itemsize == 2) MTS_WELCH_CASE(uint16_t);
        if (itemsize == 4) MTS_WELCH_CASE(uint32_t);
        if (itemsize == 8) MTS_WELCH_CASE(uint64_t);
    } else {
        if (itemsize == 1) MTS_WELCH_CASE(int8_t);
        if (itemsize == 2) MTS_WELCH_CASE(int16_t);
        if (itemsize == 4) MTS_WELCH_CASE(int32_t);
        if (itemsize == 8) MTS_WELCH_CASE(int64_t);
    }
#undef MTS_WELCH_CASE
    return MTS_E_ARG;
}

int launch_welch_combine(hipStream_t st, const double *d_part, long lb0, long lb1, long group_blocks, long n_elems, double *d_acc)
{
    if (lb1 <= lb0 || n_elems <= 0) return MTS_OK;
    const long ng = (lb1 - 1) / group_blocks - lb0 / group_blocks + 1;
    const dim3 grid((unsigned)((n_elems + 255) / 256), (unsigned)ng);
    hipLaunchKernelGGL(k_welch_combine, grid, dim3(256), 0, st, d_part, lb0, lb1, group_blocks, n_elems, d_acc);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace mts
