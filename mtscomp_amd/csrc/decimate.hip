// FIR low-pass and keep every q-th row of decoded chunks (mts_decimate, mts_dev_decimate).
//
//   y[k, c] = sum_{j = 0 .. L-1} taps[j] * x[first_row + k * q - j, cols[c]]      (x = 0 outside [valid_begin, valid_end))
//
// Input: decoded C-order (rows, n_channels) chunks in HBM -- entries of the decoded-chunk cache, or the workspace decompress_batch
// wrote -- given as a segment table: seg_row0[s] is the first file row of segment s, seg_row0[n_segs] the end of the last one
// (the segments are adjacent), seg_base[s] its row 0.
//   k_decimate  one workgroup of 4 waves per tile of TO <= 8 * R output rows x 64 columns.  A wave's lanes 0..31 and 32..63 each
//               own R consecutive outputs of the tile and two adjacent columns (2p, 2p + 1) per lane; the taps are wave-uniform.
//               The input rows of the tile live in an LDS ring of S rows x 64 columns (64 KiB, converted to the compute type F):
//               the taps are walked in slabs [js, je) of <= 64, j ascending; slab s needs rows [a0 - je + 1, a_last - js], which
//               is the previous slab's window moved down by its length, so each slab stages only its new lowest rows -- every
//               input row of a tile is converted and written once.  The loads of the next slab's rows are issued before the
//               current slab is summed and written after it.
// Every output is the same sequence of operations: acc = 0, then acc = acc + taps[j] * x for j = 0 .. L-1, in F, products and
// sums rounded separately (no contraction: numpy's order and rounding), whatever the tile, piece, call or lane.  Rows outside
// the valid range are staged as +0: their products are +-0 and adding them to an accumulator that starts at +0 changes nothing.
#include <type_traits>

#include "common.h"

namespace mts {

namespace {

constexpr int DEC_WAVES = 4;
constexpr int DEC_LDS_BYTES = 65536;
constexpr int DEC_SLAB_MAX = 64;                                   // taps per slab at most (the rows a slab stages)
constexpr int DEC_PF = DEC_SLAB_MAX * 64 / (64 * DEC_WAVES);       // staged elements per thread and slab (DEC_SLAB_MAX rows)

template <typename F> struct Vec2 { typedef F type __attribute__((ext_vector_type(2))); };

// staging: rows r0 + w + 4 i (i < DEC_PF, rows < r1) of the lane's column, converted to F; 0 outside the valid range
template <typename T, typename F>
struct Stager {
    const u8 *const *seg_base;
    const long *seg_row0;
    int n_segs, pitch, col;
    bool col_ok;
    long lo, hi;                               // rows that hold data: valid range ∩ segments
    int s;                                     // the wave's current segment (uniform) ...
    long s_lo, s_hi;                           // ... its rows ...
    const T *s_p;                              // ... and its row 0 (+ the lane's column): no scalar load while a row stays in it

    __device__ __forceinline__ void seek(long row)
    {
        while (s > 0 && row < seg_row0[s]) s--;
        while (s + 1 < n_segs && row >= seg_row0[s + 1]) s++;
        s_lo = seg_row0[s]; s_hi = seg_row0[s + 1];
        s_p = (const T *)seg_base[s] + col;
    }
    __device__ __forceinline__ F fetch(long row)
    {
        if (row < lo || row >= hi) return (F)0;
        if (row < s_lo || row >= s_hi) seek(row);
        return col_ok ? (F)s_p[(u64)(row - s_lo) * (u64)pitch] : (F)0;
    }
    __device__ __forceinline__ void load(F (&v)[DEC_PF], long r0, long r1, int w)
    {
#pragma unroll
        for (int i = 0; i < DEC_PF; i++) {
            const long row = r0 + w + DEC_WAVES * i;
            v[i] = row < r1 ? fetch(row) : (F)0;
        }
    }
};

template <int S, typename F>
__device__ __forceinline__ void store_rows(F *ring, const F (&v)[DEC_PF], long r0, long r1, int w, int lane)
{
#pragma unroll
    for (int i = 0; i < DEC_PF; i++) {
        const long row = r0 + w + DEC_WAVES * i;
        if (row < r1) ring[(int)(row & (S - 1)) * 64 + lane] = v[i];
    }
}

}  // namespace

template <typename T, typename F, int R>
__global__ __launch_bounds__(64 * DEC_WAVES) void k_decimate(const u8 *const *__restrict__ seg_base, const long *__restrict__ seg_row0,
                                                            int n_segs, int pitch, const int *__restrict__ cols, int n_cols,
                                                            const F *__restrict__ taps, int n_taps, int q, long first_row, long k_begin,
                                                            long k_end, long vb, long ve, int tile_out, int slab, F *__restrict__ out)
{
#pragma clang fp contract(off)
    constexpr int S = DEC_LDS_BYTES / (64 * (int)sizeof(F));      // ring rows (a power of two)
    typedef typename Vec2<F>::type F2;
    __shared__ __attribute__((aligned(16))) F ring[S * 64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long k0 = k_begin + (long)blockIdx.x * tile_out;
    const int n_out = (int)(k_end - k0 < tile_out ? k_end - k0 : tile_out);
    const int c0 = blockIdx.y * 64;
    const long a0 = first_row + k0 * q, a_last = a0 + (long)(n_out - 1) * q;

    Stager<T, F> sg;
    sg.seg_base = seg_base; sg.seg_row0 = seg_row0; sg.n_segs = n_segs; sg.pitch = pitch;
    sg.col_ok = c0 + lane < n_cols;
    sg.col = sg.col_ok ? cols[c0 + lane] : 0;
    sg.lo = 0; sg.hi = 0; sg.s = 0; sg.s_lo = 0; sg.s_hi = 0; sg.s_p = nullptr;
    if (n_segs > 0) {
        sg.lo = vb > seg_row0[0] ? vb : seg_row0[0];
        sg.hi = ve < seg_row0[n_segs] ? ve : seg_row0[n_segs];
        const long r = a0 - (n_taps - 1);                          // the segment of the tile's lowest row (binary search, uniform)
        int lo = 0, hi = n_segs - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg_row0[mid] <= r) lo = mid; else hi = mid - 1; }
        sg.s = lo;
        sg.seek(r < sg.lo ? sg.lo : r);
    }

    // the outputs of this lane: o = w * 2R + half * R + u, two columns 2p, 2p + 1
    const int half = lane >> 5, p = lane & 31;
    const int o0 = w * 2 * R + half * R;
    F2 acc[R];
    int e0[R];                                                     // ring element of output u's row at j = 0 (+ the lane's column)
#pragma unroll
    for (int u = 0; u < R; u++) { acc[u] = (F2)(0); e0[u] = (int)((a0 + (long)(o0 + u) * q) & (S - 1)) * 64 + 2 * p; }

    F v[DEC_PF];
    int je = n_taps < slab ? n_taps : slab;
    // slab 0: rows [a0 - je + 1, a_last], in passes of DEC_SLAB_MAX rows
    for (long r = a0 - je + 1; r <= a_last; r += DEC_SLAB_MAX) {
        const long r1 = r + DEC_SLAB_MAX < a_last + 1 ? r + DEC_SLAB_MAX : a_last + 1;
        sg.load(v, r, r1, w);
        store_rows<S>(ring, v, r, r1, w, lane);
    }
    __syncthreads();
    for (int js = 0; js < n_taps;) {
        const int jn = je + slab < n_taps ? je + slab : n_taps;    // the next slab [je, jn): its new rows [a0 - jn + 1, a0 - je]
        if (je < n_taps) sg.load(v, a0 - jn + 1, a0 - je + 1, w);
        if (o0 < n_out) {
#pragma unroll 4
            for (int j = js; j < je; j++) {
                const F t = taps[j];
                const F2 tt = (F2)(t);
#pragma unroll
                for (int u = 0; u < R; u++) {                      // (row - j mod S) * 64 + column: the column bits stay
                    const F2 x = *(const F2 *)&ring[(e0[u] - 64 * j) & (S * 64 - 1)];
                    acc[u] = acc[u] + tt * x;
                }
            }
        }
        __syncthreads();
        if (je < n_taps) store_rows<S>(ring, v, a0 - jn + 1, a0 - je + 1, w, lane);
        __syncthreads();
        js = je;
        je = jn;
    }
#pragma unroll
    for (int u = 0; u < R; u++) {
        const int o = o0 + u;
        if (o >= n_out) continue;
        F *dst = out + (u64)(k0 + o - k_begin) * (u64)n_cols + (u64)(c0 + 2 * p);
        if (c0 + 2 * p < n_cols) dst[0] = acc[u].x;
        if (c0 + 2 * p + 1 < n_cols) dst[1] = acc[u].y;
    }
}

namespace {

template <typename F>
int dec_plan(int n_taps, int q, int *R, int *tile_out, int *slab)
{
    constexpr int S = DEC_LDS_BYTES / (64 * (int)sizeof(F));
    const int want = n_taps < 32 ? n_taps : 32;                   // a slab of at least this many taps
    long to = (S - want) / q + 1;                                  // outputs whose rows fit the ring beside such a slab
    if (to > 64) to = 64;
    *R = to >= 64 ? 8 : to >= 32 ? 4 : to >= 16 ? 2 : 1;
    *tile_out = (int)(to < 8 * *R ? to : 8 * *R);
    long sl = S - (long)(*tile_out - 1) * q;
    *slab = (int)(sl < DEC_SLAB_MAX ? sl : DEC_SLAB_MAX);
    return MTS_OK;
}

template <typename T, typename F>
int launch_typed(hipStream_t st, const u8 *const *d_seg_base, const long *d_seg_row0, int n_segs, int n_channels, const int *d_cols,
                 int n_cols, const void *d_taps, int n_taps, int q, long first_row, long k_begin, long k_end, long vb, long ve, void *d_out)
{
    int R, to, slab;
    dec_plan<F>(n_taps, q, &R, &to, &slab);
    const long n = k_end - k_begin;
    if (n <= 0) return MTS_OK;
    const long nt = (n + to - 1) / to;
    if (nt > 0x7fffffffl) { set_error("decimate: too many output tiles in one launch"); return MTS_E_ARG; }
    const dim3 grid((unsigned)nt, (unsigned)((n_cols + 63) / 64));
#define MTS_DEC_LAUNCH(RR)                                                                                                                \
    hipLaunchKernelGGL((k_decimate<T, F, RR>), grid, dim3(64 * DEC_WAVES), 0, st, d_seg_base, d_seg_row0, n_segs, n_channels, d_cols,   \
                       n_cols, (const F *)d_taps, n_taps, q, first_row, k_begin, k_end, vb, ve, to, slab, (F *)d_out)
    if (R == 8) MTS_DEC_LAUNCH(8);
    else if (R == 4) MTS_DEC_LAUNCH(4);
    else if (R == 2) MTS_DEC_LAUNCH(2);
    else MTS_DEC_LAUNCH(1);
#undef MTS_DEC_LAUNCH
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

template <typename T>
int launch_item(hipStream_t st, int out_itemsize, const u8 *const *b, const long *r0, int ns, int nc, const int *cols, int n_cols, const void *taps,
                int n_taps, int q, long first_row, long k_begin, long k_end, long vb, long ve, void *out)
{
    if (out_itemsize == 4) return launch_typed<T, float>(st, b, r0, ns, nc, cols, n_cols, taps, n_taps, q, first_row, k_begin, k_end, vb, ve, out);
    return launch_typed<T, double>(st, b, r0, ns, nc, cols, n_cols, taps, n_taps, q, first_row, k_begin, k_end, vb, ve, out);
}

}  // namespace

int launch_decimate(hipStream_t st, int itemsize, int flags, int out_itemsize, const u8 *const *d_seg_base, const long *d_seg_row0, int n_segs,
                    int n_channels, const int *d_cols, int n_cols, const void *d_taps, int n_taps, int q, long first_row, long k_begin,
                    long k_end, long valid_begin, long valid_end, void *d_out)
{
    if (out_itemsize != 4 && out_itemsize != 8) return MTS_E_ARG;
#define MTS_DEC_CASE(T) \
    return launch_item<T>(st, out_itemsize, d_seg_base, d_seg_row0, n_segs, n_channels, d_cols, n_cols, d_taps, n_taps, q, first_row, k_begin, k_end, valid_begin, valid_end, d_out)
    if (flags & MTS_FLAG_FLOAT) {
        if (itemsize == 4) MTS_DEC_CASE(float);
        if (itemsize == 8) MTS_DEC_CASE(double);
    } else if (flags & MTS_FLAG_UNSIGNED) {
        if (itemsize == 1) MTS_DEC_CASE(uint8_t);
        if (itemsize == 2) MTS_DEC_CASE(uint16_t);
        if (itemsize == 4) MTS_DEC_CASE(uint32_t);
        if (itemsize == 8) MTS_DEC_CASE(uint64_t);
    } else {
        if (itemsize == 1) MTS_DEC_CASE(int8_t);
        if (itemsize == 2) MTS_DEC_CASE(int16_t);
        if (itemsize == 4) MTS_DEC_CASE(int32_t);
        if (itemsize == 8) MTS_DEC_CASE(int64_t);
    }
#undef MTS_DEC_CASE
    return MTS_E_ARG;
}

}  // namespace mts
