// Snippets around events and their extrema (mts_waveforms, mts_dev_waveforms).
//
// The filter is k_decimate with q = 1 (decimate.hip) into a float32 workspace z of file rows [ws_row0, ws_row0 + ws_rows) x n_cols,
// k_row_median (detect.hip) the reference; the kernel here works on that workspace, slab after slab (reduce.hip: waveforms_run):
//   k_waveforms     one workgroup of 4 waves per event e: wave[e, tau, w] = z[row[e] - before + tau, col0[e] + w] for the flat index
//                   i = tau * W + w < T * W, the lanes running over i so that the stores of wave[e] are contiguous (four entries per
//                   lane and store when T * W and the buffer allow it).  An entry whose row lies outside the recording or whose column
//                   position lies outside [0, n_cols) is the fill value, the quiet NaN 0x7fc00000, and no load is issued for it; a
//                   NaN of the data is stored as the same bits (what sign and payload the filter's or the median's arithmetic
//                   gives a NaN is not part of the definition).  Each lane keeps (min, its index) and (max, its index) over its
//                   entries that are not NaN; its indices ascend, so a strict comparison keeps the first.  Lanes, then waves
//                   (through LDS) are combined by the lexicographic order on (value, index): the first index of the extreme value
//                   wins whatever the order of the combination, and -0 == +0, so the first of them is returned with its own bits.
//                   No atomics: the same bytes whatever ran when.
#include "common.h"

namespace mts {

namespace {

constexpr int WAV_WAVES = 4;
constexpr int WAV_THREADS = 64 * WAV_WAVES;
constexpr u32 WAV_FILL = 0x7fc00000u;

struct Ext { float v; int i; };                                    // i < 0: none yet

// b replaces a when it is the smaller (SIGN < 0) or larger (SIGN > 0) value, or the same value at an earlier index
template <int SIGN>
__device__ __forceinline__ Ext ext_pick(Ext a, Ext b)
{
    if (b.i < 0) return a;
    if (a.i < 0) return b;
    const bool better = SIGN < 0 ? b.v < a.v : b.v > a.v;
    return (better || (b.v == a.v && b.i < a.i)) ? b : a;
}

template <int SIGN>
__device__ __forceinline__ Ext ext_wave(Ext a)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        Ext b;
        b.v = __uint_as_float((u32)__shfl_xor((int)__float_as_uint(a.v), d, 64));
        b.i = __shfl_xor(a.i, d, 64);
        a = ext_pick<SIGN>(a, b);
    }
    return a;
}

}  // namespace

// event e0 + blockIdx.x; rows [row_lo, row_hi): the recording ∩ the workspace.  VEC: entries per lane and store (4: T * W is a
// multiple of 4 and wave is 16-byte aligned, so every event's snippet is)
template <int VEC>
__global__ __launch_bounds__(WAV_THREADS) void k_waveforms(const float *__restrict__ z, long ws_row0, int n_cols, long row_lo, long row_hi,
                                                          const long *__restrict__ ev_row, const int *__restrict__ ev_col0, long e0, int before,
                                                          int T, int W, float *__restrict__ wave, float *__restrict__ o_min,
                                                          int *__restrict__ o_argmin, float *__restrict__ o_max, int *__restrict__ o_argmax)
{
    __shared__ Ext s_lo[WAV_WAVES], s_hi[WAV_WAVES];
    const long e = e0 + (long)blockIdx.x;
    const long r0 = ev_row[e] - (long)before;                      // the file row of tau = 0
    const long c0 = (long)ev_col0[e];
    const int N = T * W;
    float *out = wave ? wave + (u64)e * (u64)N : nullptr;
    Ext lo = {0.0f, -1}, hi = {0.0f, -1};
    for (int i = (int)threadIdx.x * VEC; i < N; i += WAV_THREADS * VEC) {
        int tau = i / W, w = i - tau * W;
        float v[VEC];
#pragma unroll
        for (int k = 0; k < VEC; k++) {
            const long r = r0 + tau, c = c0 + w;
            v[k] = __uint_as_float(WAV_FILL);
            if (r >= row_lo && r < row_hi && c >= 0 && c < (long)n_cols) v[k] = z[(u64)(r - ws_row0) * (u64)n_cols + (u64)c];
            if (v[k] == v[k]) {
                if (lo.i < 0 || v[k] < lo.v) lo = {v[k], i + k};
                if (hi.i < 0 || v[k] > hi.v) hi = {v[k], i + k};
            } else v[k] = __uint_as_float(WAV_FILL);              // (a NaN of the data: stored as the fill's bits)
            if (++w == W) { w = 0; tau++; }
        }
        if (out) {
            if (VEC == 4) *(float4 *)(out + i) = make_float4(v[0], v[1 % VEC], v[2 % VEC], v[3 % VEC]);
            else out[i] = v[0];
        }
    }
    lo = ext_wave<-1>(lo);
    hi = ext_wave<1>(hi);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { s_lo[wv] = lo; s_hi[wv] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < WAV_WAVES; k++) { lo = ext_pick<-1>(lo, s_lo[k]); hi = ext_pick<1>(hi, s_hi[k]); }
        o_min[e] = lo.i < 0 ? __uint_as_float(WAV_FILL) : lo.v;
        o_argmin[e] = lo.i;
        o_max[e] = hi.i < 0 ? __uint_as_float(WAV_FILL) : hi.v;
        o_argmax[e] = hi.i;
    }
}

int launch_waveforms(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, long vb, long ve, const long *d_ev_row,
                     const int *d_ev_col0, long e0, long e1, int before, int after, int width, float *d_wave, float *d_min, int *d_argmin,
                     float *d_max, int *d_argmax)
{
    if (e1 <= e0) return MTS_OK;
    const long T = (long)before + after;
    if (before < 0 || after < 0 || T < 1 || T > MTS_WAVEFORMS_MAX_ROWS || width < 1 || width > MTS_WAVEFORMS_MAX_WIDTH || n_cols < 1 || ws_rows < 0) {
        set_error("waveforms: snippet of %ld rows x %d positions (1 .. %d, 1 .. %d)", T, width, MTS_WAVEFORMS_MAX_ROWS, MTS_WAVEFORMS_MAX_WIDTH);
        return MTS_E_ARG;
    }
    // a row outside the workspace is never loaded: the slabs (SnippetPlan) hold every row of the recording that their events read
    const long row_lo = vb > ws_row0 ? vb : ws_row0, row_hi = ve < ws_row0 + ws_rows ? ve : ws_row0 + ws_rows;
    const bool vec = (T * width) % 4 == 0 && ((uintptr_t)d_wave & 15) == 0;
    for (long e = e0; e < e1;) {
        const long n = e1 - e < (1l << 30) ? e1 - e : (1l << 30);
        if (vec)
            hipLaunchKernelGGL(k_waveforms<4>, dim3((unsigned)n), dim3(WAV_THREADS), 0, st, d_z, ws_row0, n_cols, row_lo, row_hi, d_ev_row, d_ev_col0, e,
                               before, (int)T, width, d_wave, d_min, d_argmin, d_max, d_argmax);
        else
            hipLaunchKernelGGL(k_waveforms<1>, dim3((unsigned)n), dim3(WAV_THREADS), 0, st, d_z, ws_row0, n_cols, row_lo, row_hi, d_ev_row, d_ev_col0, e,
                               before, (int)T, width, d_wave, d_min, d_argmin, d_max, d_argmax);
        e += n;
    }
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace mts
