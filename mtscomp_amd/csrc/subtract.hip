// Template subtraction on filtered rows (mts_residual, mts_match_residual and their device variants).
//
// The filter is k_decimate with q = 1 (decimate.hip) into a float32 workspace z of file rows [ws_row0, ws_row0 + ws_rows) x n_cols,
// k_row_median (detect.hip) the reference; the kernel here works on that workspace, slab after slab (reduce.hip: residual_run,
// tmatch_run):
//   k_subtract      a gather: every (row, column) of the slab belongs to one thread (items of VEC = 4 adjacent columns when n_cols and
//                   the three addresses allow 16-byte accesses, of one otherwise; SUB_ITEMS items a thread, a workgroup's stride
//                   apart), which keeps its accumulators in registers and walks the events that cover its row in list order:
//                   acc = fmaf(-amplitude[e], K[template[e], t - row[e] + before, j], acc).
//                   The events arrive sorted by row, so those that cover the rows of a workgroup's tile are one range of the list:
//                   two threads find its ends by binary search, and the range goes through LDS SUB_BATCH events at a time -- an
//                   overlap of any depth needs no cap.  An event that does not cover the thread's row issues no step (a masked step
//                   with a zero amplitude would turn a -0 into +0); zero template entries are not skipped.  The templates are the
//                   plain (K, T, n_cols) copy: the lanes run over the columns and load them coalesced.  A NaN is stored as 0x7fc00000.
//                   No atomics and no float adds that race: the same bytes whatever ran when.
#include "common.h"

namespace mts {

namespace {

constexpr int SUB_THREADS = 256;
constexpr int SUB_ITEMS = 4;                                       // items of a thread
constexpr int SUB_BATCH = 256;                                     // events staged in LDS at a time
constexpr u32 SUB_NAN = 0x7fc00000u;

}  // namespace

// A workgroup's tile is SUB_THREADS * SUB_ITEMS items of VEC adjacent columns, item i = columns [c, c + VEC) of slab row i / G, c = i % G *
// VEC, G = n_cols / VEC; a thread owns the items i0 + j * SUB_THREADS + threadIdx.x, j < SUB_ITEMS, so that a wave's accesses are
// contiguous and one search and one pass over the staged events serve SUB_ITEMS items.  out may be z (in place)
template <int VEC>
__global__ __launch_bounds__(SUB_THREADS) void k_subtract(const float *z, long ws_row0, u64 n_items, int n_cols, int G, const long *__restrict__ ev_row,
                                                         const int *__restrict__ ev_tpl, const float *__restrict__ ev_namp, long n_ev,
                                                         const float *__restrict__ tpl, int T, int before, float *out)
{
#pragma clang fp contract(off)
    __shared__ long s_row[SUB_BATCH];
    __shared__ int s_tpl[SUB_BATCH];
    __shared__ float s_namp[SUB_BATCH];
    __shared__ long s_range[2];
    const u64 i0 = (u64)blockIdx.x * (SUB_THREADS * SUB_ITEMS);
    const u64 i_last = i0 + SUB_THREADS * SUB_ITEMS - 1 < n_items - 1 ? i0 + SUB_THREADS * SUB_ITEMS - 1 : n_items - 1;
    // the events that cover a row of the tile: ev_row - before <= t < ev_row - before + T for a t of [t_first, t_last]
    if (threadIdx.x < 2) {
        const long t_first = ws_row0 + (long)(i0 / (u64)G), t_last = ws_row0 + (long)(i_last / (u64)G);
        // [0]: the first event with row >= t_first + before - T + 1; [1]: the first with row > t_last + before
        const long key = threadIdx.x == 0 ? t_first + (long)before - (long)T + 1 : t_last + (long)before + 1;
        long lo = 0, hi = n_ev;
        while (lo < hi) {
            const long mid = lo + ((hi - lo) >> 1);
            if (ev_row[mid] < key) lo = mid + 1; else hi = mid;
        }
        s_range[threadIdx.x] = lo;
    }
    __syncthreads();
    const long e_lo = s_range[0], e_hi = s_range[1];
    bool live[SUB_ITEMS];
    long t[SUB_ITEMS];
    int c[SUB_ITEMS];
    u64 at[SUB_ITEMS];
    float acc[SUB_ITEMS][VEC];
#pragma unroll
    for (int j = 0; j < SUB_ITEMS; j++) {
        const u64 i = i0 + (u64)(j * SUB_THREADS) + threadIdx.x;
        live[j] = i < n_items;
        const u64 r = live[j] ? i / (u64)G : 0;
        c[j] = live[j] ? (int)(i - r * (u64)G) * VEC : 0;
        t[j] = ws_row0 + (long)r;
        at[j] = r * (u64)n_cols + (u64)c[j];
#pragma unroll
        for (int k = 0; k < VEC; k++) acc[j][k] = 0.0f;
        if (live[j]) {
            if (VEC == 4) {
                const float4 v = *(const float4 *)(z + at[j]);
                acc[j][0] = v.x; acc[j][1 % VEC] = v.y; acc[j][2 % VEC] = v.z; acc[j][3 % VEC] = v.w;
            } else acc[j][0] = z[at[j]];
        }
    }
    for (long e0 = e_lo; e0 < e_hi; e0 += SUB_BATCH) {             // (uniform: every thread of the workgroup takes every batch)
        const int nb = e_hi - e0 < (long)SUB_BATCH ? (int)(e_hi - e0) : SUB_BATCH;
        if ((int)threadIdx.x < nb) {
            s_row[threadIdx.x] = ev_row[e0 + threadIdx.x];
            s_tpl[threadIdx.x] = ev_tpl[e0 + threadIdx.x];
            s_namp[threadIdx.x] = ev_namp[e0 + threadIdx.x];
        }
        __syncthreads();
        for (int b = 0; b < nb; b++) {
            const long first = s_row[b] - (long)before;            // the file row of the event's tau = 0
            const float na = s_namp[b];
            const float *kb = tpl + (u64)s_tpl[b] * (u64)T * (u64)n_cols;
#pragma unroll
            for (int j = 0; j < SUB_ITEMS; j++) {
                const long tau = t[j] - first;
                if (!live[j] || tau < 0 || tau >= (long)T) continue;   // (no step at all)
                const float *kp = kb + (u64)tau * (u64)n_cols + (u64)c[j];
                if (VEC == 4) {
                    const float4 kv = *(const float4 *)kp;
                    acc[j][0] = __builtin_fmaf(na, kv.x, acc[j][0]); acc[j][1 % VEC] = __builtin_fmaf(na, kv.y, acc[j][1 % VEC]);
                    acc[j][2 % VEC] = __builtin_fmaf(na, kv.z, acc[j][2 % VEC]); acc[j][3 % VEC] = __builtin_fmaf(na, kv.w, acc[j][3 % VEC]);
                } else acc[j][0] = __builtin_fmaf(na, kp[0], acc[j][0]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < SUB_ITEMS; j++) {
        if (!live[j]) continue;
#pragma unroll
        for (int k = 0; k < VEC; k++)
            if (!(acc[j][k] == acc[j][k])) acc[j][k] = __uint_as_float(SUB_NAN);
        if (VEC == 4) *(float4 *)(out + at[j]) = make_float4(acc[j][0], acc[j][1 % VEC], acc[j][2 % VEC], acc[j][3 % VEC]);
        else out[at[j]] = acc[j][0];
    }
}

int launch_subtract(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, const long *d_ev_row, const int *d_ev_tpl,
                    const float *d_ev_namp, long n_ev, const float *d_tpl, int T, int before, float *d_out)
{
    if (ws_rows <= 0) return MTS_OK;
    if (n_cols < 1 || n_ev < 0 || T < 1 || before < 0 || before > T || (n_ev && (!d_ev_row || !d_ev_tpl || !d_ev_namp || !d_tpl))) {
        set_error("subtract: %ld events of %d template rows over %d columns invalid", n_ev, T, n_cols);
        return MTS_E_ARG;
    }
    const bool vec = n_cols % 4 == 0 && (((uintptr_t)d_z | (uintptr_t)d_out | (uintptr_t)d_tpl) & 15) == 0;
    const int G = vec ? n_cols / 4 : n_cols;
    const u64 n_items = (u64)ws_rows * (u64)G;
    const u64 n_blocks = (n_items + SUB_THREADS * SUB_ITEMS - 1) / (SUB_THREADS * SUB_ITEMS);
    if (n_blocks >= (1ull << 31)) { set_error("subtract: a slab of %ld rows x %d columns is too large", ws_rows, n_cols); return MTS_E_ARG; }
    if (vec)
        hipLaunchKernelGGL(k_subtract<4>, dim3((unsigned)n_blocks), dim3(SUB_THREADS), 0, st, d_z, ws_row0, n_items, n_cols, G, d_ev_row, d_ev_tpl,
                           d_ev_namp, n_ev, d_tpl, T, before, d_out);
    else
        hipLaunchKernelGGL(k_subtract<1>, dim3((unsigned)n_blocks), dim3(SUB_THREADS), 0, st, d_z, ws_row0, n_items, n_cols, G, d_ev_row, d_ev_tpl,
                           d_ev_namp, n_ev, d_tpl, T, before, d_out);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace mts
