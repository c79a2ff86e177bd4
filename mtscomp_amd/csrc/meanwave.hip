// Per-label sums of snippets in fixed point (mts_mean_waveforms, mts_dev_mean_waveforms).
//
// The filter is k_decimate with q = 1 (decimate.hip) into a float32 workspace z of file rows [ws_row0, ws_row0 + ws_rows) x n_cols,
// k_row_median (detect.hip) the reference; the kernel here works on that workspace, slab after slab (reduce.hip: mean_waveforms_run):
//   k_mean_waveforms  a segmented reduction.  The host has grouped the slab's events by label and cut every label's run into parts
//                   (MeanParts, reduce_plan.h).  One workgroup per (part, tile of the T * W entries of a snippet): a thread owns
//                   VEC adjacent entries of the flat index i = tau * W + w -- its (tau, w) do not depend on the event -- and walks
//                   the part's events, staged through LDS MEAN_BATCH at a time, with an int64 sum, an int32 count and a skip count
//                   in registers: d = (double)z[r, c] * (1 / resolution) (exact: a power of two), a NaN or |d| >= 2^42 is
//                   skipped, every other d adds rint(d) (ties to even) and 1.  An entry outside the recording, the workspace or
//                   [0, n_cols) issues no load and counts nowhere.  Then one 64-bit and one 32-bit integer atomic add per entry with
//                   a count; the skip counts of a wave are added up and go out as one atomic add.
//                   Integer addition is associative: the same bytes whatever ran when, which part an event fell in, and however
//                   the slabs were cut -- the one kernel of the family that may use atomics.  No float atomics, no protocol
//                   between workgroups; the launches of successive slabs follow each other in stream order.
//                   VEC = 4: the four entries of a thread are adjacent in z when they lie in one row of the snippet, or when the
//                   snippet is as wide as z (then all four are valid only for ev_col0 == 0, and row follows row); they are then
//                   one 16-byte load from an address that is a multiple of 4 bytes, which global loads take.  Otherwise, and
//                   when one of the four is clipped, they are loaded one by one, as with VEC = 1.
#include "common.h"
#include "reduce_plan.h"

namespace mts {

namespace {

constexpr int MEAN_THREADS = 256;
constexpr int MEAN_BATCH = 256;                                    // events staged in LDS at a time
constexpr int MEAN_VEC_MIN = 4 * MEAN_THREADS;                     // snippets of fewer entries take the scalar path: more workgroups

typedef float mean_f4 __attribute__((ext_vector_type(4), aligned(4)));

// rint(d) as an integer for |d| < 2^51: d + 1.5 * 2^52 lies in [2^52, 2^53), where doubles are the integers -- the addition rounds to
// nearest, ties to even -- and has the exponent of 1.5 * 2^52, so the difference of the bit patterns is the rounded value
__device__ __forceinline__ long long mean_rint(double d)
{
    const double magic = 0x1.8p52;
    return __double_as_longlong(d + magic) - __double_as_longlong(magic);
}

}  // namespace

// blockIdx.x: the part parts[blockIdx.x]; blockIdx.y: the tile of MEAN_THREADS * VEC entries.  Rows [row_lo, row_hi): the recording ∩
// the workspace.  N = T * W
template <int VEC>
__global__ __launch_bounds__(MEAN_THREADS) void k_mean_waveforms(const float *__restrict__ z, long ws_row0, int n_cols, long row_lo, long row_hi,
                                                                const long *__restrict__ ev_row, const int *__restrict__ ev_col0,
                                                                const long *__restrict__ perm, const MeanPart *__restrict__ parts, int before,
                                                                int N, int W, double inv_res, unsigned long long *sum, int *count,
                                                                unsigned long long *skipped)
{
    __shared__ long s_r0[MEAN_BATCH];
    __shared__ int s_c0[MEAN_BATCH];
    const MeanPart P = parts[blockIdx.x];
    const int i0 = ((int)blockIdx.y * MEAN_THREADS + (int)threadIdx.x) * VEC;
    int tau[VEC], w[VEC];
    bool live[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) {
        live[k] = i0 + k < N;
        tau[k] = live[k] ? (i0 + k) / W : 0;
        w[k] = live[k] ? i0 + k - tau[k] * W : 0;
    }
    const bool adjacent = VEC == 4 && live[VEC - 1] && (tau[VEC - 1] == tau[0] || W == n_cols);
    long long acc[VEC];
    int cnt[VEC];
    u32 skip = 0;
#pragma unroll
    for (int k = 0; k < VEC; k++) { acc[k] = 0; cnt[k] = 0; }
    for (int b0 = 0; b0 < P.count; b0 += MEAN_BATCH) {              // (uniform: every thread of the workgroup takes every batch)
        const int nb = P.count - b0 < MEAN_BATCH ? P.count - b0 : MEAN_BATCH;
        if ((int)threadIdx.x < nb) {
            const long e = perm[P.first + b0 + (long)threadIdx.x];
            s_r0[threadIdx.x] = ev_row[e] - (long)before;          // the file row of tau = 0
            s_c0[threadIdx.x] = ev_col0[e];
        }
        __syncthreads();
        if (live[0]) {
            for (int b = 0; b < nb; b++) {
                const long r0 = s_r0[b], c0 = (long)s_c0[b];
                bool ok[VEC], all = true;
                float v[VEC];
#pragma unroll
                for (int k = 0; k < VEC; k++) {
                    const long r = r0 + tau[k], c = c0 + w[k];
                    ok[k] = live[k] && r >= row_lo && r < row_hi && c >= 0 && c < (long)n_cols;
                    all = all && ok[k];
                    v[k] = 0.0f;
                }
                if (VEC == 4 && adjacent && all) {
                    const mean_f4 q = *(const mean_f4 *)(z + (u64)(r0 + tau[0] - ws_row0) * (u64)n_cols + (u64)(c0 + w[0]));
                    v[0] = q.x; v[1 % VEC] = q.y; v[2 % VEC] = q.z; v[3 % VEC] = q.w;
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; k++)
                        if (ok[k]) v[k] = z[(u64)(r0 + tau[k] - ws_row0) * (u64)n_cols + (u64)(c0 + w[k])];
                }
#pragma unroll
                for (int k = 0; k < VEC; k++) {
                    if (!ok[k]) continue;
                    const double d = (double)v[k] * inv_res;
                    if (__builtin_fabs(d) < 0x1p42) { acc[k] += mean_rint(d); cnt[k]++; }      // (false for a NaN)
                    else skip++;
                }
            }
        }
        __syncthreads();
    }
    const u64 at = (u64)P.label * (u64)N + (u64)i0;
#pragma unroll
    for (int k = 0; k < VEC; k++)
        if (cnt[k]) {
            atomicAdd(sum + at + k, (unsigned long long)acc[k]);
            atomicAdd(count + at + k, cnt[k]);
        }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) skip += (u32)__shfl_xor((int)skip, d, 64);
    if ((threadIdx.x & 63) == 0 && skip) atomicAdd(skipped + P.label, (unsigned long long)skip);
}

int launch_mean_waveforms(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, long vb, long ve, const long *d_ev_row,
                          const int *d_ev_col0, const long *d_perm, const MeanPart *d_parts, long n_parts, int before, int after, int width,
                          double resolution, long long *d_sum, int *d_count, long *d_skipped)
{
    if (n_parts <= 0) return MTS_OK;
    const long T = (long)before + after;
    if (before < 0 || after < 0 || T < 1 || T > MTS_WAVEFORMS_MAX_ROWS || width < 1 || width > MTS_WAVEFORMS_MAX_WIDTH || n_cols < 1 || ws_rows < 0 ||
        !(resolution > 0) || !d_sum || !d_count || !d_skipped) {
        set_error("mean_waveforms: snippet of %ld rows x %d positions (1 .. %d, 1 .. %d)", T, width, MTS_WAVEFORMS_MAX_ROWS, MTS_WAVEFORMS_MAX_WIDTH);
        return MTS_E_ARG;
    }
    // a row outside the workspace is never loaded: the slabs (SnippetPlan) hold every row of the recording that their events read
    const long row_lo = vb > ws_row0 ? vb : ws_row0, row_hi = ve < ws_row0 + ws_rows ? ve : ws_row0 + ws_rows;
    const int N = (int)(T * width);
    const bool vec = N >= MEAN_VEC_MIN;
    const unsigned tiles = (unsigned)((N + MEAN_THREADS * (vec ? 4 : 1) - 1) / (MEAN_THREADS * (vec ? 4 : 1)));     // (<= 16384)
    for (long p = 0; p < n_parts;) {
        const long n = n_parts - p < (1l << 30) ? n_parts - p : (1l << 30);
        if (vec)
            hipLaunchKernelGGL(k_mean_waveforms<4>, dim3((unsigned)n, tiles), dim3(MEAN_THREADS), 0, st, d_z, ws_row0, n_cols, row_lo, row_hi, d_ev_row,
                               d_ev_col0, d_perm, d_parts + p, before, N, width, 1.0 / resolution, (unsigned long long *)d_sum, d_count,
                               (unsigned long long *)d_skipped);
        else
            hipLaunchKernelGGL(k_mean_waveforms<1>, dim3((unsigned)n, tiles), dim3(MEAN_THREADS), 0, st, d_z, ws_row0, n_cols, row_lo, row_hi, d_ev_row,
                               d_ev_col0, d_perm, d_parts + p, before, N, width, 1.0 / resolution, (unsigned long long *)d_sum, d_count,
                               (unsigned long long *)d_skipped);
        p += n;
    }
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace mts
