// Snippets projected on a temporal basis (mts_waveform_features, mts_dev_waveform_features).
//
// The filter is k_decimate with q = 1 (decimate.hip) into a float32 workspace z of file rows [ws_row0, ws_row0 + ws_rows) x n_cols,
// k_row_median (detect.hip) the reference; the kernel here works on that workspace, slab after slab (reduce.hip: waveform_features_run):
//   k_waveform_features  the work items are the flat pairs i = (event of the slab) * W + w, one thread each, so that a 17-wide snippet
//                   fills the lanes of a wave: adjacent lanes read adjacent positions of one row of z and store adjacent entries of
//                   features[e, p, .].  A thread owns its pair's chains from +0 to their stores: it walks tau = 0 .. T - 1 in
//                   ascending order with FEAT_PB accumulators in registers, acc[k] = fmaf(z[r0 + tau, c], basis[p0 + k, tau], acc[k]),
//                   one explicit fmaf each (no contraction, no fast-math, zero basis entries are not skipped: inf * 0 is NaN), and
//                   repeats the walk for the next block of components.  A NaN result is stored as 0x7fc00000.  No atomics and no
//                   cross-lane step: the bytes depend on nothing but z and the basis.
//                   A pair whose column position lies outside [0, n_cols), or any of whose T rows lies outside the recording, is NaN
//                   in all P components by the definition (one fill entry makes the chain NaN): it stores the fill bits and
//                   issues no load.
//                   LDS: the basis, staged once per workgroup in the layout the host repacked it to (features_basis_image, common.h): blocks of
//                   FEAT_PB components, [tau][k] inside a block, so that every lane reads the same address at a step -- a broadcast
//                   -- and the components of a block are one wide read; the last block holds the P % FEAT_PB components that
//                   remain, [tau][P % FEAT_PB], so the image is P * T entries whatever P (a padded [tau][P] image would pass 32 KiB
//                   for a long T with P = 1).  And the (row - before, col0) of the at most FEAT_THREADS events that the workgroup's
//                   pairs belong to, staged under the same barrier.
#include "common.h"

namespace mts {

namespace {

constexpr int FEAT_THREADS = 256;                                  // pairs of a workgroup; its events are at most as many (W = 1)
constexpr u32 FEAT_FILL = 0x7fc00000u;

// the chains of NB components [p0, p0 + NB) of one pair.  sb: the block's image, [tau][NB]; zp: z at (r0, c)
template <int NB>
__device__ __forceinline__ void feat_walk(const float *__restrict__ zp, u64 n_cols, int T, const float *sb, float *__restrict__ out, u64 W)
{
    float acc[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) acc[k] = 0.0f;
#pragma unroll 4
    for (int tau = 0; tau < T; tau++) {
        const float v = zp[(u64)tau * n_cols];
        float b[NB];
        if constexpr (NB % 4 == 0) {
#pragma unroll
            for (int k = 0; k < NB; k += 4) {
                const float4 q = *(const float4 *)(sb + tau * NB + k);
                b[k] = q.x; b[k + 1] = q.y; b[k + 2] = q.z; b[k + 3] = q.w;
            }
        } else if constexpr (NB % 2 == 0) {
#pragma unroll
            for (int k = 0; k < NB; k += 2) {
                const float2 q = *(const float2 *)(sb + tau * NB + k);
                b[k] = q.x; b[k + 1] = q.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NB; k++) b[k] = sb[tau * NB + k];
        }
#pragma unroll
        for (int k = 0; k < NB; k++) acc[k] = __builtin_fmaf(v, b[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < NB; k++) out[(u64)k * W] = acc[k] == acc[k] ? acc[k] : __uint_as_float(FEAT_FILL);
}

}  // namespace

// pairs [blockIdx.x * FEAT_THREADS, ...) of the events [e0, e0 + n_ev); rows [row_lo, row_hi): the recording ∩ the workspace.
// Dynamic LDS: the basis image, P * T floats
__global__ __launch_bounds__(FEAT_THREADS) void k_waveform_features(const float *__restrict__ z, long ws_row0, int n_cols, long row_lo, long row_hi,
                                                                   const long *__restrict__ ev_row, const int *__restrict__ ev_col0, long e0,
                                                                   long n_ev, int before, int T, int W, int P,
                                                                   const float *__restrict__ basis, float *__restrict__ feat)
{
    extern __shared__ float4 s_dyn[];                              // (float4: the base is 16-byte aligned for the wide reads)
    __shared__ long s_r0[FEAT_THREADS];
    __shared__ int s_c0[FEAT_THREADS];
    float *s_basis = (float *)s_dyn;
    const long n_pairs = n_ev * (long)W;
    const long i0 = (long)blockIdx.x * FEAT_THREADS;               // the workgroup's first pair; i0 < n_pairs
    const long i1 = i0 + FEAT_THREADS < n_pairs ? i0 + FEAT_THREADS : n_pairs;
    const long b0 = i0 / W, b1 = (i1 - 1) / W + 1;                 // its events [b0, b1) of the slab: at most FEAT_THREADS
    for (int k = (int)threadIdx.x; k < P * T; k += FEAT_THREADS) s_basis[k] = basis[k];
    if ((long)threadIdx.x < b1 - b0) {
        const long e = e0 + b0 + (long)threadIdx.x;
        s_r0[threadIdx.x] = ev_row[e] - (long)before;              // the file row of tau = 0
        s_c0[threadIdx.x] = ev_col0[e];
    }
    __syncthreads();
    const long i = i0 + (long)threadIdx.x;
    if (i >= n_pairs) return;
    const long b = i / W;
    const int w = (int)(i - b * W);
    const long r0 = s_r0[b - b0], c = (long)s_c0[b - b0] + w;
    float *out = feat + ((u64)(e0 + b) * (u64)P) * (u64)W + (u64)w;      // features[e, 0, w]; component p lies p * W further
    if (c < 0 || c >= (long)n_cols || r0 < row_lo || r0 + T > row_hi) {
        for (int p = 0; p < P; p++) out[(u64)p * (u64)W] = __uint_as_float(FEAT_FILL);
        return;
    }
    const float *zp = z + (u64)(r0 - ws_row0) * (u64)n_cols + (u64)c;
    int p = 0;
    for (; p + FEAT_PB <= P; p += FEAT_PB) feat_walk<FEAT_PB>(zp, (u64)n_cols, T, s_basis + p * T, out + (u64)p * (u64)W, (u64)W);
    const float *sb = s_basis + p * T;
    float *o = out + (u64)p * (u64)W;
    static_assert(FEAT_PB == 8, "the remainders below are those of blocks of 8");
    switch (P - p) {
    case 1: feat_walk<1>(zp, (u64)n_cols, T, sb, o, (u64)W); break;
    case 2: feat_walk<2>(zp, (u64)n_cols, T, sb, o, (u64)W); break;
    case 3: feat_walk<3>(zp, (u64)n_cols, T, sb, o, (u64)W); break;
    case 4: feat_walk<4>(zp, (u64)n_cols, T, sb, o, (u64)W); break;
    case 5: feat_walk<5>(zp, (u64)n_cols, T, sb, o, (u64)W); break;
    case 6: feat_walk<6>(zp, (u64)n_cols, T, sb, o, (u64)W); break;
    case 7: feat_walk<7>(zp, (u64)n_cols, T, sb, o, (u64)W); break;
    default: break;
    }
}

int launch_waveform_features(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, long vb, long ve, const long *d_ev_row,
                             const int *d_ev_col0, long e0, long e1, int before, int after, int width, int n_comp, const float *d_basis,
                             float *d_feat)
{
    if (e1 <= e0) return MTS_OK;
    const long T = (long)before + after;
    if (before < 0 || after < 0 || T < 1 || T > MTS_WAVEFORMS_MAX_ROWS || width < 1 || width > MTS_WAVEFORMS_MAX_WIDTH || n_cols < 1 || ws_rows < 0 ||
        n_comp < 1 || n_comp > MTS_FEATURES_MAX_COMPONENTS || (long)n_comp * T > MTS_FEATURES_MAX_BASIS || !d_basis || !d_feat) {
        set_error("waveform_features: snippet of %ld rows x %d positions (1 .. %d, 1 .. %d) on %d components (1 .. %d, %d entries)", T, width,
                  MTS_WAVEFORMS_MAX_ROWS, MTS_WAVEFORMS_MAX_WIDTH, n_comp, MTS_FEATURES_MAX_COMPONENTS, MTS_FEATURES_MAX_BASIS);
        return MTS_E_ARG;
    }
    // a row outside the workspace is never loaded: the slabs (SnippetPlan) hold every row of the recording that their events read
    const long row_lo = vb > ws_row0 ? vb : ws_row0, row_hi = ve < ws_row0 + ws_rows ? ve : ws_row0 + ws_rows;
    const size_t lds = ((size_t)n_comp * (size_t)T * 4 + 15) & ~(size_t)15;
    const long per = (1l << 30) / width;                           // events of a launch: fewer than 2^30 pairs, 2^22 workgroups
    for (long e = e0; e < e1;) {
        const long n = e1 - e < per ? e1 - e : per;
        const unsigned blocks = (unsigned)((n * width + FEAT_THREADS - 1) / FEAT_THREADS);
        hipLaunchKernelGGL(k_waveform_features, dim3(blocks), dim3(FEAT_THREADS), lds, st, d_z, ws_row0, n_cols, row_lo, row_hi, d_ev_row, d_ev_col0, e,
                           n, before, (int)T, width, n_comp, d_basis, d_feat);
        e += n;
    }
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace mts
