// Spike positions and channel amplitudes from the snippets (mts_localize, mts_dev_localize).
//
// The filter is k_decimate with q = 1 (decimate.hip) into a float32 workspace z of file rows [ws_row0, ws_row0 + ws_rows) x n_cols,
// k_row_median (detect.hip) the reference; the kernel here works on that workspace, slab after slab (reduce.hip: localize_run).
// The definition, all float32 and bit for bit, with s[e, tau, w] the entry that mts_waveforms returns (fill and NaN entries alike
// the quiet NaN 0x7fc00000):
//   1. column extrema  over the entries s[e, tau, w], tau = 0 .. T - 1, that are not NaN: lo the first minimum and hi the first
//                   maximum, each with its own bits (-0 == +0, so the first wins, as in k_waveforms).  A column without such an
//                   entry has none.
//   2. amplitude    a[e, w] = hi - lo (LOC_PTP, one subtraction), -lo (LOC_NEG, an exact negation: +0 gives -0), hi (LOC_POS), the
//                   first maximum of fabsf(entry) (LOC_ABS); 0x7fc00000 for a column without extrema and for a NaN result
//                   (inf - inf).
//   3. weight       g[e, w] = a[e, w] if a[e, w] > 0, else +0 (NaN, negative and zero amplitudes give +0; +inf stays).
//   4. sums         one chain per event over w = 0 .. W - 1 in ascending order, c = col0[e] + w, a w with c outside [0, n_cols)
//                   left out:  weight = weight + g[e, w] (one addition);  moment[d] = fmaf(g[e, w], positions[c, d], moment[d])
//                   (one explicit fmaf; no contraction is relied on), both from +0; a NaN result is stored as 0x7fc00000.
//                   Skipping a w with g = +0 yields the same bits: the positions are finite and the chains start at +0, so such a
//                   step adds +-0 to an accumulator that is never -0 (and leaves an inf or a NaN what it is).  The kernel skips
//                   them, which also covers every c outside the selection (its a is the NaN): no position is loaded for it.
//   5. best[e]      the lowest w whose a[e, w] is the largest among those that are not NaN (-0 == +0); -1 when there is none.
// No division and no reciprocal: location = moment / weight is formed on the host.
//   k_localize      a workgroup of LOC_THREADS threads owns whole events: LOC_THREADS / W of them for W <= LOC_THREADS (thread t has
//                   event t / W of the workgroup and position t % W; the threads beyond the last whole event idle), one event whose
//                   positions the threads stride over for wider snippets.  A thread walks its column's tau upwards with lo, hi and
//                   the largest fabsf in registers -- adjacent lanes read adjacent columns of one row of z, as in
//                   k_waveform_features; strict comparisons keep the first extremum; a column position outside [0, n_cols) issues
//                   no load and a row outside [row_lo, row_hi) is skipped -- and writes a to out_amp (when given) and to LDS, at
//                   an odd stride per event so that the chains' reads do not all hit one bank when W is a power of two.  After one
//                   barrier thread k < (the workgroup's events) walks event k's w upwards through steps 3 - 5 and stores weight,
//                   moment[0 .. D) and best.  One thread owns an event's chain from +0 to its store, no atomics, no cross-lane
//                   arithmetic: the bytes depend on nothing but z and the positions.
#include "common.h"

namespace mts {

namespace {

constexpr int LOC_THREADS = 256;
constexpr int LOC_LDS = MTS_WAVEFORMS_MAX_WIDTH + 1;               // floats: one event of 1024 positions at stride 1025; for W <= 256,
                                                                   // (256 / W) * (W | 1) <= 384
constexpr u32 LOC_FILL = 0x7fc00000u;

}  // namespace

// events [e0 + blockIdx.x * G, ...) of [e0, e0 + n_ev), G = max(1, LOC_THREADS / W); rows [row_lo, row_hi): the recording ∩ the workspace
__global__ __launch_bounds__(LOC_THREADS) void k_localize(const float *__restrict__ z, long ws_row0, int n_cols, long row_lo, long row_hi,
                                                         const long *__restrict__ ev_row, const int *__restrict__ ev_col0, long e0, long n_ev,
                                                         int before, int T, int W, int G, int mode, int D, const float *__restrict__ pos,
                                                         float *__restrict__ amp, float *__restrict__ o_weight, float *__restrict__ o_moment,
                                                         int *__restrict__ o_best)
{
    __shared__ float s_amp[LOC_LDS];
    const int S = W | 1;                                           // the LDS stride of an event: odd
    const int t = (int)threadIdx.x;
    const int k = t / W;                                           // the thread's event of the workgroup (0 for W > LOC_THREADS)
    const long b0 = (long)blockIdx.x * G;                          // the workgroup's first event of the launch; b0 < n_ev
    if (k < G && b0 + k < n_ev) {
        const long e = e0 + b0 + k;
        const long r0 = ev_row[e] - (long)before;                  // the file row of tau = 0
        const long c0 = (long)ev_col0[e];
        const long t0 = row_lo > r0 ? row_lo - r0 : 0, t1 = row_hi - r0 < (long)T ? row_hi - r0 : (long)T;      // the taus inside
        for (int w = t - k * W; w < W; w += LOC_THREADS) {         // (one round for W <= LOC_THREADS)
            const long c = c0 + w;
            float a = __uint_as_float(LOC_FILL);
            if (c >= 0 && c < (long)n_cols && t0 < t1) {
                const float *zp = z + (u64)(r0 + t0 - ws_row0) * (u64)n_cols + (u64)c;
                float lo = __builtin_inff(), hi = -__builtin_inff(), ab = -1.0f;
                bool some = false;
#pragma unroll 4
                for (long tau = t0; tau < t1; tau++, zp += n_cols) {
                    const float v = *zp;                           // (a NaN passes none of the comparisons)
                    some |= v == v;
                    if (v < lo) lo = v;
                    if (v > hi) hi = v;
                    const float m = __builtin_fabsf(v);
                    if (m > ab) ab = m;
                }
                if (some) {
                    a = mode == MTS_LOCALIZE_PTP ? hi - lo : mode == MTS_LOCALIZE_NEG ? -lo : mode == MTS_LOCALIZE_POS ? hi : ab;
                    if (!(a == a)) a = __uint_as_float(LOC_FILL);
                }
            }
            if (amp) amp[(u64)e * (u64)W + (u64)w] = a;
            s_amp[k * S + w] = a;
        }
    }
    __syncthreads();
    if (t < G && b0 + t < n_ev) {                                  // event t of the workgroup: its chain
        const long e = e0 + b0 + t;
        const long c0 = (long)ev_col0[e];
        const float *sa = s_amp + t * S;
        float weight = 0.0f, m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, top = 0.0f;
        int best = -1;
        for (int w = 0; w < W; w++) {
            const float a = sa[w];
            if (a == a && (best < 0 || a > top)) { best = w; top = a; }
            if (a > 0.0f) {                                        // g = a; else g = +0 and the step changes no bit: skipped
                const float *p = pos + (u64)(c0 + w) * (u64)D;    // (a > 0: the column position lies in [0, n_cols))
                weight = weight + a;
                m0 = __builtin_fmaf(a, p[0], m0);
                if (D > 1) m1 = __builtin_fmaf(a, p[1], m1);
                if (D > 2) m2 = __builtin_fmaf(a, p[2], m2);
                if (D > 3) m3 = __builtin_fmaf(a, p[3], m3);
            }
        }
        const float fill = __uint_as_float(LOC_FILL);
        o_weight[e] = weight == weight ? weight : fill;
        float *om = o_moment + (u64)e * (u64)D;
        om[0] = m0 == m0 ? m0 : fill;
        if (D > 1) om[1] = m1 == m1 ? m1 : fill;
        if (D > 2) om[2] = m2 == m2 ? m2 : fill;
        if (D > 3) om[3] = m3 == m3 ? m3 : fill;
        o_best[e] = best;
    }
}

int launch_localize(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, long vb, long ve, const long *d_ev_row,
                    const int *d_ev_col0, long e0, long e1, int before, int after, int width, int mode, int n_dims, const float *d_pos,
                    float *d_amp, float *d_weight, float *d_moment, int *d_best)
{
    if (e1 <= e0) return MTS_OK;
    const long T = (long)before + after;
    static_assert(MTS_LOCALIZE_MAX_DIMS == 4, "k_localize keeps four moments in registers");
    if (before < 0 || after < 0 || T < 1 || T > MTS_WAVEFORMS_MAX_ROWS || width < 1 || width > MTS_WAVEFORMS_MAX_WIDTH || n_cols < 1 || ws_rows < 0 ||
        mode < MTS_LOCALIZE_PTP || mode > MTS_LOCALIZE_ABS || n_dims < 1 || n_dims > MTS_LOCALIZE_MAX_DIMS) {
        set_error("localize: snippet of %ld rows x %d positions (1 .. %d, 1 .. %d), mode %d (0 .. 3), %d dimensions (1 .. %d)", T, width,
                  MTS_WAVEFORMS_MAX_ROWS, MTS_WAVEFORMS_MAX_WIDTH, mode, n_dims, MTS_LOCALIZE_MAX_DIMS);
        return MTS_E_ARG;
    }
    if (!d_pos || !d_weight || !d_moment || !d_best) {
        set_error("localize: no positions, weight, moment or best buffer on the device");
        return MTS_E_ARG;
    }
    // a row outside the workspace is never loaded: the slabs (SnippetPlan) hold every row of the recording that their events read
    const long row_lo = vb > ws_row0 ? vb : ws_row0, row_hi = ve < ws_row0 + ws_rows ? ve : ws_row0 + ws_rows;
    const int G = width <= LOC_THREADS ? LOC_THREADS / width : 1;  // events of a workgroup
    for (long e = e0; e < e1;) {
        const long n = e1 - e < (1l << 30) ? e1 - e : (1l << 30);
        const unsigned blocks = (unsigned)((n + G - 1) / G);
        hipLaunchKernelGGL(k_localize, dim3(blocks), dim3(LOC_THREADS), 0, st, d_z, ws_row0, n_cols, row_lo, row_hi, d_ev_row, d_ev_col0, e, n, before,
                           (int)T, width, G, mode, n_dims, d_pos, d_amp, d_weight, d_moment, d_best);
        e += n;
    }
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace mts
