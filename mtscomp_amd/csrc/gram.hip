// Per-window channel Gram matrices and column sums of decoded chunks (mts_gram, mts_dev_gram), on the fp64 matrix cores.
//
// Input: a segment table, as for k_welch: chunk s of the table holds file rows [seg_row0[s], seg_row0[s + 1]) at seg_base[s]
// (n_channels items per row).  A group (MTS_GRAM_GROUP_ROWS rows of a window, aligned to its start) is cut into slabs of
// GRAM_SLAB_ROWS rows, aligned to the group's start; the host passes each slab's file rows [begin, end).
//   k_gram    one workgroup of 256 threads (4 waves) per (slab) x (pair si <= sj of super tiles of 64 columns).  Per step of
//             GRAM_STEP_ROWS rows it stages the items of the 64 + 64 columns in LDS, widened to double (rows past the slab and
//             columns past n_cols read as 0), and wave w runs, for every 4 rows k = 0, 4, .., one v_mfma_f64_16x16x4_f64 per B tile
//             q: acc[q] = A(16 x 4) * B(4 x 16) + acc[q], A = rows k .. k + 3 of the columns of A tile w, B = the same rows of B tile
//             q.  An entry's slab partial is therefore the MFMA chain over the slab's 4-row steps in row order, from +0; it depends
//             on the two columns' items alone, not on the tile it lands in (products commute, so G[i,j] and G[j,i] agree).
//   k_gram_colsum  one thread per (slab, column): the slab's items of the column added in row order from 0 (u64 with wrap for
//             integers, double for floats).
//   k_gram_combine adds the slab partials of a launch to their groups' accumulators in slab order; entry (i, j) and (j, i) both
//             read the partial of (min, max): the matrix is one triangle mirrored.  k_gram_finish converts the exact types'
//             double accumulators to int64 once every slab is in.
// Nothing depends on the piece, launch, call, chunk boundaries or device: the same bits everywhere.
#include "common.h"

namespace mts {

namespace {

constexpr int GT = 256;                                            // threads per workgroup (4 waves)
constexpr int GS = 64;                                             // columns per super tile
constexpr int GP = 2 * GS + 2;                                     // LDS row pitch in doubles (A columns, B columns, padding)

typedef double v4d __attribute__((ext_vector_type(4)));

// pair p -> (si, sj), si <= sj, rows of the upper triangle in order: p = si * S - si * (si - 1) / 2 + (sj - si)
__device__ __forceinline__ void pair_of(int p, int S, int *si, int *sj)
{
    int i = 0;
    while (p >= S - i) { p -= S - i; i++; }
    *si = i;
    *sj = i + p;
}

__device__ __forceinline__ int chunk_of_row(const long *seg_row0, int n_segs, long r)
{
    int lo = 0, hi = n_segs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg_row0[mid] <= r) lo = mid; else hi = mid - 1; }
    return lo;
}

template <typename T> __device__ __forceinline__ bool is_float() { return false; }
template <> __device__ __forceinline__ bool is_float<float>() { return true; }
template <> __device__ __forceinline__ bool is_float<double>() { return true; }

}  // namespace

template <typename T>
__global__ __launch_bounds__(GT) void k_gram(const u8 *const *__restrict__ seg_base, const long *__restrict__ seg_row0, int n_segs, int pitch,
                                             const int *__restrict__ cols, int n_cols, int S, const long *__restrict__ slab_rows, long slab0,
                                             double *__restrict__ part)
{
    __shared__ double xs[GRAM_STEP_ROWS][GP];
    __shared__ const T *rp[2][GRAM_STEP_ROWS];                     // row pointers of this step and the next
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long slab = slab0 + blockIdx.x;                          // the call's slab
    int si, sj;
    pair_of(blockIdx.y, S, &si, &sj);
    const long r_begin = slab_rows[2 * slab], r_end = slab_rows[2 * slab + 1];
    // staging: thread t loads column c = t % 128 (A columns, then B columns) of rows t / 128, t / 128 + 2, ..
    const int c = t & 127;
    const int gc = c < GS ? si * GS + c : sj * GS + (c - GS);
    const bool cok = gc < n_cols;
    const int col = cok ? cols[gc] : 0;
    constexpr int KL = GRAM_STEP_ROWS / (GT / 128);                // rows a thread stages per step
    auto row_ptr = [&](long r) -> const T * {
        if (r >= r_end) return nullptr;
        const int ci = chunk_of_row(seg_row0, n_segs, r);
        return r >= seg_row0[ci] && r < seg_row0[ci + 1] ? (const T *)seg_base[ci] + (u64)(r - seg_row0[ci]) * (u64)pitch : nullptr;
    };
    v4d acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
    // the items of step s are loaded into registers while the MFMAs of step s - 1 run
    T v[KL];
    if (t < GRAM_STEP_ROWS) rp[0][t] = row_ptr(r_begin + t);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KL; kk++) {
        const T *p = rp[0][kk * (GT / 128) + (t >> 7)];
        v[kk] = (p && cok) ? p[col] : (T)0;
    }
    int buf = 0;
    for (long r0 = r_begin; r0 < r_end; r0 += GRAM_STEP_ROWS, buf ^= 1) {
#pragma unroll
        for (int kk = 0; kk < KL; kk++) xs[kk * (GT / 128) + (t >> 7)][c] = (double)v[kk];
        const bool more = r0 + GRAM_STEP_ROWS < r_end;
        if (more && t < GRAM_STEP_ROWS) rp[buf ^ 1][t] = row_ptr(r0 + GRAM_STEP_ROWS + t);
        __syncthreads();
        if (more) {
#pragma unroll
            for (int kk = 0; kk < KL; kk++) {
                const T *p = rp[buf ^ 1][kk * (GT / 128) + (t >> 7)];
                v[kk] = (p && cok) ? p[col] : (T)0;
            }
        }
        const int kr = lane >> 4, kc = lane & 15;
#pragma unroll
        for (int k = 0; k < GRAM_STEP_ROWS; k += 4) {
            const double a = xs[k + kr][w * 16 + kc];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const double b = xs[k + kr][GS + q * 16 + kc];
                acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // D layout of the f64 form: column lane & 15, row (lane >> 4) + 4 * reg
    double *o = part + ((u64)blockIdx.x * gridDim.y + blockIdx.y) * (u64)(GS * GS);
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) o[(w * 16 + (lane >> 4) + 4 * reg) * GS + q * 16 + (lane & 15)] = acc[q][reg];
}

template <typename T>
__global__ void k_gram_colsum(const u8 *const *__restrict__ seg_base, const long *__restrict__ seg_row0, int n_segs, int pitch,
                              const int *__restrict__ cols, int n_cols, const long *__restrict__ slab_rows, long slab0, u64 *__restrict__ part)
{
    const int gc = blockIdx.x * blockDim.x + threadIdx.x;
    if (gc >= n_cols) return;
    const long slab = slab0 + blockIdx.y;
    const long r_begin = slab_rows[2 * slab], r_end = slab_rows[2 * slab + 1];
    const int col = cols[gc];
    double sf = 0.0;
    u64 si = 0;
    // rows in order, a chunk at a time, the loads of 8 rows issued together
    for (long r = r_begin; r < r_end;) {
        const int ci = chunk_of_row(seg_row0, n_segs, r);
        if (r < seg_row0[ci] || r >= seg_row0[ci + 1]) { r++; continue; }   // (rows outside the chunks: none when the host's checks hold)
        const long e = seg_row0[ci + 1] < r_end ? seg_row0[ci + 1] : r_end;
        const T *q = (const T *)seg_base[ci] + (u64)(r - seg_row0[ci]) * (u64)pitch + col;
        long i = 0;
        for (; i + 8 <= e - r; i += 8) {
            T v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = q[(u64)(i + j) * (u64)pitch];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (is_float<T>()) sf = sf + (double)v[j];
                else si += (u64)(long long)v[j];                     // (sign- or zero-extended by the type, then modulo 2^64)
            }
        }
        for (; i < e - r; i++) {
            const T x = q[(u64)i * (u64)pitch];
            if (is_float<T>()) sf = sf + (double)x;
            else si += (u64)(long long)x;
        }
        r = e;
    }
    u64 bits;
    if (is_float<T>()) memcpy(&bits, &sf, 8);
    else bits = si;
    part[(u64)blockIdx.y * (u64)n_cols + gc] = bits;
}

// acc_gram[g][i][j] = acc_gram[g][i][j] + part[slab][pair(i, j)][..] and acc_sum[g][c] likewise (u64 with wrap for integer sums) for
// the launch's slabs [s0, s1) of group g, in slab order; gfirst[g]: the call's first slab of group g
__global__ void k_gram_combine(const double *__restrict__ part, const u64 *__restrict__ psum, long s0, long s1, long g0, const long *__restrict__ gfirst,
                               int n_cols, int S, int float_sum, double *__restrict__ acc_gram, u64 *__restrict__ acc_sum)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nn = (long)n_cols * n_cols;
    if (e >= nn + n_cols) return;
    const long g = g0 + blockIdx.y;
    const long b0 = gfirst[g] > s0 ? gfirst[g] : s0, b1 = gfirst[g + 1] < s1 ? gfirst[g + 1] : s1;
    if (e < nn) {
        const int i = (int)(e / n_cols), j = (int)(e % n_cols);
        const int a = i < j ? i : j, b = i < j ? j : i;
        const int si = a / GS, sj = b / GS;
        const long p = (long)si * S - (long)si * (si - 1) / 2 + (sj - si);
        const long n_pairs = (long)S * (S + 1) / 2;
        const u64 off = (u64)p * (GS * GS) + (u64)(a % GS) * GS + (u64)(b % GS);
        double v = acc_gram[(u64)g * (u64)nn + (u64)e];
        for (long s = b0; s < b1; s++) v = v + part[(u64)(s - s0) * (u64)n_pairs * (GS * GS) + off];
        acc_gram[(u64)g * (u64)nn + (u64)e] = v;
    } else {
        const long c = e - nn;
        u64 *dst = acc_sum + (u64)g * (u64)n_cols + (u64)c;
        if (float_sum) {
            double v;
            memcpy(&v, dst, 8);
            for (long s = b0; s < b1; s++) { double x; const u64 bits = psum[(u64)(s - s0) * (u64)n_cols + c]; memcpy(&x, &bits, 8); v = v + x; }
            memcpy(dst, &v, 8);
        } else {
            u64 v = *dst;
            for (long s = b0; s < b1; s++) v += psum[(u64)(s - s0) * (u64)n_cols + c];
            *dst = v;
        }
    }
}

// the exact types' group sums: integers below 2^52 held as doubles -> int64 in place
__global__ void k_gram_finish(double *__restrict__ acc, long n)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const long long v = (long long)acc[e];
    memcpy(acc + e, &v, 8);
}

namespace {

template <typename T>
int launch_t(hipStream_t st, const u8 *const *b, const long *r0, int ns, int nc, const int *cols, int n_cols, const long *slab_rows, long slab0,
             long n_slabs, double *d_part, u64 *d_psum)
{
    const int S = (n_cols + GS - 1) / GS;
    const long P = (long)S * (S + 1) / 2;
    hipLaunchKernelGGL(k_gram<T>, dim3((unsigned)n_slabs, (unsigned)P), dim3(GT), 0, st, b, r0, ns, nc, cols, n_cols, S, slab_rows, slab0, d_part);
    MTS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_gram_colsum<T>, dim3((unsigned)((n_cols + 255) / 256), (unsigned)n_slabs), dim3(256), 0, st, b, r0, ns, nc, cols, n_cols,
                       slab_rows, slab0, d_psum);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace

long gram_pairs(int n_cols)
{
    const long S = (n_cols + GS - 1) / GS;
    return S * (S + 1) / 2;
}

long gram_slab_bytes(int n_cols)
{
    return gram_pairs(n_cols) * GS * GS * 8 + 8l * n_cols;
}

int launch_gram(hipStream_t st, int itemsize, int flags, const u8 *const *d_seg_base, const long *d_seg_row0, int n_segs, int n_channels,
                const int *d_cols, int n_cols, const long *d_slab_rows, long slab0, long n_slabs, double *d_part, u64 *d_psum)
{
    if (n_slabs <= 0) return MTS_OK;
    if (n_slabs > 65535 || gram_pairs(n_cols) > 65535) { set_error("gram: too many slabs or columns in one launch"); return MTS_E_ARG; }
#define MTS_GRAM_CASE(T) return launch_t<T>(st, d_seg_base, d_seg_row0, n_segs, n_channels, d_cols, n_cols, d_slab_rows, slab0, n_slabs, d_part, d_psum)
    if (flags & MTS_FLAG_FLOAT) {
        if (itemsize == 4) MTS_GRAM_CASE(float);
        if (itemsize == 8) MTS_GRAM_CASE(double);
    } else if (flags & MTS_FLAG_UNSIGNED) {
        if (itemsize == 1) MTS_GRAM_CASE(uint8_t);
        if (itemsize == 2) MTS_GRAM_CASE(uint16_t);
        if (itemsize == 4) MTS_GRAM_CASE(uint32_t);
        if (itemsize == 8) MTS_GRAM_CASE(uint64_t);
    } else {
        if (itemsize == 1) MTS_GRAM_CASE(int8_t);
        if (itemsize == 2) MTS_GRAM_CASE(int16_t);
        if (itemsize == 4) MTS_GRAM_CASE(int32_t);
        if (itemsize == 8) MTS_GRAM_CASE(int64_t);
    }
#undef MTS_GRAM_CASE
    return MTS_E_ARG;
}

int launch_gram_combine(hipStream_t st, const double *d_part, const u64 *d_psum, long s0, long s1, long g0, long g1, const long *d_gfirst, int n_cols,
                        int float_sum, double *d_gram, u64 *d_sum)
{
    if (s1 <= s0 || g1 <= g0) return MTS_OK;
    const int S = (n_cols + GS - 1) / GS;
    const long n = (long)n_cols * n_cols + n_cols;
    hipLaunchKernelGGL(k_gram_combine, dim3((unsigned)((n + 255) / 256), (unsigned)(g1 - g0)), dim3(256), 0, st, d_part, d_psum, s0, s1, g0, d_gfirst,
                       n_cols, S, float_sum, d_gram, d_sum);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

int launch_gram_finish(hipStream_t st, double *d_gram, long n)
{
    if (n <= 0) return MTS_OK;
    hipLaunchKernelGGL(k_gram_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_gram, n);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace mts
