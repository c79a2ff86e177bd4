// Gram partials and column sums of a dense float32 slab of the filtered signal z (mts_filtered_gram, mts_dev_filtered_gram), on the
// fp64 matrix cores.
//
// Input: d_y, the file rows [z_row0, ..) of z as the filter stage left them (C order, n_cols items per row), and the call's table of
// Gram slabs (slab s: file rows [slab_rows[2 s], slab_rows[2 s + 1]), GRAM_SLAB_ROWS rows of a group at most), of which the launch
// takes [slab0, slab0 + n_slabs): all of them lie in the z slab.  Output: the partial layout of gram.hip, which k_gram_combine reads --
// d_part[s - slab0][pair][64][64] double and d_psum[s - slab0][c], the column sums as double bits.
//   k_zgram   one workgroup of 256 threads (4 waves) per (Gram slab) x (pair si <= sj of super tiles of 64 columns), as k_gram.  The
//             arithmetic is k_gram<float>'s, step for step: per step of GRAM_STEP_ROWS rows the items of the pair's columns are staged
//             in LDS, widened to double (rows past the slab's end and columns past n_cols are 0), and wave w runs, for every 4 rows, one
//             v_mfma_f64_16x16x4_f64 per B tile q, acc[q] = A(16 x 4) * B(4 x 16) + acc[q] from +0 -- the same chain on the same items,
//             so the same bits.  What differs is how the items get there.  The slab is dense: a row is n_cols consecutive floats, so
//             there is no segment search, no column gather and no item type.  A row's 64 columns of a super tile are loaded with the
//             widest vectors the row pitch keeps aligned -- float4 when n_cols % 4 == 0, float2 when n_cols % 2 == 0, else float (the
//             slab's base is 256-byte aligned, super tiles begin at multiples of 64 columns, so element r * n_cols + 64 s is a multiple
//             of V exactly when n_cols is; a vector lies wholly inside or outside the n_cols columns for the same reason).  A diagonal
//             pair stages its 64 columns once and reads both operands from them, half the loads of k_gram there.
//             The LDS row pitch is 144 doubles: 288 dwords = 32 mod 64, so the ds_read_b64 of lanes 0..15 (row k, banks 0..31) and
//             lanes 16..31 (row k + 1, banks 32..63) of a half-wave share no bank (k_gram's pitch of 130 puts them 4 banks apart).
//             Column sums: in a diagonal pair thread c < 64 owns column 64 si + c and adds its staged, widened items in row order
//             across the steps, in double from +0 -- the additions of k_gram_colsum in the same order, so the same bits, without a
//             second pass over the slab.
// Nothing depends on the z slab, piece, launch or call.
#include "common.h"

namespace mts {

namespace {

constexpr int ZG_T = 256;                                          // threads per workgroup (4 waves)
constexpr int ZG_S = 64;                                           // columns per super tile (gram.hip's GS: the combine reads that layout)
constexpr int ZG_P = 144;                                          // LDS row pitch in doubles

typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void zg_pair_of(int p, int S, int *si, int *sj)
{
    int i = 0;
    while (p >= S - i) { p -= S - i; i++; }
    *si = i;
    *sj = i + p;
}

// V consecutive floats at p (aligned to V floats)
template <int V> __device__ __forceinline__ void zg_load(const float *p, float (&x)[V])
{
    if constexpr (V == 4) { const float4 q = *(const float4 *)p; x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w; }
    else if constexpr (V == 2) { const float2 q = *(const float2 *)p; x[0] = q.x; x[1] = q.y; }
    else x[0] = *p;
}

}  // namespace

template <int V>
__global__ __launch_bounds__(ZG_T) void k_zgram(const float *__restrict__ y, long z_row0, int n_cols, int S, const long *__restrict__ slab_rows,
                                                long slab0, double *__restrict__ part, u64 *__restrict__ psum)
{
    __shared__ double xs[GRAM_STEP_ROWS][ZG_P];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long slab = slab0 + blockIdx.x;
    int si, sj;
    zg_pair_of(blockIdx.y, S, &si, &sj);
    const bool diag = si == sj;
    const long r_begin = slab_rows[2 * slab], r_end = slab_rows[2 * slab + 1];
    // staging: a row of the step is VR vectors (the A columns, then, off the diagonal, the B columns); thread t loads vector t % VR of
    // the rows t / VR, t / VR + RP, ..: NP of them a step
    constexpr int KL = 16 / V;                                     // vectors a thread stages per step off the diagonal: 16 floats
    const int VR = (diag ? ZG_S : 2 * ZG_S) / V, RP = ZG_T / VR, NP = diag ? KL / 2 : KL;
    const int c = (t % VR) * V, rr = t / VR;                       // column in the staged row, first row in the step
    const int gc = c < ZG_S ? si * ZG_S + c : sj * ZG_S + (c - ZG_S);
    const bool cok = gc < n_cols;                                  // (n_cols % V == 0: the whole vector is inside, or none of it)
    const float *src = y + (u64)(r_begin - z_row0) * (u64)n_cols + (u64)(cok ? gc : 0);
    const long n_rows = r_end - r_begin;
    float v[KL][V];
    auto load_step = [&](long k0) {                                // rows k0 .. k0 + GRAM_STEP_ROWS - 1 of the slab
#pragma unroll
        for (int kk = 0; kk < KL; kk++) {
            if (kk >= NP) continue;
            const long k = k0 + rr + kk * RP;
            if (cok && k < n_rows) {
                zg_load<V>(src + (u64)k * (u64)n_cols, v[kk]);
            } else {
#pragma unroll
                for (int e = 0; e < V; e++) v[kk][e] = 0.0f;
            }
        }
    };
    v4d acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
    double cs = 0.0;                                               // the column sum of thread t < 64 of a diagonal pair
    const int boff = diag ? 0 : ZG_S;                              // where the B columns lie in a staged row
    // the items of step s + 1 are loaded into registers while the MFMAs of step s run
    load_step(0);
    for (long k0 = 0; k0 < n_rows; k0 += GRAM_STEP_ROWS) {
#pragma unroll
        for (int kk = 0; kk < KL; kk++) {
            if (kk >= NP) continue;
#pragma unroll
            for (int e = 0; e < V; e++) xs[rr + kk * RP][c + e] = (double)v[kk][e];
        }
        __syncthreads();
        if (k0 + GRAM_STEP_ROWS < n_rows) load_step(k0 + GRAM_STEP_ROWS);
        if (diag && t < ZG_S) {                                    // (one wave: rows in order)
            const long left = n_rows - k0;
            if (left >= GRAM_STEP_ROWS) {
#pragma unroll
                for (int k = 0; k < GRAM_STEP_ROWS; k++) cs = cs + xs[k][t];
            } else {
                for (int k = 0; k < (int)left; k++) cs = cs + xs[k][t];
            }
        }
        const int kr = lane >> 4, kc = lane & 15;
#pragma unroll
        for (int k = 0; k < GRAM_STEP_ROWS; k += 4) {
            const double a = xs[k + kr][w * 16 + kc];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const double b = xs[k + kr][boff + q * 16 + kc];
                acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // D layout of the f64 form: column lane & 15, row (lane >> 4) + 4 * reg
    double *o = part + ((u64)blockIdx.x * gridDim.y + blockIdx.y) * (u64)(ZG_S * ZG_S);
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) o[(w * 16 + (lane >> 4) + 4 * reg) * ZG_S + q * 16 + (lane & 15)] = acc[q][reg];
    if (diag && t < ZG_S && si * ZG_S + t < n_cols) {
        u64 bits;
        memcpy(&bits, &cs, 8);
        psum[(u64)blockIdx.x * (u64)n_cols + (u64)(si * ZG_S + t)] = bits;
    }
}

namespace {

template <int V>
int launch_v(hipStream_t st, const float *d_y, long z_row0, int n_cols, const long *d_slab_rows, long slab0, long n_slabs, double *d_part, u64 *d_psum)
{
    const int S = (n_cols + ZG_S - 1) / ZG_S;
    hipLaunchKernelGGL(k_zgram<V>, dim3((unsigned)n_slabs, (unsigned)gram_pairs(n_cols)), dim3(ZG_T), 0, st, d_y, z_row0, n_cols, S, d_slab_rows, slab0,
                       d_part, d_psum);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace

int launch_zgram(hipStream_t st, const float *d_y, long z_row0, int n_cols, const long *d_slab_rows, long slab0, long n_slabs, double *d_part,
                 u64 *d_psum)
{
    if (n_slabs <= 0) return MTS_OK;
    if (n_slabs > 65535 || n_cols < 1 || gram_pairs(n_cols) > 65535) { set_error("filtered gram: too many slabs or columns in one launch"); return MTS_E_ARG; }
    if (n_cols % 4 == 0) return launch_v<4>(st, d_y, z_row0, n_cols, d_slab_rows, slab0, n_slabs, d_part, d_psum);
    if (n_cols % 2 == 0) return launch_v<2>(st, d_y, z_row0, n_cols, d_slab_rows, slab0, n_slabs, d_part, d_psum);
    return launch_v<1>(st, d_y, z_row0, n_cols, d_slab_rows, slab0, n_slabs, d_part, d_psum);
}

}  // namespace mts
