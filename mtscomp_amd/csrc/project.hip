// Channel-mixing matrix products of decoded chunks (mts_project, mts_dev_project), on the matrix cores.
//
//   y[t, k] = sum_{j < n_cols} (x[t, cols[j]] - offset[j]) * w[j, k]          for file rows t of [r_begin, r_end), k < n_out
//
// Input: decoded C-order (rows, n_channels) chunks in HBM, given as a segment table as for k_decimate and k_gram: segment s holds
// file rows [seg_row0[s], seg_row0[s + 1]) at seg_base[s].  The launcher's caller has converted the weights to the compute type F
// and padded them with zeros to multiples of PROJECT_PAD rows and columns (common.h); offsets come in F as well.
//   k_project  one workgroup of 256 threads (4 waves) per (tile of 64 rows) x (tile of 64 outputs).  Per step of KS = 64 (float) or
//              32 (double) columns it stages d = F(x) - F(offset) of the 64 rows in LDS (rows past the range and columns past
//              n_cols read as 0) and the matching KS x 64 slab of w, and wave v runs, for every 4 columns j = 0, 4, .. < n4 of
//              the step, one v_mfma_f32_16x16x4_f32 (v_mfma_f64_16x16x4_f64) per 16-wide output tile q: acc[q] = A(16 x 4) *
//              B(4 x 16) + acc[q], A = d of rows 16 v .. 16 v + 15, B = w of outputs 16 q .. 16 q + 15.  The global loads of the
//              next step sit in registers while the MFMAs of this one run.
// Every output is therefore the chain of 4-column steps over j = 0, 4, .. < n4 = n_cols rounded up to 4, in that order, from +0 (no
// step past n4 is issued: a padded step would turn an accumulated -0 into +0).  It depends on its row, cols, offset and its column
// of w alone, not on the tile, the other outputs, the segments, the piece, the call or the device.
#include "common.h"

namespace mts {

namespace {

constexpr int PT = 256;                                            // threads per workgroup (4 waves)
constexpr int PRJ_TILE = PROJECT_PAD;                              // rows and outputs per workgroup
constexpr int PW_PITCH = PRJ_TILE + 16;                            // LDS pitch of a row of the w slab (B reads: 4 rows x 16 columns a wave)

template <typename F> struct Prj;
template <> struct Prj<float> {
    static constexpr int KS = 64;                                  // columns per step
    typedef float acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row_of(int lane, int reg) { return (lane >> 4) * 4 + reg; }     // C/D: column lane & 15
};
template <> struct Prj<double> {
    static constexpr int KS = 32;
    typedef double acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row_of(int lane, int reg) { return (lane >> 4) + 4 * reg; }     // the f64 form's own map
};

}  // namespace

template <typename T, typename F>
__global__ __launch_bounds__(PT) void k_project(const u8 *const *__restrict__ seg_base, const long *__restrict__ seg_row0, int n_segs, int pitch,
                                                const int *__restrict__ cols, const F *__restrict__ offs, int n_cols, const F *__restrict__ w,
                                                int w_pitch, int n_out, int n_otiles, long r_begin, long r_end, F *__restrict__ out)
{
    constexpr int KS = Prj<F>::KS;
    constexpr int DP = KS + 16 / (int)sizeof(F);                   // LDS pitch of a row of d: 4 (2) elements of padding, A reads conflict-free
    constexpr int DR = PT / KS;                                    // rows a staging pass covers
    constexpr int DN = PRJ_TILE / DR;                              // d items a thread stages per step
    constexpr int WN = KS * PRJ_TILE / PT;                         // w items a thread stages per step
    typedef typename Prj<F>::acc_t acc_t;
    __shared__ F ds[PRJ_TILE * DP];
    __shared__ F wsm[KS * PW_PITCH];
    __shared__ const T *rp[PRJ_TILE];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long t0 = r_begin + (long)(blockIdx.x / n_otiles) * PRJ_TILE;
    const int n0 = (int)(blockIdx.x % n_otiles) * PRJ_TILE;
    const int n4 = (n_cols + 3) & ~3;

    // the tile's rows: one pointer each, null past the range or outside the segments
    if (t < PRJ_TILE) {
        const long r = t0 + t;
        const T *p = nullptr;
        if (r < r_end && n_segs > 0) {
            int lo = 0, hi = n_segs - 1;
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (seg_row0[mid] <= r) lo = mid; else hi = mid - 1; }
            if (r >= seg_row0[lo] && r < seg_row0[lo + 1]) p = (const T *)seg_base[lo] + (u64)(r - seg_row0[lo]) * (u64)pitch;
        }
        rp[t] = p;
    }
    __syncthreads();

    // staging: thread t holds column t % KS of rows t / KS + DR * i, and element t % 64 of rows t / 64 + 4 * i of the w slab
    const int dc = t % KS, dr = t / KS;
    const int wc = t & 63, wr = t >> 6;
    F dv[DN], wvv[WN];
    auto load = [&](int j0) {
        const int j = j0 + dc;
        const bool cok = j < n_cols;
        const int col = cok ? cols[j] : 0;
        const F o = cok ? offs[j] : (F)0;
#pragma unroll
        for (int i = 0; i < DN; i++) {
            const T *p = rp[dr + DR * i];
            dv[i] = (p && cok) ? (F)p[col] - o : (F)0;
        }
#pragma unroll
        for (int i = 0; i < WN; i++) wvv[i] = w[(u64)(j0 + wr + 4 * i) * (u64)w_pitch + (u64)(n0 + wc)];
    };

    acc_t acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = acc_t{0, 0, 0, 0};
    const int kr = lane >> 4, kc = lane & 15;
    load(0);
    for (int j0 = 0; j0 < n4; j0 += KS) {
#pragma unroll
        for (int i = 0; i < DN; i++) ds[(dr + DR * i) * DP + dc] = dv[i];
#pragma unroll
        for (int i = 0; i < WN; i++) wsm[(wr + 4 * i) * PW_PITCH + wc] = wvv[i];
        __syncthreads();
        if (j0 + KS < n4) load(j0 + KS);
        const int ke = n4 - j0 < KS ? n4 - j0 : KS;                // no step past n4
        for (int k = 0; k < ke; k += 4) {
            const F a = ds[(wv * 16 + kc) * DP + k + kr];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const F b = wsm[(k + kr) * PW_PITCH + q * 16 + kc];
                acc[q] = Prj<F>::mfma(a, b, acc[q]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const long r = t0 + wv * 16 + Prj<F>::row_of(lane, reg);
        if (r >= r_end) continue;
        F *dst = out + (u64)(r - r_begin) * (u64)n_out;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = n0 + q * 16 + kc;
            if (k < n_out) dst[k] = acc[q][reg];
        }
    }
}

namespace {

template <typename T, typename F>
int launch_typed(hipStream_t st, const u8 *const *b, const long *r0, int ns, int nc, const int *cols, const void *offs, int n_cols, const void *w,
                 int w_pitch, int n_out, long r_begin, long r_end, void *out)
{
    const long n = r_end - r_begin;
    if (n <= 0) return MTS_OK;
    const long n_otiles = (n_out + PRJ_TILE - 1) / PRJ_TILE;
    const long nt = (n + PRJ_TILE - 1) / PRJ_TILE * n_otiles;
    if (nt > 0x7fffffffl) { set_error("project: too many tiles in one launch"); return MTS_E_ARG; }
    hipLaunchKernelGGL((k_project<T, F>), dim3((unsigned)nt), dim3(PT), 0, st, b, r0, ns, nc, cols, (const F *)offs, n_cols, (const F *)w, w_pitch,
                       n_out, (int)n_otiles, r_begin, r_end, (F *)out);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

template <typename T>
int launch_item(hipStream_t st, int out_itemsize, const u8 *const *b, const long *r0, int ns, int nc, const int *cols, const void *offs, int n_cols,
                const void *w, int w_pitch, int n_out, long r_begin, long r_end, void *out)
{
    if (out_itemsize == 4) return launch_typed<T, float>(st, b, r0, ns, nc, cols, offs, n_cols, w, w_pitch, n_out, r_begin, r_end, out);
    return launch_typed<T, double>(st, b, r0, ns, nc, cols, offs, n_cols, w, w_pitch, n_out, r_begin, r_end, out);
}

}  // namespace

int launch_project(hipStream_t st, int itemsize, int flags, int out_itemsize, const u8 *const *d_seg_base, const long *d_seg_row0, int n_segs,
                   int n_channels, const int *d_cols, const void *d_offs, int n_cols, const void *d_w, int w_pitch, int n_out, long r_begin,
                   long r_end, void *d_out)
{
    if (out_itemsize != 4 && out_itemsize != 8) return MTS_E_ARG;
    if (n_cols < 1 || n_out < 1 || w_pitch % PRJ_TILE || w_pitch < n_out) return MTS_E_ARG;
#define MTS_PRJ_CASE(T) \
    return launch_item<T>(st, out_itemsize, d_seg_base, d_seg_row0, n_segs, n_channels, d_cols, d_offs, n_cols, d_w, w_pitch, n_out, r_begin, r_end, d_out)
    if (flags & MTS_FLAG_FLOAT) {
        if (itemsize == 4) MTS_PRJ_CASE(float);
        if (itemsize == 8) MTS_PRJ_CASE(double);
    } else if (flags & MTS_FLAG_UNSIGNED) {
        if (itemsize == 1) MTS_PRJ_CASE(uint8_t);
        if (itemsize == 2) MTS_PRJ_CASE(uint16_t);
        if (itemsize == 4) MTS_PRJ_CASE(uint32_t);
        if (itemsize == 8) MTS_PRJ_CASE(uint64_t);
    } else {
        if (itemsize == 1) MTS_PRJ_CASE(int8_t);
        if (itemsize == 2) MTS_PRJ_CASE(int16_t);
        if (itemsize == 4) MTS_PRJ_CASE(int32_t);
        if (itemsize == 8) MTS_PRJ_CASE(int64_t);
    }
#undef MTS_PRJ_CASE
    return MTS_E_ARG;
}

}  // namespace mts
