// Spatio-temporal template scores of filtered rows (mts_correlate, mts_dev_correlate), on the f32 matrix cores.
//
//   score[t, k] = sum_tau sum_j z[t - before + tau, j] * K[k, tau, j]            for file rows t of [r_begin, r_end), k < n_out
//
// The filter is k_decimate with q = 1 (decimate.hip) into a float32 workspace z of file rows [ws_row0, ws_row0 + ws_rows) x n_cols,
// k_row_median (detect.hip) the reference; the kernel here works on that workspace, slab after slab (reduce.hip: correlate_run).  The
// launcher's caller has repacked the templates group-major: with n4 = n_cols rounded up to 4 and kp = n_out rounded up to COR_TILE,
// row (g / 4 * T + tau) * 4 + c of d_tpl holds K[0 .. kp, tau, g + c] (kp floats; +0 past n_cols and past n_out).
//   k_correlate  one workgroup of 256 threads (4 waves) per (tile of 64 rows) x (tile of 64 outputs).  Per band of COR_BAND = 16
//                columns it stages the (64 + T - 1) x 16 tile of z in LDS (a row outside the workspace or the recording and a column
//                past n_cols are +0, and no load is issued for them).  Per 4-column group g of the band the group's T x 4 x 64 slab
//                of templates streams through LDS in chunks of COR_TC = 16 taus, and wave v runs, for every tau, one
//                v_mfma_f32_16x16x4_f32 per 16-wide output tile q: acc[q] = A(16 x 4) * B(4 x 16) + acc[q], A = columns g .. g + 3 of
//                staged rows 16 v + tau .. 16 v + tau + 15 (one LDS read for the four tiles), B = the templates of outputs 16 q ..
//                16 q + 15 at (tau, g .. g + 3).  The global loads of the next chunk sit in registers while the MFMAs of this one run.
// Every score is therefore the chain of matrix steps over (g, tau), g = 0, 4, .. < n4 outermost and tau = 0 .. T - 1 inside, from +0
// -- bit for bit acc = fmaf(z[t - before + tau, j], K[k, tau, j], acc) in that order (no step past n4 or T is issued: a padded step
// would turn an accumulated -0 into +0).  A NaN is stored as the quiet NaN 0x7fc00000 (what sign and payload the arithmetic gives a
// NaN is not part of the definition).  A score depends on its row, the columns, the taps, the reference and its own template alone,
// not on the tile, the band, the other templates, the slab, the piece, the call or the device.
// LDS: z tile (64 + 255) x 18 floats (pitch 18: the 16 rows x 2 columns that one half-wave reads for A fall on 32 different banks),
// template chunk 64 x 80 floats (pitch 80: the 2 rows x 16 outputs of a half-wave likewise) -- 22 968 + 20 480 bytes, static.
#include "common.h"

namespace mts {

namespace {

constexpr int CT = 256;                                            // threads per workgroup (4 waves)
constexpr int COR_TILE = CORRELATE_PAD;                            // rows and outputs per workgroup
constexpr int COR_BAND = 16;                                       // columns of z staged at a time
constexpr int COR_TC = 16;                                         // taus of a template chunk
constexpr int ZP = COR_BAND + 2;                                   // LDS pitch of a row of the z tile
constexpr int BP = COR_TILE + 16;                                  // LDS pitch of a row of the template chunk
constexpr int ZROWS = COR_TILE + CORRELATE_MAX_T - 1;
constexpr int BN = COR_TC * 4 * COR_TILE / (CT * 4);               // float4 a thread stages per chunk
constexpr u32 COR_NAN = 0x7fc00000u;

typedef float v4f __attribute__((ext_vector_type(4)));

}  // namespace

// rows [row_lo, row_hi): the recording ∩ the workspace
__global__ __launch_bounds__(CT) void k_correlate(const float *__restrict__ z, long ws_row0, int n_cols, long row_lo, long row_hi,
                                                  const float *__restrict__ tpl, int kp, int T, int before, int n_out, int n_otiles, long r_begin,
                                                  long r_end, float *__restrict__ out)
{
    __shared__ float zs[ZROWS * ZP];
    __shared__ __attribute__((aligned(16))) float bs[COR_TC * 4 * BP];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long t0 = r_begin + (long)(blockIdx.x / n_otiles) * COR_TILE;
    const int n0 = (int)(blockIdx.x % n_otiles) * COR_TILE;
    const int n4 = (n_cols + 3) & ~3;
    const int zrows = COR_TILE + T - 1;
    const long zr0 = t0 - before;                                  // the file row of staged row 0

    // a template chunk: rows 4 * tau + c of group g, taus [c0, c0 + COR_TC) ∩ [0, T); thread t holds 4 outputs of rows t / 16 + 16 i
    const int br = t >> 4, bc = (t & 15) * 4;
    float4 bv[BN];
    auto load = [&](int g, int c0) {
        const int rows = 4 * (T - c0 < COR_TC ? T - c0 : COR_TC);
        const float *src = tpl + ((u64)(g >> 2) * (u64)T + (u64)c0) * 4 * (u64)kp + (u64)(n0 + bc);
#pragma unroll
        for (int i = 0; i < BN; i++) {
            const int r = br + 16 * i;
            bv[i] = r < rows ? *(const float4 *)(src + (u64)r * (u64)kp) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    v4f acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = v4f{0.f, 0.f, 0.f, 0.f};
    const int kr = lane >> 4, kc = lane & 15;
    const float *arow = zs + (wv * 16 + kc) * ZP + kr;
    load(0, 0);
    for (int g = 0; g < n4; g += 4) {
        if ((g & (COR_BAND - 1)) == 0) {
            // the band's tile of z (the last readers of the old one have passed the barrier that ends their chunk)
            for (int e = t; e < zrows * COR_BAND; e += CT) {
                const int i = e / COR_BAND, c = e % COR_BAND;
                const long r = zr0 + i;
                float v = 0.f;
                if (r >= row_lo && r < row_hi && g + c < n_cols) v = z[(u64)(r - ws_row0) * (u64)n_cols + (u64)(g + c)];
                zs[i * ZP + c] = v;
            }
        }
        const float *ag = arow + (g & (COR_BAND - 1));
        for (int c0 = 0; c0 < T; c0 += COR_TC) {
#pragma unroll
            for (int i = 0; i < BN; i++) *(float4 *)(bs + (br + 16 * i) * BP + bc) = bv[i];
            __syncthreads();
            if (c0 + COR_TC < T) load(g, c0 + COR_TC);
            else if (g + 4 < n4) load(g + 4, 0);
            const int te = T - c0 < COR_TC ? T - c0 : COR_TC;      // no step past T
            for (int tl = 0; tl < te; tl++) {
                const float a = ag[(c0 + tl) * ZP];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float b = bs[(tl * 4 + kr) * BP + q * 16 + kc];
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[q], 0, 0, 0);
                }
            }
            __syncthreads();
        }
    }
    // C/D: column lane & 15, row (lane >> 4) * 4 + reg
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const long r = t0 + wv * 16 + kr * 4 + reg;
        if (r >= r_end) continue;
        float *dst = out + (u64)(r - r_begin) * (u64)n_out;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = n0 + q * 16 + kc;
            const float v = acc[q][reg];
            if (k < n_out) dst[k] = v == v ? v : __uint_as_float(COR_NAN);
        }
    }
}

int launch_correlate(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, long vb, long ve, const float *d_tpl, int tpl_pitch,
                     int T, int before, int n_out, long r_begin, long r_end, float *d_out)
{
    const long n = r_end - r_begin;
    if (n <= 0) return MTS_OK;
    if (T < 1 || T > CORRELATE_MAX_T || before < 0 || before > T || n_cols < 1 || n_cols > CORRELATE_MAX_COLS || n_out < 1 ||
        n_out > CORRELATE_MAX_OUT || tpl_pitch % COR_TILE || tpl_pitch < n_out || ws_rows < 0) {
        set_error("correlate: templates of %d rows x %d columns, %d outputs (1 .. %d, 1 .. %d, 1 .. %d)", T, n_cols, n_out, CORRELATE_MAX_T,
                  CORRELATE_MAX_COLS, CORRELATE_MAX_OUT);
        return MTS_E_ARG;
    }
    // a row outside the workspace is never loaded: a slab holds every row of the recording that its rows read
    const long row_lo = vb > ws_row0 ? vb : ws_row0, row_hi = ve < ws_row0 + ws_rows ? ve : ws_row0 + ws_rows;
    const long n_otiles = (n_out + COR_TILE - 1) / COR_TILE;
    const long nt = (n + COR_TILE - 1) / COR_TILE * n_otiles;
    if (nt > 0x7fffffffl) { set_error("correlate: too many tiles in one launch"); return MTS_E_ARG; }
    hipLaunchKernelGGL(k_correlate, dim3((unsigned)nt), dim3(CT), 0, st, d_z, ws_row0, n_cols, row_lo, row_hi, d_tpl, tpl_pitch, T, before, n_out,
                       (int)n_otiles, r_begin, r_end, d_out);
    MTS_HIP(hipGetLastError());
    return MTS_OK;
}

}  // namespace mts
