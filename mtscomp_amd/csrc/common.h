// Internal declarations shared by the HIP translation units of libmtscomp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/mtscomp_hip.h"
#include "codec_plan.h"      // the descriptors and constants the host plans share with the kernels: TileDesc, ChunkDesc, InfChunk, TILE, HALO, SEG, ...

namespace mts {

// ---- DEFLATE constants (zlib 1.2.11, windowBits 15, memLevel 8) --------------------------------
constexpr int MIN_MATCH = 3;
constexpr int MAX_MATCH = 258;
constexpr int WSIZE = 32768;
constexpr int MAX_DIST = WSIZE - 262;      // 32506
constexpr int TOO_FAR = 4096;
constexpr int L_CODES = 286;
constexpr int D_CODES = 30;
constexpr int BL_CODES = 19;

constexpr u32 REL_MASK = (1u << REL_BITS) - 1;

struct LevelCfg { int good, lazy, nice, chain; };

// per-block record produced by the tree stage
#define MTS_PACK_RANGES 8    // ranges of token indices the block packer's waves take (deflate.hip: PACK_RANGES)
struct BlockRec {
    u32 tok0, ntok;          // token range (chunk-relative)
    u32 in_start, in_len;    // input byte range
    u32 nbits;               // bits of the block incl. the 3 header bits (stored: payload handled apart)
    u32 btype;               // 0 stored 1 fixed 2 dynamic
    u32 hdr_bits;            // dynamic: bits of the tree header (after the 3-bit block header)
    u32 last;
    u32 range_bits[MTS_PACK_RANGES];   // fixed / dynamic: code bits of the token indices [r * 16384 / MTS_PACK_RANGES, ..) (index ntok = the end-of-block code): where the packer's waves start
    u64 bit_start;           // bit offset in the chunk's zlib stream
};

struct ChunkOut {
    u64 nbytes;              // compressed size
    u32 ntok, nblk;
    u32 adler;
    u32 trailing;            // last token is the post-loop literal
};

// wave-wide predicates straight from the condition's lane mask (HIP's __ballot / __any take an int: the mask is first turned into a
// value per lane -- v_cndmask -- and compared again -- v_cmp: two vector instructions per use in kernels that are bound by them)
__device__ __forceinline__ u64 ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool any64(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

// ---- error plumbing -------------------------------------------------------------------------------
void set_error(const char *fmt, ...);
#define MTS_HIP(call)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            mts::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                           __LINE__);                                                       \
            return MTS_E_HIP;                                                               \
        }                                                                                   \
    } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) belongs to the CURRENT DEVICE's function object: it is applied once per
// (device, kernel), under a lock (several host threads drive several devices of one process; api.hip)
int ensure_dynamic_lds(const void *kernel, int bytes);
#define MTS_LDS_ATTR(kernel, bytes)                                                 \
    do {                                                                            \
        int rc_ = mts::ensure_dynamic_lds((const void *)(kernel), (int)(bytes));    \
        if (rc_) return rc_;                                                        \
    } while (0)

// ---- kernel launchers (one per stage; all asynchronous on `st`) -----------------------------------
// transform.hip
int launch_delta_transpose(hipStream_t st, const void *d_raw, void *d_stream, const ChunkDesc *d_chunks,
                           int n_chunks, u32 max_rows, int n_channels, int itemsize, int flags,
                           u64 *d_adler_acc /* 2 per chunk, zeroed by the launcher */);
int launch_cumsum_transpose(hipStream_t st, const void *d_stream, void *d_out, const u64 *d_stream_off,
                            const u64 *d_out_off, const u32 *d_rows, const int *d_status, int n_chunks,
                            u32 max_rows, int n_channels, int itemsize, int flags, void *d_segsums);
size_t cumsum_scratch_bytes(int n_chunks, u32 max_rows, int n_channels);
int launch_synth_int16(hipStream_t st, int16_t *d_out, long t0, long t1, int n_channels, long seed);
int launch_adler_stream(hipStream_t st, const u8 *d_stream, const u64 *d_stream_off, const u32 *d_n,
                        int n_chunks, u32 max_n, u64 *d_adler_acc,
                        const u32 *d_skip /* null, or per chunk (stride in words): >= 2 = already summed; the sums are then NOT zeroed here */, u32 skip_stride);

// pieces of decoded chunks gathered on the device (mts_cache_read_slices)
struct GatherChunk { long row0; const u8 *base; long pitch; };          // first row in the concatenation; null = the chunk failed; items per row of the entry
struct GatherReq { long rb, rs, cb, cs, nr, ncol, out_off; };           // rows rb + i * rs (i < nr), columns cb + j * cs (j < ncol) -> out_off
int launch_gather_slices(hipStream_t st, const GatherChunk *d_chunks, int n_chunks, const GatherReq *d_req, int n_req, u64 max_items,
                         int n_channels, int itemsize, u8 *d_out);

// stats.hip: per-window statistics of decoded chunks (mts_window_stats)
constexpr int STAT_TILE_ROWS = 512;                                     // rows of a tile: one workgroup, one partial per column
struct StatTile { const u8 *base; long row_lo, n_rows; int chunk, pad; };   // base: row 0 of the decoded chunk (n_channels items per row)
// one partial per (tile, column) into the slab -- four planes of n_tiles * n_cols 8-byte entries: min, max, sum, sum of squares
int launch_stats_tiles(hipStream_t st, int itemsize, int flags, const StatTile *d_tiles, const int *d_ids /* the tiles of this launch */,
                       int n_launch, const int *d_ok /* per chunk: 0 = failed, its tiles are identities */, const int *d_cols, int n_cols,
                       int n_channels, u8 *d_slab, long n_tiles);
// windows w < n_windows: tiles [win_tiles[w], win_tiles[w + 1]) of the slab, in order, into the (n_windows, n_cols) outputs
int launch_stats_combine(hipStream_t st, int itemsize, int flags, const u8 *d_slab, long n_tiles, const long *d_win_tiles, long n_windows,
                         int n_cols, void *d_min, void *d_max, void *d_sum, void *d_sumsq);

// select.hip: one round of a radix select over decoded chunks (mts_rank_hist).  Tiles as above, of at most SEL_TILE_ROWS rows;
// d_tile_win[t]: the window of tile t.  Selectors and outputs: (n_windows, MTS_RANK_SELECTORS, [256,] n_cols), see include/mtscomp_hip.h;
// the outputs are accumulated with integer atomics (the caller sets hist = 0, kmin = all ones, kmax = 0 first)
constexpr int SEL_TILE_ROWS = 4096;                                     // rows of a tile: one workgroup, one LDS histogram flush per 64 columns
int launch_rank_hist(hipStream_t st, int itemsize, int flags, int mode, const StatTile *d_tiles, const long *d_tile_win, const int *d_ids,
                     int n_launch, const int *d_ok, const int *d_cols, int n_cols, int n_channels, const double *d_center, const u64 *d_prefix,
                     const int *d_shift, u32 *d_hist, u64 *d_kmin, u64 *d_kmax);

// zselect.hip: the same round over a float32 workspace z that launch_decimate (q = 1) and launch_row_median filled
// (mts_filtered_rank_hist).  d_y holds the file rows [s0, s1), n_cols items a row, and every one of them is counted on the window grid
// (row_begin, window_rows); selectors, centers and outputs as launch_rank_hist, accumulated the same way.  One workgroup per
// block_rows rows and 64 columns, its rows cut at the grid's windows by arithmetic alone (zrank_segment, reduce_plan.h)
constexpr long ZSEL_BLOCK_ROWS = 4096;                                  // H: as SEL_TILE_ROWS, one LDS histogram flush per 64 columns and window
int launch_zrank_hist(hipStream_t st, int mode, const float *d_y, long s0, long s1, long block_rows, int n_cols, long row_begin, long window_rows,
                      const double *d_center, const u64 *d_prefix, const int *d_shift, u32 *d_hist, u64 *d_kmin, u64 *d_kmax);

// decimate.hip: FIR + keep every q-th row of decoded chunks (mts_decimate).  Outputs k in [k_begin, k_end) of the call:
// out[(k - k_begin) * n_cols + c] = sum_j taps[j] * x[first_row + k * q - j, cols[c]] in the out_itemsize float type, j ascending,
// x = 0 outside [valid_begin, valid_end) and outside the segments; segment s holds file rows [seg_row0[s], seg_row0[s + 1]) at
// d_seg_base[s] (n_channels items per row); d_taps: n_taps values of the output type
int launch_decimate(hipStream_t st, int itemsize, int flags, int out_itemsize, const u8 *const *d_seg_base, const long *d_seg_row0, int n_segs,
                    int n_channels, const int *d_cols, int n_cols, const void *d_taps, int n_taps, int q, long first_row, long k_begin,
                    long k_end, long valid_begin, long valid_end, void *d_out);

// detect.hip: peak detection on a float32 workspace z of file rows [ws_row0, ws_row0 + ws_rows) x n_cols that launch_decimate (q = 1)
// filled (mts_detect).  launch_row_median subtracts every row's median in place.  launch_detect_mask: one bit per (row of [s0, s1),
// column position), row-major in words of 64 positions ((n_cols + 63) / 64 words per row): 1 = an event; neighbours outside the
// workspace do not exist.  launch_detect_emit: the events of the bitmap in (row, position) order to d_row / d_pos / d_amp from position
// *d_total on, those at positions >= max_events counted only; *d_total += the events of the bitmap.  d_counts / d_offsets: one entry
// per detect_blocks(n_words)
int launch_row_median(hipStream_t st, float *d_y, long n_rows, int n_cols);
long detect_bitmap_words(long n_rows, int n_cols);
long detect_blocks(long n_words);
int launch_detect_mask(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, const float *d_thr, int sign, int exclude_rows,
                       int exclude_cols, long s0, long s1, u64 *d_bitmap);
int launch_detect_emit(hipStream_t st, const u64 *d_bitmap, long n_words, u32 *d_counts, u64 *d_offsets, u64 *d_total, const float *d_z,
                       long ws_row0, int n_cols, long s0, long max_events, long *d_row, int *d_pos, float *d_amp);

// waveforms.hip: snippets of the same workspace (mts_waveforms).  For the events e of [e0, e1): wave[e, tau, w] = z[ev_row[e] - before +
// tau, ev_col0[e] + w] (tau < before + after, w < width; the quiet NaN 0x7fc00000 for a row outside [vb, ve) or the workspace and a
// column position outside [0, n_cols), and for a z that is a NaN), and the first minimum and maximum over the entries that are not NaN with their flat indices
// tau * width + w (NaN and -1 when there is none).  d_wave may be null: the stores are skipped, nothing else
int launch_waveforms(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, long vb, long ve, const long *d_ev_row,
                     const int *d_ev_col0, long e0, long e1, int before, int after, int width, float *d_wave, float *d_min, int *d_argmin,
                     float *d_max, int *d_argmax);

// meanwave.hip: per-label fixed-point sums of the same snippets (mts_mean_waveforms).  d_parts[0 .. n_parts): the parts of a slab's
// events (MeanParts, reduce_plan.h) into d_perm.  For every event e of a part with label l and every entry (tau, w) whose row lies in
// [vb, ve) and the workspace and whose column position lies in [0, n_cols): d = (double)z * (1 / resolution); a NaN or |d| >= 2^42 adds 1
// to d_skipped[l], every other d adds rint(d) to d_sum[l, tau, w] and 1 to d_count[l, tau, w] -- integer atomics on buffers that the
// caller zeroed before the first slab
struct MeanPart;
int launch_mean_waveforms(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, long vb, long ve, const long *d_ev_row,
                          const int *d_ev_col0, const long *d_perm, const MeanPart *d_parts, long n_parts, int before, int after, int width,
                          double resolution, long long *d_sum, int *d_count, long *d_skipped);

// features.hip: the same snippets projected on a temporal basis (mts_waveform_features).  For the events e of [e0, e1), p < n_comp and
// w < width: feat[e, p, w] = the chain acc = fmaf(z[ev_row[e] - before + tau, ev_col0[e] + w], basis[p, tau], acc) over tau = 0 .. T - 1
// from +0; the quiet NaN 0x7fc00000 when the column position lies outside [0, n_cols), when one of the T rows lies outside [vb, ve)
// or the workspace, and for a NaN result.  d_basis: the image that features_basis_image made, n_comp * T floats
constexpr int FEAT_PB = 8;                                         // components of a register block
int launch_waveform_features(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, long vb, long ve, const long *d_ev_row,
                             const int *d_ev_col0, long e0, long e1, int before, int after, int width, int n_comp, const float *d_basis,
                             float *d_feat);
// basis (P, T) C order -> the kernel's image: blocks of FEAT_PB components one behind the other, the last of the P % FEAT_PB that
// remain; component p0 + k of a block of nb components from p0 lies at p0 * T + tau * nb + k
inline void features_basis_image(const float *basis, int P, int T, float *image)
{
    for (int p0 = 0; p0 < P; p0 += FEAT_PB) {
        const int nb = P - p0 < FEAT_PB ? P - p0 : FEAT_PB;
        for (int tau = 0; tau < T; tau++)
            for (int k = 0; k < nb; k++) image[(size_t)p0 * T + (size_t)tau * nb + k] = basis[(size_t)(p0 + k) * T + tau];
    }
}

// localize.hip: the same snippets reduced to channel amplitudes and amplitude-weighted position sums (mts_localize).  For the events e of
// [e0, e1) and w < width: amp[e, w] (when d_amp is given) = the amplitude (mode: MTS_LOCALIZE_PTP / NEG / POS / ABS) of the column
// z[ev_row[e] - before + tau, ev_col0[e] + w], tau < T, over its entries that are not NaN and whose row lies in [vb, ve) and the
// workspace; the quiet NaN 0x7fc00000 when there is none, when the column position lies outside [0, n_cols), and for a NaN result.
// weight[e], moment[e, d < n_dims]: the chains over w upwards of g = amp > 0 ? amp : +0 and fmaf(g, pos[ev_col0[e] + w, d], .) from +0;
// best[e]: the first w of the largest amplitude that is not NaN, -1 for none.  d_pos: (n_cols, n_dims) C order, finite
int launch_localize(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, long vb, long ve, const long *d_ev_row,
                    const int *d_ev_col0, long e0, long e1, int before, int after, int width, int mode, int n_dims, const float *d_pos,
                    float *d_amp, float *d_weight, float *d_moment, int *d_best);

// correlate.hip: template scores on the same workspace (mts_correlate).  out[(t - r_begin) * n_out + k] for file rows t of [r_begin,
// r_end) = the chain of matrix steps over (g, tau), g = 0, 4, .. < n4 outermost and tau < T inside, of z[t - before + tau, g .. g + 3]
// against the templates; z = +0 for a row outside [vb, ve) or the workspace; a NaN is stored as 0x7fc00000.  d_tpl: the templates
// group-major, row (g / 4 * T + tau) * 4 + c = K[0 .. tpl_pitch, tau, g + c], zeros past n_cols and n_out; tpl_pitch: n_out rounded up
// to CORRELATE_PAD
constexpr int CORRELATE_MAX_T = MTS_CORRELATE_MAX_T;               // include/mtscomp_hip.h
constexpr int CORRELATE_MAX_OUT = MTS_CORRELATE_MAX_OUT;
constexpr int CORRELATE_MAX_COLS = MTS_CORRELATE_MAX_COLS;
constexpr int CORRELATE_PAD = 64;
int launch_correlate(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, long vb, long ve, const float *d_tpl, int tpl_pitch,
                     int T, int before, int n_out, long r_begin, long r_end, float *d_out);

// tmatch.hip: the events of a slab of those scores (mts_match_templates).  d_score: score[t, k] of file rows [sc_row0, sc_row0 + sc_rows)
// x n_out, every row of the recording within exclude_rows of [s0, s1).  launch_tmatch_best: per score row the largest score that is not
// a NaN and the first template that attains it (NaN and -1 for a row of NaNs).  launch_tmatch_mask: one bit per row of [s0, s1), in
// words of 64 rows (tmatch_bitmap_words): 1 = an event, best > d_thr[arg] and no row within exclude_rows that beats it; rows outside the
// slab do not exist.  launch_tmatch_emit: the events of the bitmap in row order to d_row / d_tpl / d_score from position *d_total on,
// those at positions >= max_events counted only; *d_total += the events of the bitmap (launch_bitmap_offsets, detect.hip: the counts
// and offsets of any bitmap's blocks of DETECT_BLOCK_WORDS words, one entry per detect_blocks(n_words))
constexpr int TMATCH_MAX_EXCLUDE = MTS_TMATCH_MAX_EXCLUDE;         // include/mtscomp_hip.h
constexpr int DETECT_BLOCK_WORDS = 1024;
int launch_bitmap_offsets(hipStream_t st, const u64 *d_bitmap, long n_words, u32 *d_counts, u64 *d_offsets, u64 *d_total);
long tmatch_bitmap_words(long n_rows);
int launch_tmatch_best(hipStream_t st, const float *d_score, long n_rows, int n_out, float *d_best, int *d_arg);
int launch_tmatch_mask(hipStream_t st, const float *d_best, const int *d_arg, long sc_row0, long sc_rows, const float *d_thr, int exclude_rows,
                       long s0, long s1, u64 *d_bitmap);
int launch_tmatch_emit(hipStream_t st, const u64 *d_bitmap, long n_words, u32 *d_counts, u64 *d_offsets, u64 *d_total, const float *d_best,
                       const int *d_arg, long sc_row0, long s0, long max_events, long *d_row, int *d_tpl, float *d_score);

// subtract.hip: template subtraction on the same workspace (mts_residual, mts_match_residual).  For every row t of the workspace and
// column j: acc = z[t, j]; for the events e with 0 <= tau = t - ev_row[e] + before < T, in list order: acc = fmaf(ev_namp[e],
// K[ev_tpl[e], tau, j], acc); out[t - ws_row0, j] = acc, a NaN as 0x7fc00000.  d_ev_row ascending, d_ev_namp the negated amplitudes,
// d_tpl the plain (K, T, n_cols) templates (none of the four is read when n_ev == 0); d_out may be d_z: in place
int launch_subtract(hipStream_t st, const float *d_z, long ws_row0, long ws_rows, int n_cols, const long *d_ev_row, const int *d_ev_tpl,
                    const float *d_ev_namp, long n_ev, const float *d_tpl, int T, int before, float *d_out);

// welch.hip: Welch PSD partials (mts_welch).  Segments s of blocks [block0, block0 + n_blocks) (block b: segments [b * B, (b + 1) * B)
// ∩ [.., seg_end)) start at file row row_seg0 + s * step; d_part[(b - block0), k, c] = sum over the block's segments, in order, of
// |X_k|^2 of column cols[c] (float64; X in the csize float type).  d_taper: 2^log2n values, d_tw: 2^log2n complex values
// exp(-2 pi i q / 2^log2n), both in the compute type.  The combine adds the partials of call blocks [lb0, lb1) to the accumulators of
// their groups (group_blocks blocks each; acc: (groups of the call, n_elems)) in block order.
#define WELCH_BLOCK_SEGMENTS MTS_WELCH_BLOCK_SEGMENTS   // B and G: include/mtscomp_hip.h
#define WELCH_GROUP_ROWS MTS_WELCH_GROUP_ROWS
int welch_tile_columns(int csize, int log2n);
int launch_welch(hipStream_t st, int itemsize, int flags, int csize, int log2n, const u8 *const *d_seg_base, const long *d_seg_row0, int n_segs,
                 int n_channels, const int *d_cols, int n_cols, const void *d_taper, const void *d_tw, long row_seg0, long step, long seg_end,
                 long block0, long n_blocks, int detrend, double *d_part);
int launch_welch_combine(hipStream_t st, const double *d_part, long lb0, long lb1, long group_blocks, long n_elems, double *d_acc);

// gram.hip: Gram partials (mts_gram).  Slab s of the call covers file rows [slab_rows[2 s], slab_rows[2 s + 1]) (GRAM_SLAB_ROWS rows of
// a group at most, aligned to its start).  launch_gram: for the call's slabs [slab0, slab0 + n_slabs), d_part[s - slab0][pair][64][64]
// double (pair: super tiles si <= sj of 64 columns, gram_pairs of them) and d_psum[s - slab0][c] (u64: integers modulo 2^64, floats as
// double bits).  launch_gram_combine adds the slabs [s0, s1) (partials at d_part / d_psum) to the accumulators of their groups [g0, g1)
// (d_gfirst[g]: the first slab of the call's group g) in slab order: d_gram (groups, n_cols, n_cols) double, d_sum (groups, n_cols).
// launch_gram_finish turns n doubles holding integers into int64 in place.
#define GRAM_GROUP_ROWS MTS_GRAM_GROUP_ROWS            // include/mtscomp_hip.h
#define GRAM_SLAB_ROWS MTS_GRAM_SLAB_ROWS
constexpr int GRAM_STEP_ROWS = 32;                    // rows staged in LDS per step of k_gram (a multiple of 4)
static_assert(GRAM_SLAB_ROWS % GRAM_STEP_ROWS == 0, "slabs are whole steps");
long gram_pairs(int n_cols);
long gram_slab_bytes(int n_cols);                     // partial bytes per slab
int launch_gram(hipStream_t st, int itemsize, int flags, const u8 *const *d_seg_base, const long *d_seg_row0, int n_segs, int n_channels,
                const int *d_cols, int n_cols, const long *d_slab_rows, long slab0, long n_slabs, double *d_part, u64 *d_psum);
int launch_gram_combine(hipStream_t st, const double *d_part, const u64 *d_psum, long s0, long s1, long g0, long g1, const long *d_gfirst, int n_cols,
                        int float_sum, double *d_gram, u64 *d_sum);
int launch_gram_finish(hipStream_t st, double *d_gram, long n);

// zgram.hip: the same partials from a float32 workspace z that launch_decimate (q = 1) and launch_row_median filled
// (mts_filtered_gram).  d_y holds the file rows from z_row0 on, n_cols items a row; the slabs [slab0, slab0 + n_slabs) of d_slab_rows lie
// inside them.  d_part and d_psum as launch_gram's for a float32 recording (the sums as double bits), bit for bit: one launch for both
int launch_zgram(hipStream_t st, const float *d_y, long z_row0, int n_cols, const long *d_slab_rows, long slab0, long n_slabs, double *d_part,
                 u64 *d_psum);

// project.hip: channel-mixing products (mts_project).  out[(t - r_begin) * n_out + k] = the chain of 4-column MFMA steps over
// (x[t, cols[j]] - offs[j]) * w[j, k], j ascending, for file rows t of [r_begin, r_end) in the out_itemsize float type.  d_offs: n_cols
// values and d_w: (n_cols rounded up to PROJECT_PAD, w_pitch) values of that type, zeros past n_cols and n_out; w_pitch: n_out rounded
// up to PROJECT_PAD
constexpr int PROJECT_PAD = 64;
int launch_project(hipStream_t st, int itemsize, int flags, int out_itemsize, const u8 *const *d_seg_base, const long *d_seg_row0, int n_segs,
                   int n_channels, const int *d_cols, const void *d_offs, int n_cols, const void *d_w, int w_pitch, int n_out, long r_begin,
                   long r_end, void *d_out);

// deflate.hip
size_t hash_sort_ws_bytes(int n_tiles);                            // the one-pass sort's per-tile records
int launch_hash_sort(hipStream_t st, const u8 *d_stream, const TileDesc *d_tiles, int n_tiles, u32 *d_tmp, u32 *d_sorted,
                     int force_ballot, void *d_ws);
int launch_match(hipStream_t st, const u8 *d_stream, const TileDesc *d_tiles, int n_tiles, const u32 *d_sorted, u32 *d_tables, u32 *d_quarter,
                 LevelCfg cfg, u32 *d_flags /* [0] |= 1: a hash run out of position order; [MATCH_SINK_WORD0 ...]: MATCH_SINK_BYTES of sink (codec_plan.h) */,
                 int all_quarters /* debug tap: write the side table for every position */);
struct ParseBufs {
    u32 *entry, *exit_a, *exit_b, *cnt, *tokbase;   // per segment
    u32 *cp;                                        // per segment 16 words: 7 checkpoint positions, 7 token counts
    u32 *marks;                                     // per segment MARK_WORDS words: what the walk did at every position (deflate.hip: MarkW)
    u32 *seg_chunk, *seg_start;                     // per segment: owning chunk / start position
    int *changed;                                   // device flag
};
// d_tables: one word per stream position (deflate.hip: te_pack), d_quarter: the side table of the quarter-budget results
int launch_parse_spec(hipStream_t st, const u32 *d_tables, const u32 *d_quarter, const ChunkDesc *d_chunks, ParseBufs pb,
                      int n_segs, LevelCfg cfg, int n_chunks, u32 max_nseg /* segments of the longest chunk */);
int launch_parse_fix(hipStream_t st, const u32 *d_tables, const u32 *d_quarter, const ChunkDesc *d_chunks, ParseBufs pb,
                     int n_segs, LevelCfg cfg, int round);
int launch_parse_fix_serial(hipStream_t st, const u32 *d_tables, const u32 *d_quarter, const ChunkDesc *d_chunks, ParseBufs pb, int n_chunks,
                            LevelCfg cfg, int rounds_done);
int launch_parse_count(hipStream_t st, const u32 *d_tables, const ChunkDesc *d_chunks, ParseBufs pb,
                       int n_segs, int n_chunks, LevelCfg cfg, ChunkOut *d_cout);
int launch_parse_emit_marks(hipStream_t st, const u8 *d_stream, const u32 *d_tables, const u32 *d_quarter, const ChunkDesc *d_chunks,
                            ParseBufs pb, int rounds_done, u32 *d_tokens, u32 *d_blk_in_start, ChunkOut *d_cout, int n_chunks, u32 max_nseg);
size_t parse_marks_words(size_t n_segs);
size_t parse_cp_words();                                          // words of checkpoints per segment
int launch_block_trees(hipStream_t st, const ChunkDesc *d_chunks, const u32 *d_blk_chunk, int total_blk_cap,
                       const u32 *d_tokens, const u32 *d_blk_in_start, const ChunkOut *d_cout,
                       BlockRec *d_blocks, u32 *d_blk_codes, u32 *d_blk_hdr, int fast /* levels 1..3: deflate_fast's flush points */);
// levels 1..3 (deflate_fast): inverse map of the sorted order, the rounds of the speculative greedy walk, its in-order completion, the token pass
int launch_inverse_map(hipStream_t st, const u8 *d_stream, const TileDesc *d_tiles, int n_tiles, const u32 *d_sorted, u32 *d_inv, u32 *d_flags);
size_t fast_seq_state_bytes(int n_chunks);
int fast_list_len(int level);           // members per position in the candidate lists of levels 1..3
int fast_list_rows(int level);          // words per position (members + masks + header)
int launch_fast_cands(hipStream_t st, const u8 *d_stream, const ChunkDesc *d_chunks, const TileDesc *d_tiles, const u32 *d_sorted, const u32 *d_inv,
                      u32 *d_lists, u32 W, u32 phase, int n_chunks, int level, LevelCfg cfg);
int launch_fast_seq(hipStream_t st, const u8 *d_stream, const ChunkDesc *d_chunks, const TileDesc *d_tiles, const u32 *d_sorted, const u32 *d_inv,
                    const u32 *d_lists, u32 W, u32 phase, void *d_state, int n_chunks, int level, LevelCfg cfg, u32 *d_tokens, u32 *d_blk_in_start,
                    ChunkOut *d_cout);
int launch_block_layout(hipStream_t st, const ChunkDesc *d_chunks, int n_chunks, BlockRec *d_blocks,
                        ChunkOut *d_cout, const u64 *d_adler_acc);
int launch_block_pack(hipStream_t st, const u8 *d_stream, const ChunkDesc *d_chunks, const u32 *d_blk_chunk,
                      int total_blk_cap, const u32 *d_tokens, const BlockRec *d_blocks,
                      const u32 *d_blk_codes, const u32 *d_blk_hdr, const ChunkOut *d_cout, u8 *d_out,
                      int level);
int launch_zero_edges(hipStream_t st, const ChunkDesc *d_chunks, const u32 *d_blk_chunk, int total_blk_cap, const BlockRec *d_blocks,
                      const ChunkOut *d_cout, u8 *d_out);      // the words of the output the packer ORs into
constexpr int BLK_CODE_WORDS = 320;     // per block: 286 lit/len + 30 dist (code | len << 16), padded
constexpr int BLK_HDR_WORDS = 96;       // per block: packed dynamic-tree header bits (<= 3072 bits)

// inflate.hip
constexpr int MTS_CHUNK_NEEDMORE = 1;      // internal per-chunk status (never leaves the library: the cache answers MTS_E_MISS)
struct InfResult {
    int status;          // MTS_CHUNK_*
    u32 n_out;
    u32 ntok;
    u32 adler_stored;
    u64 end_bit;
};
struct InflateKnobs {      // the MTS_* environment of an inflate batch (inflate_knobs reads it, per batch)
    int lz_segs = 0;             // MTS_LZ_SEGS: segments per chunk of the LZ resolver, 1 .. LZ_MAXSEG (0: not set)
    long row_rounds = -1;        // MTS_INF_ROW_ROUNDS: pass A's row pool, in rounds (< 0: not set)
    bool seq = false;            // MTS_INFLATE_SEQ: every chunk through the block-after-block decoder
    int lz_workers = 0;          // MTS_LZ_WORKERS: worker waves of the LZ resolver
    u64 final_zone_bits = 0;     // MTS_SCAN_FINAL_ZONE (bytes): where the scan looks at candidates with BFINAL = 1
    bool no_rows = false, force_retry = false, lz_prof = false, debug_status = false;      // MTS_INF_NO_ROWS, MTS_LZ_FORCE_RETRY, MTS_LZ_PROF, MTS_DEBUG_STATUS
};
struct Engine;             // engine.h
InflateKnobs inflate_knobs() MTS_LOCAL;
InflateScratch inflate_scratch(const InflatePlan &P, const InflateKnobs &K) MTS_LOCAL;      // every region of the engine's inf_scratch
int launch_inflate(Engine &E, hipStream_t st, const u8 *d_cdata, const InfChunk *d_chunks, const InflatePlan &P, const InflateScratch &L,
                   const InflateKnobs &K, u8 *d_stream, u32 *d_tokens, InfResult *d_res, u64 *d_adler_acc, int *d_status_out) MTS_LOCAL;

}  // namespace mts
