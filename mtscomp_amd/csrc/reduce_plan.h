// How a reduction is fed: the part that decides and touches no device.  Which chunks go into which piece, where the compressed
// bytes of the missing chunks lie in the staging buffer, where each of them is decoded to, which chunks a piece of the halo family
// reads and what its segment table holds, how the tile family cuts and orders its tiles, how the events of waveforms and the rows of match_templates
// are cut into slabs, how mean_waveforms groups a slab's events by label, which rows and windows a workgroup of the filtered select
// counts, how the Gram slabs of the filtered Gram are gathered into z slabs.  Addresses are plain integers here: the header includes
// the C++ standard library only, so tests/plan_check.cpp, tests/snippet_plan_check.cpp, tests/tmatch_plan_check.cpp,
// tests/mean_plan_check.cpp, tests/zrank_plan_check.cpp and tests/zgram_plan_check.cpp sweep these plans on the CPU.  reduce.hip puts the
// device side around them (ChunkFeed, feed_pieces, HaloFeed, TileFeed) and says there what every caller keeps to.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "codec_plan.h"

// (what a kernel runs too: no HIP in here beyond the function attributes, as op_rank.h)
#ifdef __HIPCC__
#define MTS_PLAN_FN __host__ __device__ inline
#else
#define MTS_PLAN_FN inline
#endif

namespace mts {

// chunks [pb[p], pb[p + 1]) make piece p: a piece ends before the chunk that would take it past `piece` bytes (0: one piece)
inline std::vector<int> cut_pieces(const long *n_rows_or_bounds, bool is_bounds, int n_chunks, uint64_t row_bytes, size_t piece)
{
    std::vector<int> pb = {0};
    if (piece) {
        uint64_t acc = 0;
        for (int i = 0; i < n_chunks; i++) {
            const uint64_t n = (uint64_t)(is_bounds ? n_rows_or_bounds[i + 1] - n_rows_or_bounds[i] : n_rows_or_bounds[i]) * row_bytes;
            if (acc && acc + n > piece) { pb.push_back(i); acc = 0; }
            acc += n;
        }
    }
    pb.push_back(n_chunks);
    return pb;
}

// one piece: the missing chunks `miss` (ascending) are decoded to the piece workspace + ooff[]; a halo piece covers the op's units
// [u0, u1) and reads chunks [c0, c1] (c1 < c0: nothing to read)
struct FeedPiece {
    long u0 = 0, u1 = 0;
    int c0 = 0, c1 = -1;
    std::vector<int> miss;
    std::vector<long> ooff;
    uint64_t ws = 0;
    void add(int chunk, uint64_t bytes) { miss.push_back(chunk); ooff.push_back((long)ws); ws += (bytes + 255) / 256 * 256; }
};

// what the plans know of a call's chunks: the table, which chunks are resident (set by the owner before layout()), and the
// layout of the missing chunks' compressed bytes in the staging buffer
struct FeedPlan {
    const long *c_off, *c_len, *row0, *n_rows;
    int n_chunks;
    uint64_t row_bytes;
    bool on_device;
    std::vector<char> resident;
    std::vector<long> mcoff;                                  // per missing chunk: its compressed bytes in the staging buffer
    uint64_t ctot = 0;
    bool any_miss = false;

    FeedPlan(const long *c_off_, const long *c_len_, const long *row0_, const long *n_rows_, int n_chunks_, uint64_t row_bytes_, bool on_device_)
        : c_off(c_off_), c_len(c_len_), row0(row0_), n_rows(n_rows_), n_chunks(n_chunks_), row_bytes(row_bytes_), on_device(on_device_),
          resident(n_chunks_, 0), mcoff(n_chunks_, 0) {}

    uint64_t chunk_bytes(int i) const { return (uint64_t)n_rows[i] * row_bytes; }

    // The compressed bytes of the missing chunks lie in the staging buffer in chunk order, at mcoff[], by the run-joined rule
    // (stage_runs, codec_plan.h).  Device input stays where it is.
    // -> the first missing chunk without compressed bytes, or -1
    MTS_LOCAL int layout()
    {
        std::vector<int> miss;
        for (int i = 0; i < n_chunks; i++) {
            if (resident[i]) continue;
            if (c_len[i] == 0) return i;
            miss.push_back(i);
            if (on_device) mcoff[i] = c_off[i];
        }
        any_miss = !miss.empty();
        if (!on_device) ctot = stage_runs(c_off, c_len, miss.data(), (int)miss.size(), mcoff.data());
        return -1;
    }

    // chunks [pb[p], pb[p + 1]) are decoded in piece p: pieces of `piece` decoded bytes, resident chunks weigh nothing; device
    // input is one piece (nothing to copy beside the kernels, and smaller batches inflate slower)
    std::vector<int> piece_bounds(size_t piece) const
    {
        if (on_device) return {0, n_chunks};
        std::vector<long> weight(n_chunks, 0);
        for (int i = 0; i < n_chunks; i++) if (!resident[i]) weight[i] = n_rows[i];
        return cut_pieces(weight.data(), false, n_chunks, row_bytes, piece);
    }

    // the chunk holding `row` (clamped to the chunks)
    int chunk_of(long row) const
    {
        int lo = 0, hi = n_chunks - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) / 2; if (row0[mid] <= row) lo = mid; else hi = mid - 1; }
        return lo;
    }
};

// ---- halo family: a unit of output (outputs, rows, blocks, groups) reads rows of several adjacent chunks.  The op says which:
//   first(r)               the first unit owned by a piece that starts at file row r (any value: it is clamped to [0, n_units]);
//   rows(u0, u1, &lo, &hi) the file rows [lo, hi) that the units [u0, u1) read; lo >= hi: none (c1 < c0, every row is 0).
// Piece p owns the units from first(first row of its chunks) up to the next piece's; the pieces partition the units in order and a
// piece without units is left out.  A piece reads chunks [c0, c1] through a table of segment bases and first rows ((c1 - c0 + 1)
// bases, then (c1 - c0 + 2) first rows) and decodes the missing ones among them to ooff[] of the piece workspace: a boundary chunk
// that two pieces read is decoded in both, chunks that no unit reads are not decoded at all.
struct HaloPlan {
    std::vector<FeedPiece> pieces;
    std::vector<long> seg_at = {0};                           // piece p's table: seg[seg_at[p] ..)
    uint64_t piece_cap = 0;

    template <class First, class Rows>
    HaloPlan(const FeedPlan &F, size_t piece, long n_units, First &&first, Rows &&rows)
    {
        const std::vector<int> pb = F.piece_bounds(piece);
        const int np = (int)pb.size() - 1;
        std::vector<long> cut = {0};
        for (int p = 1; p < np; p++) cut.push_back(std::max(cut.back(), std::min(n_units, std::max(0l, (long)first(F.row0[pb[p]])))));
        cut.push_back(n_units);
        for (int p = 0; p < np; p++) {
            if (cut[p + 1] <= cut[p]) continue;
            FeedPiece P;
            P.u0 = cut[p]; P.u1 = cut[p + 1];
            long lo = 0, hi = 0;
            rows(P.u0, P.u1, &lo, &hi);
            if (lo < hi && F.n_chunks) { P.c0 = F.chunk_of(lo); P.c1 = F.chunk_of(hi - 1); }
            for (int i = P.c0; i <= P.c1; i++) if (!F.resident[i]) P.add(i, F.chunk_bytes(i));
            piece_cap = std::max(piece_cap, P.ws);
            seg_at.push_back(seg_at.back() + 2l * (P.c1 - P.c0 + 1) + 1);
            pieces.push_back(std::move(P));
        }
    }

    // the segment tables, one after the other: res_base[i] is the address of resident chunk i, out_base that of the piece workspace
    std::vector<long> tables(const FeedPlan &F, const uintptr_t *res_base, uintptr_t out_base) const
    {
        std::vector<long> seg(seg_at.back() + 1, 0);
        for (size_t p = 0; p < pieces.size(); p++) {
            const FeedPiece &P = pieces[p];
            long *b = seg.data() + seg_at[p], *r = b + (P.c1 - P.c0 + 1);
            size_t m = 0;
            for (int i = P.c0; i <= P.c1; i++) {
                b[i - P.c0] = (long)(F.resident[i] ? res_base[i] : out_base + (uintptr_t)P.ooff[m++]);
                r[i - P.c0] = F.row0[i];
            }
            r[P.c1 - P.c0 + 1] = P.c1 >= P.c0 ? F.row0[P.c1] + F.n_rows[P.c1] : 0;
        }
        return seg;
    }
};

// ---- snippets (waveforms): the events of one piece, by ascending file row, cut into slabs.  Event e reads the rows [row[e] - before,
// row[e] + after) of the filtered workspace, within the recording [vb, ve).  Slab { e0, e1, a, b } owns the events [e0, e1) and holds
// the rows [a, b) = [max(vb, row[e0] - before), min(ve, row[e1 - 1] + after)): every row of the recording that its events read.  A new
// slab starts where the next event would take b - a past cap_rows (never less than before + after: one event always fits), and where
// the next event's first row lies more than gap_rows past b, so that the rows between events far apart are not filtered
// (gap_rows < 0: never).  The slabs partition the events in order; the results do not depend on them.
struct SnippetSlab { long e0, e1, a, b; };

struct SnippetPlan {
    std::vector<SnippetSlab> slabs;
    long max_rows = 0;                                        // of a slab
    long gap_cuts = 0;                                        // slabs begun because of the gap

    SnippetPlan(const long *row, long e0, long e1, long before, long after, long vb, long ve, long cap_rows, long gap_rows)
    {
        const long cap = std::max(cap_rows, before + after);
        for (long e = e0; e < e1; e++) {
            const long a = std::max(vb, row[e] - before), b = std::min(ve, row[e] + after);
            if (!slabs.empty()) {
                SnippetSlab &S = slabs.back();
                const bool far = gap_rows >= 0 && a - S.b > gap_rows;
                if (b - S.a <= cap && !far) { S.e1 = e + 1; S.b = std::max(S.b, b); continue; }
                gap_cuts += far;
            }
            slabs.push_back({e, e + 1, a, b});
        }
        for (const SnippetSlab &S : slabs) max_rows = std::max(max_rows, S.b - S.a);
    }
};

// ---- per-label sums of snippets (mean_waveforms): the events [e0, e1) of one slab grouped by label.  perm holds the slab's events, a
// label's events together and in list order (stable); each label's run is cut into parts of at most part_events events.  Part
// { label, count, first } is perm[first - e0 .. first - e0 + count): `first` counts from the call's first event, so that the perms of
// a call's slabs, one behind the other, are one array of n_events entries.  The parts partition the slab's events; none is empty.
struct MeanPart { int label, count; long first; };

struct MeanParts {
    std::vector<long> perm;
    std::vector<MeanPart> parts;

    MeanParts(const int *label, long e0, long e1, long part_events)
    {
        const long cap = std::max(1l, part_events);
        perm.resize((size_t)(e1 > e0 ? e1 - e0 : 0));
        for (long e = e0; e < e1; e++) perm[(size_t)(e - e0)] = e;
        std::stable_sort(perm.begin(), perm.end(), [&](long a, long b) { return label[a] < label[b]; });
        for (long k = 0, n = (long)perm.size(); k < n;) {
            long run = k + 1;
            while (run < n && label[perm[(size_t)run]] == label[perm[(size_t)k]]) run++;
            for (long j = k; j < run; j += cap) parts.push_back({label[perm[(size_t)k]], (int)std::min(cap, run - j), e0 + j});
            k = run;
        }
    }
};

// ---- template events (match_templates): the rows of one piece cut into slabs of `own` owned rows.  The events of the rows [s0, s1)
// read the scores of [sa, sb) = [max(vb, s0 - R), min(ve, s1 + R)) -- every row of the recording within R -- and those the filtered rows
// [a, b) = [max(vb, sa - before), min(ve, sb + after - 1)) (b == a: they read nothing of the recording and every score is +0).  `own` is
// the largest count that keeps the score slab (sc_rows x n_out floats) and the z slab (z_rows x n_cols floats) within slab_bytes and the
// z slab within max_rows rows, and is never less than one row with its neighbours; sc_rows and z_rows bound every slab's.
struct TmatchSlab { long s0, s1, sa, sb, a, b; };

struct TmatchSlabs {
    long R, before, after, vb, ve, own, sc_rows, z_rows;

    TmatchSlabs(long n_units, long R_, long before_, long n_tau, long vb_, long ve_, long n_cols, long n_out, uint64_t slab_bytes, long max_rows)
        : R(R_), before(before_), after(n_tau - before_), vb(vb_), ve(ve_)
    {
        const long big = 1l << 40;
        const long z_fit = (long)std::min<uint64_t>(slab_bytes / (4 * (uint64_t)n_cols), (uint64_t)std::min(max_rows, big));
        const long sc_fit = (long)std::min<uint64_t>(slab_bytes / (4 * (uint64_t)n_out), (uint64_t)big);
        own = std::max(1l, std::min(n_units, std::min(z_fit - 2 * R - (n_tau - 1), sc_fit - 2 * R)));
        sc_rows = own + 2 * R;
        z_rows = sc_rows + n_tau - 1;
    }

    // the slab that starts at row s0 of a piece that ends at p1
    TmatchSlab at(long s0, long p1) const
    {
        TmatchSlab S;
        S.s0 = s0; S.s1 = std::min(p1, s0 + own);
        S.sa = std::max(vb, S.s0 - R); S.sb = std::min(ve, S.s1 + R);
        S.a = std::max(vb, S.sa - before); S.b = std::max(S.a, std::min(ve, S.sb + after - 1));
        return S;
    }
};

// ---- filtered select (k_zrank_hist, zselect.hip): the rows [s0, s1) that one launch counts, on the window grid (row_begin,
// window_rows).  Block b owns the rows [s0 + b * H, min(s1, s0 + (b + 1) * H)) and walks them in segments that end at the window
// boundaries of the grid: the segments of all blocks partition [s0, s1), none crosses a window and each names its own.  Arithmetic
// alone -- the kernel and tests/zrank_plan_check.cpp run the same functions.
struct ZrankSeg { long r0, r1, win; };                        // the rows [r0, r1) of window `win`

MTS_PLAN_FN long zrank_blocks(long s0, long s1, long H) { return s1 > s0 ? (s1 - s0 + H - 1) / H : 0; }
// the rows of block b
MTS_PLAN_FN ZrankSeg zrank_block_rows(long s0, long s1, long H, long b)
{
    const long r0 = s0 + b * H;
    return {r0, s1 - r0 < H ? s1 : r0 + H, -1};
}
// the segment that starts at row r of a block that ends at `end` (r < end; row_begin <= r)
MTS_PLAN_FN ZrankSeg zrank_segment(long r, long end, long row_begin, long window_rows)
{
    const long win = (r - row_begin) / window_rows;
    // (rows to the window's end, not its last row + 1: row_begin + (win + 1) * window_rows may pass 2^63 for a window of 2^62 rows)
    const long left = window_rows - (r - row_begin - win * window_rows);
    return {r, end - r < left ? end : r + left, win};
}

// ---- filtered Gram (filtered_gram_run, reduce.hip): the groups of mts_gram's grid, their Gram slabs, and the z slabs that a piece's
// Gram slabs go through.  The groups of a grid are adjacent in the file (a window begins where the one before it ends), so a run of
// Gram slabs is a run of rows.
// group g of the grid (range, window_rows) in groups of GR rows: its file rows [lo, hi)
inline void gram_group_rows(long range_begin, long range_end, long window_rows, long GR, long g, long *lo, long *hi)
{
    const long K = (window_rows + GR - 1) / GR;                   // groups per whole window
    const long w = g / K, k = g % K, w0 = range_begin + w * window_rows;
    const long w1 = window_rows < range_end - w0 ? w0 + window_rows : range_end;
    *lo = w0 + k * GR;
    *hi = GR < w1 - *lo ? *lo + GR : w1;
}
// the Gram slabs of a group's rows [lo, hi): SR rows each from lo, the last may be short; 2 entries (begin, end) per slab
inline void gram_cut_slabs(long lo, long hi, long SR, std::vector<long> &slab_rows)
{
    for (long r = lo; r < hi; r += SR) { slab_rows.push_back(r); slab_rows.push_back(SR < hi - r ? r + SR : hi); }
}
// the rows of z that a bound of `bytes` holds (n_cols float32 a row), rounded down to whole Gram slabs and never less than one
inline long zgram_cap_rows(uint64_t bytes, int n_cols, long SR)
{
    const uint64_t rows = bytes / (4 * (uint64_t)n_cols), most = (uint64_t)1 << 40;
    return std::max(SR, (long)(std::min(rows, most) / (uint64_t)SR) * SR);
}
// Gram slabs [s0, s1) of the call make one z slab: the rows [slab_rows[2 s0], slab_rows[2 s1 - 1])
struct ZgramSlab { long s0, s1; };
// the Gram slabs [s_begin, s_end) (adjacent rows, in order) in z slabs of at most cap_rows rows and cap_slabs Gram slabs: each takes
// whole Gram slabs while they fit, at least one (cap_rows >= SR holds any one of them)
inline std::vector<ZgramSlab> zgram_slabs(const long *slab_rows, long s_begin, long s_end, long cap_rows, long cap_slabs)
{
    std::vector<ZgramSlab> out;
    for (long s = s_begin; s < s_end;) {
        long e = s + 1;
        while (e < s_end && e - s < cap_slabs && slab_rows[2 * e + 1] - slab_rows[2 * s] <= cap_rows) e++;
        out.push_back({s, e});
        s = e;
    }
    return out;
}

// ---- tile family: the rows of every (chunk ∩ window) segment cut into tiles of tile_rows rows, in row order; a chunk's rows are
// reduced on their own, so each piece decodes exactly its own missing chunks.  Tile is the kernels' descriptor
// { base, row_lo, n_rows, chunk, pad }.
template <class Tile>
struct TilePlan {
    std::vector<Tile> tiles;
    std::vector<long> tile_win, chunk_tile0;
    std::vector<FeedPiece> pieces;
    uint64_t piece_cap = 0;
    std::vector<int> ids;                                     // the tiles in launch order: the resident chunks', then piece after piece
    std::vector<long> launch0;                                // ids [launch0[0], launch0[1]): resident, [launch0[1 + p], launch0[2 + p]): piece p

    TilePlan(const FeedPlan &F, size_t piece, long row_begin, long row_end, long window_rows, long tile_rows) : chunk_tile0(F.n_chunks + 1)
    {
        for (int i = 0; i < F.n_chunks; i++) {
            chunk_tile0[i] = (long)tiles.size();
            const long a = std::max(F.row0[i], row_begin), b = std::min(F.row0[i] + F.n_rows[i], row_end);
            for (long r = a; r < b;) {
                const long w = (r - row_begin) / window_rows, wend = row_begin + (w + 1) * window_rows, e = b < wend ? b : wend;
                for (long q = r; q < e; q += tile_rows) {
                    Tile t;
                    t.base = nullptr; t.row_lo = q - F.row0[i]; t.n_rows = (e - q) < tile_rows ? (e - q) : tile_rows; t.chunk = i; t.pad = 0;
                    tiles.push_back(t);
                    tile_win.push_back(w);
                }
                r = e;
            }
        }
        chunk_tile0[F.n_chunks] = (long)tiles.size();
        const std::vector<int> pb = F.piece_bounds(piece);
        for (size_t p = 0; p + 1 < pb.size(); p++) {
            FeedPiece P;
            for (int i = pb[p]; i < pb[p + 1]; i++) if (!F.resident[i]) P.add(i, F.chunk_bytes(i));
            if (P.miss.empty()) continue;
            piece_cap = std::max(piece_cap, P.ws);
            pieces.push_back(std::move(P));
        }
    }

    // the tiles' bases and the order of the launches (res_base, out_base as in HaloPlan::tables)
    void place(const FeedPlan &F, const uintptr_t *res_base, uintptr_t out_base)
    {
        auto take = [&](int i, uintptr_t base) {
            for (long t = chunk_tile0[i]; t < chunk_tile0[i + 1]; t++) { tiles[t].base = (decltype(tiles[t].base))base; ids.push_back((int)t); }
        };
        launch0.push_back(0);
        for (int i = 0; i < F.n_chunks; i++) if (F.resident[i]) take(i, res_base[i]);
        for (const FeedPiece &P : pieces) {
            launch0.push_back((long)ids.size());
            for (size_t z = 0; z < P.miss.size(); z++) take(P.miss[z], out_base + (uintptr_t)P.ooff[z]);
        }
        launch0.push_back((long)ids.size());
    }

    // ok[chunk]: its rows count
    void add_counts(const std::vector<int> &ok, long *count) const
    {
        for (size_t t = 0; t < tiles.size(); t++) if (ok[tiles[t].chunk]) count[tile_win[t]] += tiles[t].n_rows;
    }
};

}  // namespace mts
