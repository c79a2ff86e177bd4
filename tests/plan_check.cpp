// A seeded sweep over the plans of the device reductions and of the codec (mtscomp_amd/csrc/reduce_plan.h, codec_plan.h: no HIP in
// them), built with the address and undefined-behaviour sanitizers by `make -C mtscomp_amd/csrc plan_check` and run by
// tests/test_feed_plan.py.  Reductions: small chunk tables, every residency mask, compressed bytes with and without gaps, five piece
// sizes; the staging layout, the tile family's plan and, through a stand-in for each op's map from units to rows, the halo family's.
// Codec: the compress and inflate batch geometry at every size where the arithmetic turns (0 .. 3 bytes, a segment, the history, a
// tile, 2^31), the arrays inside the compress workspaces and the match stage's sink, every region of the inflate kernels' scratch with
// its per-chunk capacities, the sub-batch cut, the phase width of levels 1..3 and both staging rules, each property stated from what the
// kernels and the copies need, not from the code.  Exits 1 with the case printed at the first property that fails.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <random>
#include <string>

#include "reduce_plan.h"

using namespace mts;

static std::string g_case;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) { printf("FAILED %s\n  %s:%d: %s\n", g_case.c_str(), __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

struct Tile { const unsigned char *base; long row_lo, n_rows; int chunk, pad; };

struct Table {
    int n;
    std::vector<long> rows, row0, c_off, c_len;
    uint64_t row_bytes;
    long begin() const { return row0[0]; }
    long end() const { return row0[n - 1] + rows[n - 1]; }
    int holder(long r) const { for (int i = 0; i < n; i++) if (r >= row0[i] && r < row0[i] + rows[i]) return i; return -1; }
};

static const uintptr_t OUT_BASE = 0x700000000000ull;
static std::vector<uintptr_t> res_bases(int n) { std::vector<uintptr_t> v(n); for (int i = 0; i < n; i++) v[i] = 0x10000000ull * (i + 1); return v; }
static uint64_t up256(uint64_t x) { return (x + 255) / 256 * 256; }

static FeedPlan make_feed(const Table &T, unsigned mask, bool on_device)
{
    FeedPlan F(T.c_off.data(), T.c_len.data(), T.row0.data(), T.rows.data(), T.n, T.row_bytes, on_device);
    for (int i = 0; i < T.n; i++) F.resident[i] = (mask >> i) & 1;
    CHECK(F.layout() == -1);
    return F;
}

// ---- the staging layout of the missing chunks' compressed bytes
static void check_layout(const Table &T, const FeedPlan &F)
{
    int prev = -1;
    bool any = false;
    for (int i = 0; i < T.n; i++) {
        if (F.resident[i]) continue;
        any = true;
        if (F.on_device) { CHECK(F.mcoff[i] == T.c_off[i]); continue; }
        if (prev < 0) CHECK(F.mcoff[i] == 0);
        else {
            CHECK(F.mcoff[i] >= F.mcoff[prev] + T.c_len[prev]);                                   // ascending, no overlap
            if (T.c_off[i] == T.c_off[prev] + T.c_len[prev]) CHECK(F.mcoff[i] == F.mcoff[prev] + T.c_len[prev]);   // adjacent chunks keep their distance
            else CHECK(F.mcoff[i] % 16 == 0);                                                     // a gap starts at a multiple of 16
        }
        prev = i;
    }
    CHECK(F.any_miss == any);
    if (prev >= 0) CHECK(F.ctot >= (uint64_t)(F.mcoff[prev] + T.c_len[prev]) + 16);
}

// ---- what holds of every piece, of either family: where its missing chunks are decoded to
static void check_piece_outputs(const Table &T, const FeedPiece &P, uint64_t piece_cap)
{
    CHECK(P.miss.size() == P.ooff.size());
    uint64_t at = 0;
    for (size_t z = 0; z < P.miss.size(); z++) {
        if (z) CHECK(P.miss[z] > P.miss[z - 1]);
        CHECK((uint64_t)P.ooff[z] == at && P.ooff[z] % 256 == 0);
        at += up256((uint64_t)T.rows[P.miss[z]] * T.row_bytes);
    }
    CHECK(P.ws == at && P.ws <= piece_cap);
}

// ---- tile family
static void check_tiles(const Table &T, const FeedPlan &F, size_t piece, long row_begin, long row_end, long window_rows, long tile_rows)
{
    TilePlan<Tile> P(F, piece, row_begin, row_end, window_rows, tile_rows);
    const size_t nt = P.tiles.size();
    CHECK(P.tile_win.size() == nt && (int)P.chunk_tile0.size() == T.n + 1 && P.chunk_tile0[T.n] == (long)nt);
    std::vector<int> seen(T.end() - T.begin(), 0);
    for (size_t t = 0; t < nt; t++) {
        const Tile &a = P.tiles[t];
        CHECK(a.chunk >= 0 && a.chunk < T.n && a.n_rows >= 1 && a.n_rows <= tile_rows && a.row_lo >= 0 && a.row_lo + a.n_rows <= T.rows[a.chunk]);
        const long r0 = T.row0[a.chunk] + a.row_lo, r1 = r0 + a.n_rows;
        CHECK(r0 >= row_begin && r1 <= row_end);
        CHECK((r0 - row_begin) / window_rows == P.tile_win[t] && (r1 - 1 - row_begin) / window_rows == P.tile_win[t]);   // one window
        CHECK(P.chunk_tile0[a.chunk] <= (long)t && (long)t < P.chunk_tile0[a.chunk + 1]);
        if (t) CHECK(T.row0[P.tiles[t - 1].chunk] + P.tiles[t - 1].row_lo + P.tiles[t - 1].n_rows <= r0);              // ascending
        for (long r = r0; r < r1; r++) seen[r - T.begin()]++;
    }
    for (long r = T.begin(); r < T.end(); r++) CHECK(seen[r - T.begin()] == (r >= row_begin && r < row_end && T.holder(r) >= 0 ? 1 : 0));
    std::vector<int> in_piece(T.n, 0);
    uint64_t cap = 0;
    for (const FeedPiece &Q : P.pieces) {
        CHECK(!Q.miss.empty());
        for (int i : Q.miss) in_piece[i]++;
        check_piece_outputs(T, Q, P.piece_cap);
        cap = std::max(cap, Q.ws);
    }
    CHECK(cap == P.piece_cap);
    for (int i = 0; i < T.n; i++) CHECK(in_piece[i] == (F.resident[i] ? 0 : 1));
    for (size_t p = 1; p < P.pieces.size(); p++) CHECK(P.pieces[p].miss.front() > P.pieces[p - 1].miss.back());
    // launch order: the resident chunks' tiles, then piece after piece
    const std::vector<uintptr_t> rb = res_bases(T.n);
    P.place(F, rb.data(), OUT_BASE);
    CHECK(P.ids.size() == nt && P.launch0.size() == P.pieces.size() + 2 && P.launch0.front() == 0 && P.launch0.back() == (long)nt);
    std::vector<int> used(nt, 0);
    for (int id : P.ids) { CHECK(id >= 0 && id < (int)nt); used[id]++; }
    for (size_t t = 0; t < nt; t++) CHECK(used[t] == 1);
    for (size_t k = 0; k + 1 < P.launch0.size(); k++) {
        CHECK(P.launch0[k] <= P.launch0[k + 1]);
        for (long z = P.launch0[k]; z < P.launch0[k + 1]; z++) {
            const Tile &a = P.tiles[P.ids[z]];
            if (k == 0) CHECK(F.resident[a.chunk] && (uintptr_t)a.base == rb[a.chunk]);
            else {
                const FeedPiece &Q = P.pieces[k - 1];
                const auto it = std::find(Q.miss.begin(), Q.miss.end(), a.chunk);
                CHECK(it != Q.miss.end() && (uintptr_t)a.base == OUT_BASE + (uintptr_t)Q.ooff[it - Q.miss.begin()]);
            }
            if (z > P.launch0[k]) CHECK(P.ids[z] > P.ids[z - 1]);
        }
    }
}

// ---- halo family
typedef std::function<long(long)> FirstFn;
typedef std::function<void(long, long, long *, long *)> RowsFn;

// slack: [c0, c1] is exactly the span of the chunks that the units read (0), or may reach up to `slack` rows further at either end
static void check_halo(const Table &T, const FeedPlan &F, size_t piece, long n_units, const FirstFn &first, const RowsFn &rows, long slack = 0)
{
    HaloPlan H(F, piece, n_units, first, rows);
    CHECK(H.seg_at.size() == H.pieces.size() + 1 && H.seg_at[0] == 0);
    const std::vector<uintptr_t> rb = res_bases(T.n);
    const std::vector<long> seg = H.tables(F, rb.data(), OUT_BASE);
    CHECK((long)seg.size() == H.seg_at.back() + 1);
    long u = 0;
    uint64_t cap = 0;
    for (size_t p = 0; p < H.pieces.size(); p++) {
        const FeedPiece &P = H.pieces[p];
        CHECK(P.u0 == u && P.u1 > P.u0);                                       // a partition of the units, in order, no piece empty
        u = P.u1;
        // the chunks that the piece's units read, unit by unit
        int b0 = T.n, b1 = -1;
        long lo_min = T.end(), hi_max = T.begin();
        for (long k = P.u0; k < P.u1; k++) {
            long lo = 0, hi = 0;
            rows(k, k + 1, &lo, &hi);
            if (lo >= hi) continue;
            CHECK(T.holder(lo) >= 0 && T.holder(hi - 1) >= 0);                 // (the stand-ins keep to the chunks, as check_cover has it)
            b0 = std::min(b0, T.holder(lo)); b1 = std::max(b1, T.holder(hi - 1));
            lo_min = std::min(lo_min, lo); hi_max = std::max(hi_max, hi);
        }
        if (b1 < 0) CHECK(P.c1 < P.c0 || P.c1 - P.c0 + 1 <= slack);
        else {
            CHECK(P.c0 <= b0 && P.c1 >= b1);
            CHECK(T.row0[P.c0] + T.rows[P.c0] > lo_min - slack && T.row0[P.c1] < hi_max + slack);   // (slack 0: c0 == b0 and c1 == b1)
        }
        // miss: the non-resident chunks of [c0, c1], so a chunk that two pieces read is in both
        std::vector<int> want;
        for (int i = P.c0; i <= P.c1; i++) if (!F.resident[i]) want.push_back(i);
        CHECK(P.miss == want);
        for (size_t o = 0; o < p; o++)
            for (int i : want) if (i >= H.pieces[o].c0 && i <= H.pieces[o].c1) CHECK(std::count(H.pieces[o].miss.begin(), H.pieces[o].miss.end(), i) == 1);
        check_piece_outputs(T, P, H.piece_cap);
        cap = std::max(cap, P.ws);
        // the table: ns bases, then ns + 1 first rows
        const int ns = std::max(0, P.c1 - P.c0 + 1);
        CHECK(H.seg_at[p + 1] - H.seg_at[p] == 2 * ns + 1);
        const long *b = seg.data() + H.seg_at[p], *r = b + ns;
        size_t m = 0;
        for (int k = 0; k < ns; k++) {
            const int i = P.c0 + k;
            CHECK((uintptr_t)b[k] == (F.resident[i] ? rb[i] : OUT_BASE + (uintptr_t)P.ooff[m++]));
            CHECK(r[k] == T.row0[i] && r[k] < r[k + 1]);
        }
        CHECK(r[ns] == (ns ? T.row0[P.c1] + T.rows[P.c1] : 0));
    }
    CHECK(u == n_units && cap == H.piece_cap);
}

// the five ops' maps from units to rows (reduce.hip), at small parameters, on the rows [b, e) of the table
static void check_halo_ops(const Table &T, const FeedPlan &F, size_t piece, long a, long z)
{
    const long b = T.begin(), e = T.end(), rb = std::min(b + a, e - 1), re = std::max(e - z, rb + 1);
    const std::string base = g_case;
    // decimate: output k's newest row is first_row + k q, its support L rows; outputs lie inside the valid range [b, e), or begin
    // before and end behind it -- pieces with nothing to read.  With L < q the rows between two supports are read by no output, and a
    // piece whose first or last outputs lie outside the range reads from the clamp, up to q - 1 rows away from the nearest row that
    // an output reads: there [c0, c1] may hold a chunk that no output reads, never one too few.
    for (long q : {1l, 3l}) for (long L : {1l, 5l, 90l}) for (int outside = 0; outside < 2; outside++) {
        g_case = base + " decimate q=" + std::to_string(q) + " L=" + std::to_string(L) + " outside=" + std::to_string(outside);
        const long first_row = outside ? b - 7 + a : rb, last = outside ? e + 5 : re - 1, n_out = (last - first_row) / q + 1;
        check_halo(T, F, piece, n_out, [=](long r) { return r <= first_row ? 0 : (r - first_row + q - 1) / q; },
                   [=](long u0, long u1, long *lo, long *hi) { *lo = std::max(b, first_row + u0 * q - (L - 1)); *hi = std::min(e, first_row + (u1 - 1) * q + 1); },
                   outside && L < q ? q - 1 : 0);
    }
    // project: the unit is a row of [rb, re), the halo is empty
    g_case = base + " project";
    check_halo(T, F, piece, re - rb, [=](long r) { return r - rb; }, [=](long u0, long u1, long *lo, long *hi) { *lo = rb + u0; *hi = rb + u1; });
    // detect: a row's events read R rows either side and the filter's support
    for (long R : {0l, 2l}) for (long L : {1l, 5l}) {
        g_case = base + " detect R=" + std::to_string(R) + " L=" + std::to_string(L);
        const long half = (L - 1) / 2;
        check_halo(T, F, piece, re - rb, [=](long r) { return r - rb; },
                   [=](long u0, long u1, long *lo, long *hi) { *lo = std::max(b, rb + u0 - R + half - (L - 1)); *hi = std::min(e, rb + u1 + R + half); });
    }
    // welch: blocks of 32 segments of 16 rows
    for (long step : {8l, 16l}) {
        g_case = base + " welch step=" + std::to_string(step);
        const long B = 32, nperseg = 16, n_seg = (e - rb - nperseg) / step + 1;
        if (e - rb < nperseg) continue;
        check_halo(T, F, piece, (n_seg + B - 1) / B, [=](long r) { return r <= rb ? 0 : (r - rb + step * B - 1) / (step * B); },
                   [=](long u0, long u1, long *lo, long *hi) { *lo = rb + u0 * B * step; *hi = rb + (std::min(n_seg, u1 * B) - 1) * step + nperseg; });
    }
    // gram: windows of 100 rows in groups of 64 (the last group of a window is short), slabs of 16
    {
        g_case = base + " gram";
        const long W = 100, GR = 64, K = (W + GR - 1) / GR, n_range = re - rb, n_groups = n_range / W * K + (n_range % W + GR - 1) / GR;
        auto group_rows = [=](long g, long *lo, long *hi) {
            const long w0 = rb + g / K * W;
            *lo = w0 + g % K * GR; *hi = std::min(*lo + GR, std::min(w0 + W, re));
        };
        std::vector<long> glo(n_groups);
        for (long g = 0; g < n_groups; g++) { long hi; group_rows(g, &glo[g], &hi); }
        check_halo(T, F, piece, n_groups, [&](long r) { return (long)(std::lower_bound(glo.begin(), glo.end(), r) - glo.begin()); },
                   [&](long u0, long u1, long *lo, long *hi) { long t; group_rows(u0, lo, &t); group_rows(u1 - 1, &t, hi); });
    }
    g_case = base;
}

// ================================================================================================
// the codec's plans (codec_plan.h)
// ================================================================================================
typedef unsigned long long ull;
static size_t dim_sort_ws(int n_tiles) { return (size_t)(n_tiles + 1) * 48; }
static size_t dim_marks(size_t n_segs) { return (n_segs + 64) / 64 * 64 * 4; }
static const CompressDims DIMS = {dim_sort_ws, dim_marks, 14, 40, 24, 320, 96, MATCH_SINK_BYTES};
static const ull TWO31 = 1ull << 31;

// ---- a compress batch: chunk i is n[i] bytes (raw_is_stream: bounds in bytes; else rows of row_bytes)
static void check_compress(const std::vector<ull> &rows, ull row_bytes, bool raw_is_stream, int level)
{
    const int nc = (int)rows.size();
    std::vector<long> bounds(nc + 1, 5), slots(nc);
    std::vector<ull> n(nc);
    for (int i = 0; i < nc; i++) { bounds[i + 1] = bounds[i] + (long)rows[i]; n[i] = raw_is_stream ? rows[i] : rows[i] * row_bytes; slots[i] = 16l * i * 1000; }
    const CompressPlan P(bounds.data(), nc, row_bytes, raw_is_stream, slots.data(), level, DIMS);
    bool too_big = false;
    for (int i = 0; i < nc; i++) too_big = too_big || n[i] >= TWO31;
    CHECK((P.error[0] != 0) == too_big);                                             // 2^31 - 1 accepted, 2^31 refused
    if (too_big) { CHECK(strstr(P.error, "2 GiB")); return; }
    CHECK((int)P.cd.size() == nc);
    ull seg = 0, blk = 0, tile = 0, max_n = 0, max_rows = 0, max_nseg = 0;
    for (int i = 0; i < nc; i++) {
        const ChunkDesc &c = P.cd[i];
        CHECK(c.n == n[i] && c.n_rows == rows[i] && c.out_off == (ull)slots[i]);     // (no 32-bit field wraps)
        CHECK(c.raw_off == (ull)(bounds[i] - bounds[0]) * (raw_is_stream ? 1 : row_bytes));
        // streams: aligned, disjoint, STREAM_PAD bytes behind each; tokens: disjoint, room for n + 1
        const ull s_end = i + 1 < nc ? P.cd[i + 1].stream_off : P.stream_bytes, t_end = i + 1 < nc ? P.cd[i + 1].tok_off : P.tok_words;
        CHECK(c.stream_off % STREAM_ALIGN == 0 && c.stream_off + n[i] + STREAM_PAD <= s_end);
        CHECK(c.tok_off + n[i] + 1 <= t_end);
        // segments and block slots partition their ranges
        CHECK(c.seg0 == seg && c.nseg == (n[i] + SEG - 1) / SEG && c.blk0 == blk && c.blk_cap == n[i] / BLOCK_TOKENS + 2);
        seg += c.nseg; blk += c.blk_cap;
        // tiles: a partition of [0, n) in order
        CHECK(c.tile0 == tile);
        ull at = 0;
        while (at < n[i]) {
            CHECK(tile < P.tiles.size());
            const TileDesc &t = P.tiles[tile];
            CHECK(t.chunk == (u32)i && t.n == n[i] && t.stream_off == c.stream_off);
            CHECK(t.a == at && t.own_end > t.a && t.own_end - t.a <= (ull)TILE && t.own_end <= n[i]);
            CHECK(t.own_end == n[i] || t.own_end - t.a == (ull)TILE);
            CHECK(t.w == (t.a > (ull)HALO ? t.a - HALO : 0));
            // the hashed window: every position has three bytes, and it reaches the last owned position that has
            if (n[i] < 3) CHECK(t.wlen == 0);
            else {
                CHECK(t.wlen > 0 && (ull)t.w + t.wlen - 1 <= n[i] - 3);
                CHECK((ull)t.w + t.wlen == std::min<ull>(t.own_end, n[i] - 2));
                CHECK(t.wlen <= (ull)WIN);
            }
            // sorted regions: 64-aligned, disjoint, inside both sort buffers
            const ull so_end = tile + 1 < P.tiles.size() ? P.tiles[tile + 1].sorted_off : P.sort_n;
            CHECK(t.sorted_off % 64 == 0 && t.sorted_off + t.wlen <= so_end);
            at = t.own_end; tile++;
        }
        CHECK(at == n[i]);
        max_n = std::max(max_n, n[i]); max_rows = std::max(max_rows, rows[i]); max_nseg = std::max<ull>(max_nseg, c.nseg);
    }
    CHECK(tile == P.tiles.size() && seg == P.nseg && blk == P.nblk);
    CHECK(P.max_n == max_n && P.max_rows == max_rows && P.max_nseg == max_nseg);
    // the workspaces hold what is laid out in them
    CHECK(P.sort_a >= P.sort_n * 4 && P.sort_a >= dim_marks(seg + 64) * 4 && P.sort_b >= P.sort_n * 4 && P.sort_ws >= dim_sort_ws((int)tile));
    CHECK(P.tables >= (P.stream_bytes + 64) * 4 * (level < 4 ? 1 : 2) && P.table_words >= P.stream_bytes && P.table_words % 64 == 0);
    CHECK(P.tokens >= (P.tok_words + 64) * 4 && P.segbuf >= (seg + 64) * 4 * (7 + 14) && P.blk >= (blk + 1) * (40 + 8));
    CHECK(P.blkcodes >= (blk + 1) * 320 * 4 && P.blkhdr >= (blk + 1) * 96 * 4 && P.adler >= 16ull * nc + 8 + 65536 && P.misc >= 12ull * nc);
    CHECK(P.o_chunks % 256 == 0 && P.o_tiles % 256 == 0 && P.o_cout % 256 == 0);
    CHECK(P.o_chunks + sizeof(ChunkDesc) * nc <= P.o_tiles && P.o_tiles + sizeof(TileDesc) * (tile + 1) <= P.o_cout && P.o_cout + 24ull * nc <= P.desc);
    // the arrays inside segbuf, blk, adler and misc: apart, and inside the bytes the plan asks for
    {
        struct Sub { size_t off, bytes; };
        auto apart = [&](std::vector<Sub> v, size_t cap) {
            std::sort(v.begin(), v.end(), [](const Sub &a, const Sub &b) { return a.off < b.off; });
            for (size_t k = 0; k < v.size(); k++) CHECK(v[k].off + v[k].bytes <= (k + 1 < v.size() ? v[k + 1].off : cap));
        };
        const size_t SN = (seg + 64) * 4, BN = blk + 1;                                 // a per-segment array in bytes; block slots and one more
        apart({{P.seg.entry * 4, SN}, {P.seg.exit_a * 4, SN}, {P.seg.exit_b * 4, SN}, {P.seg.cnt * 4, SN}, {P.seg.tokbase * 4, SN}, {P.seg.seg_chunk * 4, SN},
               {P.seg.seg_start * 4, SN}, {P.seg.cp * 4, SN * DIMS.parse_cp_words}}, P.segbuf);
        apart({{P.bk.blocks, BN * DIMS.block_rec_bytes}, {P.bk.chunk, BN * 4}, {P.bk.in_start, BN * 4}}, P.blk);
        CHECK(P.bk.blocks % 8 == 0 && P.bk.chunk % 4 == 0 && P.bk.in_start % 4 == 0);
        // the match stage's sink: MATCH_SINK_LINES lines of MATCH_SINK_LINE_WORDS words from word MATCH_SINK_WORD0 behind the first flag word;
        // a workgroup's line is its index under the mask, a lane's word its number in the wave
        const size_t sink_words = (size_t)MATCH_SINK_WORD0 + (size_t)(MATCH_SINK_LINES - 1) * MATCH_SINK_LINE_WORDS + 63 + 1;
        CHECK(P.ad.sink == P.ad.flags + 4 * (size_t)MATCH_SINK_WORD0 && P.ad.flags + 4 * sink_words <= P.adler);
        apart({{P.ad.sums, 16ul * nc}, {P.ad.changed, 4}, {P.ad.flags, 4}, {P.ad.sink, 4 * sink_words - 4 * (size_t)MATCH_SINK_WORD0}}, P.adler);
        CHECK(P.ad.flags == P.ad.changed + 4 && P.ad.changed % 4 == 0);                // (the two flag words are cleared and read as one 8-byte range)
        apart({{P.mi.so, 8ul * nc}, {P.mi.nn, 4ul * nc}}, P.misc);
        CHECK(P.mi.so % 8 == 0 && P.mi.nn % 4 == 0);
    }
    // the index arrays agree with cd
    std::vector<u32> h_seg, h_blk;
    P.index_arrays(h_seg, h_blk);
    CHECK(h_seg.size() == 2 * seg && h_blk.size() >= blk);
    for (int i = 0; i < nc; i++) {
        const ChunkDesc &c = P.cd[i];
        for (u32 k = 0; k < c.nseg; k++) CHECK(h_seg[c.seg0 + k] == (u32)i && h_seg[seg + c.seg0 + k] == k * (u32)SEG && (ull)k * SEG < n[i]);
        for (u32 k = 0; k < c.blk_cap; k++) CHECK(h_blk[c.blk0 + k] == (u32)i);
    }
}

// ---- an inflate batch
static void check_inflate(const std::vector<ull> &rows, int nc, int sz, int nc_full)
{
    const int n = (int)rows.size();
    std::vector<long> c_off(n), c_len(n), n_rows(n), out_off(n);
    for (int i = 0; i < n; i++) { c_off[i] = 100l * i; c_len[i] = 50 + i; n_rows[i] = (long)rows[i]; out_off[i] = 4096l * i; }
    const InflatePlan P(c_off.data(), c_len.data(), n_rows.data(), out_off.data(), n, nc, sz, nc_full, 24);
    const ull row_bytes = (ull)(nc_full ? nc_full : nc) * sz;
    bool too_big = false;
    for (int i = 0; i < n; i++) too_big = too_big || rows[i] * row_bytes >= TWO31;
    CHECK((P.error[0] != 0) == too_big);
    if (too_big) return;
    ull max_n = 0, max_rows = 0;
    for (int i = 0; i < n; i++) {
        const InfChunk &c = P.ic[i];
        const ull bytes = rows[i] * row_bytes;
        CHECK(c.c_off == (ull)c_off[i] && c.c_len == (ull)c_len[i] && c.n_expect == bytes);
        const ull s_end = i + 1 < n ? P.ic[i + 1].stream_off : P.stream_bytes(), t_end = i + 1 < n ? P.ic[i + 1].tok_off : P.toff;
        CHECK(c.stream_off % STREAM_ALIGN == 0 && c.stream_off + bytes + STREAM_PAD <= s_end);
        CHECK(c.tok_off % 4 == 0 && c.tok_off + bytes + 2 <= t_end);                     // 16-byte aligned, room for n + 2 tokens
        if (!nc_full) CHECK(c.n_need == 0);
        else CHECK(c.n_need >= 1 && c.n_need == std::max<ull>(1, rows[i] * nc * sz) && c.n_need <= std::max<ull>(1, bytes));
        CHECK(P.so[i] == c.stream_off && P.nn[i] == bytes && P.oo[i] == (ull)out_off[i] && P.rows[i] == rows[i]);
        max_n = std::max(max_n, bytes); max_rows = std::max(max_rows, rows[i]);
    }
    CHECK(P.max_n == max_n && P.max_rows == max_rows && P.token_bytes() >= (P.toff + 64) * 4);
    // descriptor regions: disjoint, 256-aligned, the host's part at the head
    const size_t off[] = {P.o_ic, P.o_so, P.o_nn, P.o_oo, P.o_rows, P.o_res, P.o_status, P.o_end};
    const size_t size[] = {sizeof(InfChunk) * n, 8ul * n, 4ul * n, 8ul * n, 4ul * n, 24ul * n, 4ul * n};
    for (int r = 0; r < 7; r++) CHECK(off[r] % 256 == 0 && off[r] + size[r] <= off[r + 1]);
    CHECK(P.o_ic == 0 && P.host_bytes == P.o_res);
    std::vector<u8> h(P.host_bytes, 0);
    P.fill(h.data());
    CHECK(!memcmp(h.data() + P.o_ic, P.ic.data(), size[0]) && !memcmp(h.data() + P.o_so, P.so.data(), size[1]) && !memcmp(h.data() + P.o_nn, P.nn.data(), size[2]) &&
          !memcmp(h.data() + P.o_oo, P.oo.data(), size[3]) && !memcmp(h.data() + P.o_rows, P.rows.data(), size[4]));
}

// ---- the scratch of an inflate batch: chunk i is c_len[i] compressed bytes that inflate to n[i]
static long n_scratch = 0;
static const InflateDims IDIMS ={32, 24, 268, 512, 192, 8, 256, 32, 32768, 4096, 2};      // (inflate.hip's records and constants)

static void check_inflate_scratch(const std::vector<ull> &n, const std::vector<ull> &c_len, int lz_segs, long row_rounds)
{
    const int nc = (int)n.size();
    std::vector<long> c_off(nc), c_l(nc), n_rows(nc), out_off(nc);
    for (int i = 0; i < nc; i++) { c_off[i] = 5000l * i; c_l[i] = (long)c_len[i]; n_rows[i] = (long)n[i]; out_off[i] = 0; }
    const InflatePlan P(c_off.data(), c_l.data(), n_rows.data(), out_off.data(), nc, 1, 1, 0, 24);
    CHECK(!P.error[0]);
    const InflateScratch L(P, IDIMS, lz_segs, row_rounds);
    // a direct recount of what the kernels index with
    const ull GS = IDIMS.gs_tile;
    std::vector<ull> cap(nc), cand0(nc + 1, 0), g(nc), g0(nc + 1, 0), t0(nc + 1, 0);
    ull cbits = 0, cells = 0, share = 0, max_clen = 0, max_groups = 1;
    for (int i = 0; i < nc; i++) {
        cap[i] = c_len[i] / 4096 + 64; cand0[i + 1] = cand0[i] + cap[i];
        g[i] = (n[i] + 2 + 63) / 64 + 2;                                                 // groups of 64 tokens (tokens <= bytes + 1), and two more
        g0[i + 1] = g0[i] + g[i]; t0[i + 1] = t0[i] + g[i] / GS + 2;
        cbits += 8 * c_len[i]; cells += up256(n[i] + STREAM_PAD); share += c_len[i] * 8 / (64 * 640) + 32;
        max_clen = std::max(max_clen, c_len[i]); max_groups = std::max(max_groups, (n[i] + 2 + 63) / 64);
    }
    const ull tc = cand0[nc], tt = 2 * tc;
    const int nseg = std::min(lz_segs ? lz_segs : nc < 128 ? 256 / nc : 1, (int)IDIMS.lz_maxseg);
    const ull rounds = std::min<ull>(row_rounds >= 0 ? (ull)row_rounds : share, 0x3ffffffull);
    CHECK(L.nseg == nseg && L.rounds_cap == rounds && L.total_cand == tc && L.total_true == tt && tt < (1ull << 32));
    CHECK(L.surv_cap == cbits / 256 + 65536 && L.max_clen == max_clen && L.max_groups == max_groups);
    // every region: 256-aligned, in the order of the members, disjoint, inside [0, end)
    const struct { const char *name; size_t off; } members[] = {
        {"so", L.so}, {"nn", L.nn}, {"fast", L.fast}, {"gb_off", L.gb_off}, {"tb_off", L.tb_off}, {"cand_cnt", L.cand_cnt}, {"true_cnt", L.true_cnt},
        {"seq_flag", L.seq_flag}, {"slot_chunk", L.slot_chunk}, {"tslot_chunk", L.tslot_chunk}, {"cand_pos", L.cand_pos}, {"cand_tmp", L.cand_tmp},
        {"cres", L.cres}, {"tblk", L.tblk}, {"subs", L.subs}, {"gbase", L.gbase}, {"tile_base", L.tile_base}, {"surv", L.surv}, {"surv_cnt", L.surv_cnt},
        {"plan", L.plan}, {"win", L.win}, {"rows_cells", L.rows_cells}, {"round_row", L.round_row}, {"row_ctr", L.row_ctr}, {"gflag", L.gflag},
        {"seg_adler", L.seg_adler}};
    const size_t NR = sizeof members / sizeof members[0];
    CHECK(L.regions.size() == NR && L.regions[0].off == 0);
    auto bytes_of = [&](const char *name) { for (const auto &r : L.regions) if (!strcmp(r.name, name)) return r.bytes; CHECK(!"region"); return (size_t)0; };
    for (size_t r = 0; r < NR; r++) {
        CHECK(!strcmp(L.regions[r].name, members[r].name) && L.regions[r].off == members[r].off && members[r].off % 256 == 0);
        CHECK(members[r].off + L.regions[r].bytes <= (r + 1 < NR ? members[r + 1].off : L.end));
    }
    CHECK(L.end % 256 == 0);
    // what each region must hold
    const ull un = (ull)nc;
    CHECK(bytes_of("so") >= 8 * un && bytes_of("nn") >= 4 * un && bytes_of("fast") >= 24 * un && bytes_of("gb_off") >= 8 * un && bytes_of("tb_off") >= 8 * un);
    CHECK(bytes_of("cand_cnt") >= 4 * un && bytes_of("true_cnt") >= 4 * un && bytes_of("seq_flag") >= 4 * un && bytes_of("plan") >= IDIMS.lz_plan_bytes * un);
    CHECK(bytes_of("slot_chunk") >= 4 * tc && bytes_of("tslot_chunk") >= 4 * tt && bytes_of("cand_pos") >= 8 * tc && bytes_of("cand_tmp") >= 8 * tc);
    CHECK(bytes_of("cres") >= IDIMS.cand_res_bytes * tc && bytes_of("tblk") >= IDIMS.true_blk_bytes * tt && bytes_of("subs") >= 8ull * IDIMS.subcap * tc);
    CHECK(bytes_of("round_row") >= 4ull * IDIMS.rounds_max * tc && bytes_of("row_ctr") >= 4 && bytes_of("surv_cnt") >= 4 && bytes_of("surv") >= 8ull * L.surv_cap);
    CHECK(bytes_of("gbase") >= 4 * g0[nc] && bytes_of("tile_base") >= 4 * t0[nc]);
    // the per-chunk ranges partition their regions: candidate slots, twice as many true-block slots, group bases, tile bases
    for (int i = 0; i < nc; i++) {
        const InfFast &f = L.h_fast[i];
        CHECK(f.cand_off == cand0[i] && f.cand_cap == cap[i] && f.true_off == 2 * cand0[i] && f.true_cap == 2 * cap[i] && f.pad == 0);
        CHECK(L.gb[i] == g0[i] && L.tb[i] == t0[i]);
        CHECK(InflateScratch::groups_of((u32)n[i]) == g[i] && InflateScratch::tiles_of((u32)n[i], IDIMS.gs_tile) == g[i] / GS + 2);
        CHECK(g[i] * 64 >= n[i] + 1 + 2 * 64 && (g[i] / GS + 2) * GS >= g[i] + GS);     // room for every token, and slack of two groups / a tile
    }
    // the host row: five regions in a row at the head, one copy; fill writes them and nothing else
    CHECK(L.host_off == L.so && L.host_off + L.host_bytes == L.cand_cnt && L.so < L.nn && L.nn < L.fast && L.fast < L.gb_off && L.gb_off < L.tb_off);
    std::vector<u8> h(L.host_bytes, 0xEE), want(L.host_bytes, 0xEE);
    L.fill(h.data());
    memcpy(want.data() + (L.so - L.host_off), P.so.data(), 8 * un); memcpy(want.data() + (L.nn - L.host_off), P.nn.data(), 4 * un);
    memcpy(want.data() + (L.gb_off - L.host_off), g0.data(), 8 * un); memcpy(want.data() + (L.tb_off - L.host_off), t0.data(), 8 * un);
    for (int i = 0; i < nc; i++) {
        const InfFast f = {cand0[i], (u32)cap[i], (u32)(2 * cand0[i]), (u32)(2 * cap[i]), 0};
        memcpy(want.data() + (L.fast - L.host_off) + sizeof f * i, &f, sizeof f);
    }
    CHECK(h == want);
    // the range the resolver zeroes: gflag and seg_adler, in two clears that meet, and nothing else (they are the last two regions)
    CHECK(L.clear[0].off == L.gflag && L.clear[0].off + L.clear[0].bytes == L.clear[1].off && L.clear[1].off == L.seg_adler);
    CHECK(L.clear[0].bytes >= bytes_of("gflag") && L.clear[1].bytes == bytes_of("seg_adler") && L.clear[1].off + L.clear[1].bytes <= L.end);
    CHECK(L.gflag > L.row_ctr && L.seg_adler >= L.gflag && (nseg > 1 || L.clear[0].bytes + L.clear[1].bytes == 0));
    // one region for pass A's token rows and the resolver's cells: it holds the larger
    CHECK(bytes_of("rows_cells") >= rounds * 64 * IDIMS.rowcap * 4 && bytes_of("rows_cells") >= (nseg > 1 ? 2 * cells : 0));
    // windows, flags and check sums: there exactly when the chunks are cut
    CHECK((bytes_of("win") == 0) == (nseg == 1) && (bytes_of("gflag") == 0) == (nseg == 1) && (bytes_of("seg_adler") == 0) == (nseg == 1));
    if (nseg > 1) CHECK(bytes_of("win") >= un * IDIMS.lz_maxseg * IDIMS.lz_win && bytes_of("gflag") >= cells / IDIMS.lz_flush + un &&
                        bytes_of("seg_adler") >= un * IDIMS.lz_maxseg * IDIMS.lz_flushers * 16);
}

// ---- the sub-batch cut
static void check_cut(const std::vector<size_t> &bytes, size_t budget, int max_chunks)
{
    const int n = (int)bytes.size();
    const std::vector<int> b = cut_batches([&](int i) { return bytes[i]; }, n, budget, max_chunks);
    CHECK(!b.empty() && b.front() == 0 && b.back() == n);
    for (size_t k = 0; k + 1 < b.size(); k++) {
        CHECK(b[k] < b[k + 1] && b[k + 1] - b[k] <= max_chunks);                         // in order, none empty, none too long
        size_t sum = 0;
        for (int i = b[k]; i < b[k + 1]; i++) sum += bytes[i];
        CHECK(sum <= budget || b[k + 1] - b[k] == 1);                                    // over the budget only when alone
        if (b[k + 1] < n) CHECK(sum + bytes[b[k + 1]] > budget || b[k + 1] - b[k] == max_chunks);   // maximal
    }
    if (n == 0) CHECK(b.size() == 1);
}

// ---- the phase width of levels 1..3
static void check_phase_width(ull budget, int n_chunks, ull K, u32 max_n)
{
    const ull W = CompressPlan::phase_width(budget, n_chunks, K, max_n);
    if (max_n == 0) return;                                                              // (nothing to walk: no lists are made)
    CHECK(W >= 256 && W % 256 == 0);
    CHECK(W == 256 || 2 * (ull)n_chunks * W * K * 4 <= budget);                          // both list buffers within the budget
    const ull phases = (max_n + W - 1) / W;
    CHECK(phases * W >= max_n && W <= std::max<ull>(256, align_up(max_n, 256)));         // the phases cover max_n, and no more than that
    // at least 8 phases when max_n allows: wider than 1024 only up to an eighth of max_n (in whole granules of 256)
    CHECK(W <= 1024 || W <= align_up((max_n + 7ull) / 8, 256));
    if (max_n % 2048 == 0 && W > 1024) CHECK(phases >= 8);
}

// ---- staging: the copies carry every listed chunk's bytes to where the layout says, once
struct Staged {
    std::vector<int> writes;                                                             // per staging byte
    std::vector<long> from;                                                              // ... and the caller's offset it came from
    explicit Staged(ull ctot) : writes(ctot, 0), from(ctot, -1) {}
    void apply(const std::vector<StageCopy> &cp)
    {
        for (const StageCopy &c : cp) {
            CHECK(c.len > 0 && c.dst >= 0 && c.src >= 0 && (ull)c.dst + c.len <= writes.size());
            for (ull b = 0; b < c.len; b++) { writes[c.dst + b]++; from[c.dst + b] = c.src + (long)b; }
        }
    }
    void holds(long soff, long c_off, long c_len) const { for (long b = 0; b < c_len; b++) CHECK(writes[soff + b] == 1 && from[soff + b] == c_off + b); }
};

static void check_run_staging(const std::vector<long> &c_off, const std::vector<long> &c_len, const std::vector<int> &ids, int piece_chunks, bool expect_one_copy)
{
    const int n = (int)c_off.size(), m = (int)ids.size();
    std::vector<long> soff(n, -1);
    const ull ctot = stage_runs(c_off.data(), c_len.data(), ids.data(), m, soff.data());
    ull end = 0;
    for (int k = 0; k < m; k++) {
        const int i = ids[k];
        CHECK(soff[i] >= 0);
        for (int q = 0; q < k; q++) { const int j = ids[q]; CHECK(soff[i] >= soff[j] + c_len[j] || soff[j] >= soff[i] + c_len[i]); }   // disjoint
        if (k) {
            const int p = ids[k - 1];
            if (c_off[i] == c_off[p] + c_len[p]) CHECK(soff[i] == soff[p] + c_len[p]);   // back to back: the distance is kept
            else CHECK(soff[i] % 16 == 0);                                               // a gap: the run starts 16-aligned
        } else CHECK(soff[i] % 16 == 0);
        end = std::max<ull>(end, soff[i] + c_len[i]);
    }
    CHECK(ctot >= end + 16);
    // the copies, piece by piece (piece_chunks listed chunks each, the last chunk of a piece listed again in the next: a halo)
    Staged S(ctot);
    std::vector<char> done(n, 0);
    ull moved = 0, want = 0;
    for (int k0 = 0; k0 < m; k0 += piece_chunks) {
        const int a = k0 ? k0 - 1 : 0, e = std::min(m, k0 + piece_chunks);
        const std::vector<StageCopy> cp = run_copies(c_off.data(), c_len.data(), soff.data(), ids.data() + a, e - a, done.data());
        if (expect_one_copy) CHECK(cp.size() == 1);
        for (const StageCopy &c : cp) moved += c.len;
        S.apply(cp);
    }
    for (int k = 0; k < m; k++) { S.holds(soff[ids[k]], c_off[ids[k]], c_len[ids[k]]); want += c_len[ids[k]]; }
    CHECK(moved == want);                                                                // nothing but the chunks' bytes
    // ... and all at once
    Staged A(ctot);
    A.apply(run_copies(c_off.data(), c_len.data(), soff.data(), ids.data(), m));
    for (int k = 0; k < m; k++) A.holds(soff[ids[k]], c_off[ids[k]], c_len[ids[k]]);
}

static void check_range_staging(const std::vector<long> &c_off, const std::vector<long> &c_len, int piece_chunks, int expect_one_range /* -1: either */)
{
    const int n = (int)c_off.size();
    RangeStaging S(c_off.data(), c_len.data(), n);
    long lo = c_off[0], hi = c_off[0] + c_len[0];
    ull sum = 0;
    bool ascending = true;
    for (int i = 0; i < n; i++) {
        lo = std::min(lo, c_off[i]); hi = std::max(hi, c_off[i] + c_len[i]); sum += c_len[i];
        if (i && c_off[i] < c_off[i - 1] + c_len[i - 1]) ascending = false;
    }
    CHECK(S.one_range == ((ull)(hi - lo) <= sum + sum / 4 + 4096));                      // a quarter of padding and 4096 bytes
    if (expect_one_range >= 0) CHECK(S.one_range == (expect_one_range != 0));
    CHECK(S.piecewise() == (!S.one_range || ascending));                                 // a range out of order is one piece
    S.pb = {0};
    if (S.piecewise()) for (int i = piece_chunks; i < n; i += piece_chunks) S.pb.push_back(i);
    S.pb.push_back(n);
    ull end = 0;
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < i; j++) CHECK(S.coff[i] >= S.coff[j] + c_len[j] || S.coff[j] >= S.coff[i] + c_len[i]);
        if (S.one_range) CHECK(S.coff[i] - S.coff[0] == c_off[i] - c_off[0]);            // the range as it is
        else CHECK(S.coff[i] % 16 == 0);
        end = std::max<ull>(end, S.coff[i] + c_len[i]);
    }
    // (behind the last chunk: 16 bytes of a range; a chunk staged alone has 8 behind it, as it had before the rules moved here)
    CHECK(S.ctot >= end + (S.one_range ? 16 : 8));
    Staged G(S.ctot);
    for (size_t k = 0; k + 1 < S.pb.size(); k++) {
        const std::vector<StageCopy> cp = S.copies((int)k);
        if (S.one_range) CHECK(cp.size() <= 1);                                          // a piece of a range is one copy
        else { size_t nz = 0; for (int i = S.pb[k]; i < S.pb[k + 1]; i++) nz += c_len[i] != 0; CHECK(cp.size() == nz); }
        G.apply(cp);
    }
    for (int i = 0; i < n; i++) G.holds(S.coff[i], c_off[i], c_len[i]);
}

static void check_codec_plans()
{
    const ull edge[] = {0, 1, 2, 3, SEG - 1, SEG + 1, HALO - 1, HALO + 1, TILE - 1, TILE, TILE + 1, 2ull * TILE + 1};
    std::mt19937 rng(77);
    // compress: every edge size alone and in pairs; 2^31 - 1 accepted, 2^31 refused; 300 chunks of mixed sizes
    for (int level : {1, 6}) for (int stream = 0; stream < 2; stream++) {
        for (ull a : edge) {
            g_case = "compress one chunk of " + std::to_string(a) + " level " + std::to_string(level) + " stream " + std::to_string(stream);
            check_compress({a}, 1, stream, level);
            for (ull b : edge) { g_case += " +" + std::to_string(b); check_compress({a, b}, 1, stream, level); }
        }
        g_case = "compress rows of 6 bytes, level " + std::to_string(level);
        check_compress({0, 1, 171, (ull)TILE / 6, (ull)TILE / 6 + 1}, 6, false, level);
        g_case = "compress 2^31 - 1 bytes, level " + std::to_string(level);
        check_compress({TWO31 - 1}, 1, stream, level);
        check_compress({3, TWO31 - 1}, 1, stream, level);
        g_case = "compress 2^31 bytes";
        check_compress({TWO31}, 1, stream, level);
        check_compress({5, TWO31 / 2}, 2, false, level);
        std::vector<ull> many(300);
        for (ull &v : many) v = rng() % 4 == 0 ? edge[rng() % 8] : rng() % 5000;
        g_case = "compress 300 chunks";
        check_compress(many, 1, stream, level);
    }
    {   // an output slot that is not 16-byte aligned is refused, and named
        g_case = "compress slot alignment";
        const long bounds[3] = {0, 10, 20}, slots[2] = {0, 24};
        const CompressPlan P(bounds, 2, 1, false, slots, 6, DIMS);
        CHECK(strstr(P.error, "slot 1"));
    }
    // inflate
    for (int nc_full : {0, 9}) {
        for (ull a : edge) for (ull b : {0ull, 1ull, 7ull}) {
            g_case = "inflate rows " + std::to_string(a) + ", " + std::to_string(b) + " nc_full " + std::to_string(nc_full);
            check_inflate({a, b}, 1, 1, nc_full ? 3 : 0);
            check_inflate({a}, 3, 2, nc_full);
        }
        std::vector<ull> many(300);
        for (ull &v : many) v = rng() % 700;
        g_case = "inflate 300 chunks nc_full " + std::to_string(nc_full);
        check_inflate(many, 5, 2, nc_full);
        g_case = "inflate 2^31";
        check_inflate({TWO31 - 1}, 1, 1, 0);
        check_inflate({1, TWO31 / 4}, 2, 2, 0);
    }
    // inflate scratch: chunk counts around the segment rule's 128; sizes either side of a whole number of groups (n + 2 a multiple of 64), of
    // GS_TILE groups (a chunk's tile count, the grid of the group sums); compressed lengths around a candidate slot's 4096 bytes; both overrides
    {
        const ull sizes[] = {0, 1, 61, 62, 63, 126, 127, 16189, 16190, 16191, 16192, 16381, 16382, 16383, 16384}, clens[] = {0, 1, 4095, 4096, 4097};
        const int NS = sizeof sizes / sizeof sizes[0], NL = sizeof clens / sizeof clens[0];
        for (int nc : {1, 2, 3, 5, 127, 128, 129, 300}) for (int segs : {0, 1, 4, 40}) for (long rounds : {-1l, 0l, 3l, (1l << 26) + 5}) {
            const std::string base = "inflate scratch chunks " + std::to_string(nc) + " segs " + std::to_string(segs) + " rounds " + std::to_string(rounds);
            std::vector<ull> n(nc), cl(nc);
            for (int a = 0; a < NS; a++) for (int b = 0; b < NL; b++) {
                g_case = base + " mixed from size " + std::to_string(sizes[a]) + " c_len " + std::to_string(clens[b]);
                for (int i = 0; i < nc; i++) { n[i] = sizes[(a + i) % NS]; cl[i] = clens[(b + 3 * i) % NL]; }
                check_inflate_scratch(n, cl, segs, rounds);
                g_case = base + " all of size " + std::to_string(sizes[a]) + " c_len " + std::to_string(clens[b]);
                check_inflate_scratch(std::vector<ull>(nc, sizes[a]), std::vector<ull>(nc, clens[b]), segs, rounds);
                n_scratch += 2;
            }
        }
    }
    // the sub-batch cut
    for (int t = 0; t < 400; t++) {
        const int n = t < 3 ? t : 1 + (int)(rng() % 40);
        const size_t budget = t % 3 == 0 ? 1 : 1000 + rng() % 5000;
        std::vector<size_t> bytes(n);
        for (size_t &v : bytes) { const unsigned r = rng() % 10; v = r == 0 ? 0 : r == 1 ? budget + 1 + rng() % 100 : r == 2 ? budget : rng() % 2000; }
        for (int max_chunks : {1, 3, 32768}) {
            g_case = "cut_batches case " + std::to_string(t) + " budget " + std::to_string(budget) + " max_chunks " + std::to_string(max_chunks);
            check_cut(bytes, budget, max_chunks);
        }
    }
    g_case = "cut_batches zeros";
    check_cut(std::vector<size_t>(50, 0), 1, 7);
    // the phase width
    for (ull budget : {1ull, 1ull << 20, 100ull << 20, 8ull << 30}) for (int n_chunks : {1, 7, 300, 32768}) for (ull K : {14ull, 26ull, 51ull})
        for (u32 max_n : {0u, 1u, 255u, 256u, 257u, 5000u, 8192u, 8200u, 16384u, 1u << 20, (1u << 20) + 2048u, 23100000u, (u32)(TWO31 - 1)}) {
            g_case = "phase_width budget " + std::to_string(budget) + " chunks " + std::to_string(n_chunks) + " K " + std::to_string(K) + " max_n " + std::to_string(max_n);
            check_phase_width(budget, n_chunks, K, max_n);
        }
    // staging.  Tables of 1 .. 9 chunks: ascending back to back (a .cbin), two runs with a gap, every chunk apart, descending
    for (int t = 0; t < 200; t++) {
        const int n = 1 + t % 9, shape = t / 9 % 4;
        std::vector<long> len(n), off(n);
        for (long &v : len) v = 1 + rng() % 60;
        long at = rng() % 30;
        for (int i = 0; i < n; i++) {
            if (shape == 1 && i == n / 2) at += 1 + rng() % 40;
            if (shape == 2) at += 1 + rng() % 40;
            off[i] = at; at += len[i];
        }
        if (shape == 3) { std::reverse(off.begin(), off.end()); std::reverse(len.begin(), len.end()); }
        std::vector<int> all(n), some;
        for (int i = 0; i < n; i++) { all[i] = i; if (rng() % 3) some.push_back(i); }
        for (int piece_chunks : {1, 2, 100}) {
            g_case = "run staging table " + std::to_string(t) + " shape " + std::to_string(shape) + " piece of " + std::to_string(piece_chunks);
            check_run_staging(off, len, all, piece_chunks, shape == 0 && piece_chunks == 100);
            g_case += " some resident";
            check_run_staging(off, len, some, piece_chunks, false);
            g_case = "range staging table " + std::to_string(t) + " shape " + std::to_string(shape) + " piece of " + std::to_string(piece_chunks);
            check_range_staging(off, len, piece_chunks, shape == 0 || shape == 3 ? 1 : -1);
            std::vector<long> len0 = len;                          // zero-length chunks (this caller allows them)
            len0[rng() % n] = 0;
            g_case += " with an empty chunk";
            check_range_staging(off, len0, piece_chunks, -1);
        }
    }
    {   // keys 0, 1, 3, 4 of a range missing, key 2 resident: two runs, two copies
        g_case = "run staging two runs around a resident chunk";
        const std::vector<long> off = {0, 100, 200, 300, 400}, len(5, 100);
        check_run_staging(off, len, {0, 1, 3, 4}, 100, false);
        std::vector<long> soff(5);
        stage_runs(off.data(), len.data(), std::vector<int>{0, 1, 3, 4}.data(), 4, soff.data());
        CHECK(run_copies(off.data(), len.data(), soff.data(), std::vector<int>{0, 1, 3, 4}.data(), 4).size() == 2);
    }
    // the slack of a range: 10 chunks of 40000 bytes, the padding between them just under and just over a quarter (+ 4096 bytes)
    for (int over = 0; over < 2; over++) {
        const long L = 40000, sum = 10 * L, span = sum + sum / 4 + 4096 + over, pad = span - sum;
        std::vector<long> off(10), len(10, L);
        for (int i = 0; i < 10; i++) off[i] = 7 + i * L + (i ? pad / 9 * i + (i == 9 ? pad % 9 : 0) : 0);
        g_case = "range staging slack, over " + std::to_string(over);
        check_range_staging(off, len, 3, !over);
    }
}

int main()
{
    long n_cases = 0;
    for (int t = 0; t < 16; t++) {
        std::mt19937 rng(1000 + t);
        auto pick = [&](long lo, long hi) { return lo + (long)(rng() % (unsigned long)(hi - lo + 1)); };
        Table T;
        T.n = 1 + t % 8;
        const uint64_t rbs[] = {2, 6, 770};
        T.row_bytes = rbs[t % 3];
        long row = pick(0, 20);
        long max_rows = 0, total = 0;
        for (int i = 0; i < T.n; i++) {
            T.rows.push_back(pick(1, 40)); T.row0.push_back(row); row += T.rows[i]; T.c_len.push_back(pick(1, 50));
            max_rows = std::max(max_rows, T.rows[i]); total += T.rows[i];
        }
        const size_t pieces[] = {0, (size_t)T.row_bytes, (size_t)(max_rows * T.row_bytes), (size_t)(3 * max_rows * T.row_bytes), (size_t)((total + 1) * T.row_bytes)};
        std::vector<unsigned> masks;
        if (T.n <= 6) for (unsigned m = 0; m < (1u << T.n); m++) masks.push_back(m);
        else { masks = {0u, (1u << T.n) - 1}; for (int k = 0; k < 10; k++) masks.push_back((unsigned)rng() & ((1u << T.n) - 1)); }
        for (int gaps = 0; gaps < 2; gaps++) {
            T.c_off.clear();
            long off = pick(0, 9);
            for (int i = 0; i < T.n; i++) { T.c_off.push_back(off); off += T.c_len[i] + (gaps && pick(0, 2) ? pick(1, 40) : 0); }
            for (unsigned mask : masks) for (int on_device = 0; on_device < 2; on_device++) {
                g_case = "table seed " + std::to_string(1000 + t) + " chunks " + std::to_string(T.n) + " row_bytes " + std::to_string(T.row_bytes) +
                         " gaps " + std::to_string(gaps) + " resident mask " + std::to_string(mask) + " on_device " + std::to_string(on_device);
                const FeedPlan F = make_feed(T, mask, on_device);
                check_layout(T, F);
                const std::string base = g_case;
                for (size_t piece : pieces) {
                    // the range leaves a few rows of the first and last chunk out (every chunk of a tile call holds a row of it)
                    const long a = pick(0, T.rows[0] - 1), z = T.n > 1 ? pick(0, T.rows[T.n - 1] - 1) : 0;
                    g_case = base + " piece " + std::to_string(piece) + " range -" + std::to_string(a) + " -" + std::to_string(z);
                    const std::string with_piece = g_case;
                    for (long window_rows : {1l, 7l, 1000l}) for (long tile_rows : {4l, 512l}) {
                        g_case = with_piece + " tiles window_rows " + std::to_string(window_rows) + " tile_rows " + std::to_string(tile_rows);
                        check_tiles(T, F, piece, std::min(T.begin() + a, T.end() - 1), std::max(T.end() - z, T.begin() + a + 1), window_rows, tile_rows);
                    }
                    g_case = with_piece;
                    check_halo_ops(T, F, piece, a, z);
                    n_cases++;
                }
            }
        }
        // a missing chunk without compressed bytes is reported, the first of them
        if (T.n >= 2) {
            g_case = "table seed " + std::to_string(1000 + t) + " no bytes";
            T.c_len[T.n - 1] = 0; T.c_len[T.n - 2] = 0;
            FeedPlan F(T.c_off.data(), T.c_len.data(), T.row0.data(), T.rows.data(), T.n, T.row_bytes, false);
            CHECK(F.layout() == T.n - 2);
            F.resident[T.n - 2] = 1;
            FeedPlan G = F;
            G.ctot = 0;
            CHECK(G.layout() == T.n - 1);
        }
    }
    check_codec_plans();
    printf("plan_check: %ld tables x pieces and the codec's plans (%ld inflate scratch layouts) passed\n", n_cases, n_scratch);
    return 0;
}
