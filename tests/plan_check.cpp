// A seeded sweep over the plans of the device reductions (mtscomp_amd/csrc/reduce_plan.h: no HIP in it), built with the address and
// undefined-behaviour sanitizers by `make -C mtscomp_amd/csrc plan_check` and run by tests/test_feed_plan.py.  Small chunk tables, every
// residency mask, compressed bytes with and without gaps, five piece sizes; the staging layout, the tile family's plan and, through a
// stand-in for each op's map from units to rows, the halo family's.  Exits 1 with the case printed at the first property that fails.
#include <stdio.h>
#include <stdlib.h>

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
    printf("plan_check: %ld tables x pieces passed\n", n_cases);
    return 0;
}
