// The host side of the device reductions (window_stats, rank_hist, decimate, project, detect, waveforms, mean_waveforms, waveform_features, localize, correlate, match_templates, residual, filtered_rank_hist, filtered_gram, welch, gram) and their C entries.
// The plans -- what goes into which piece, and where -- are in reduce_plan.h and know no device; this file allocates, copies,
// decodes and launches around them.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <future>
#include <mutex>
#include <optional>
#include <vector>

#include "engine.h"
#include "reduce_plan.h"

using namespace mts;

// ================================================================================================
// How a reduction is fed
// ================================================================================================
// A reduction reads the rows of some chunks and never keeps them.  A chunk that is whole in the call's device cache (resident) is read
// where it lies; every other chunk (missing) comes with its compressed bytes and is decoded into the piece workspace E.h_out.  The
// missing chunks are cut into pieces of MTS_PIPE_BYTES of decoded bytes (FeedPlan::piece_bounds; resident chunks weigh nothing, device
// input is one piece: nothing to copy beside the kernels, and smaller batches inflate slower): while piece p is decoded and reduced,
// the compressed bytes of piece p + 1 cross the bus on a helper thread.  Two families share this code:
//   tiles (window_stats, rank_hist): a chunk's rows are cut into tiles that are reduced on their own, so the resident chunks go first
//        and each piece decodes exactly its own missing chunks (TilePlan, TileFeed);
//   halo (decimate, project, detect, waveforms, mean_waveforms, waveform_features, localize, correlate, match_templates, residual, filtered_rank_hist, filtered_gram, welch, gram): a unit of output (outputs, rows,
//        events, blocks, groups -- the op gives HaloPlan its map from units to rows) reads rows of several adjacent chunks, so a piece
//        reads chunks [c0, c1] through a table of segment bases and first rows, and decodes the missing ones among them -- a boundary
//        chunk in both pieces (HaloPlan, HaloFeed).  Ten of them (detect, waveforms, mean_waveforms, waveform_features, localize, correlate, match_templates, residual, filtered_rank_hist, filtered_gram) start from
//        one filtered signal z: their checks, uploads, filter stage and tails are the z family's shared parts below.
// What every caller keeps to, and TileFeed, HaloFeed, feed_pieces and ChunkFeed hold up:
//   - An allocation that fails empties this device's caches before it tries again (DBuf::ensure -> drop_device_caches: hipFree,
//     which waits for the kernels already launched -- earlier reads are done).  So every allocation of the call (the op's own DBuf,
//     then ChunkFeed::ensure) comes BEFORE the first use of a resident entry's address, and ensure looks every resident entry up
//     again: a call whose entries went ends with MTS_E_MISS (the Reader sends every chunk's bytes once more).  HaloFeed::place and
//     TileFeed::place are the two places that read those addresses, each right after its ChunkFeed::ensure.
//   - A decode allocates again (decompress_batch).  The tile family therefore reduces the resident tiles and waits for the stream
//     before the first decode (only when there are resident tiles); the halo family checks after each piece's decode and before its
//     launch that every resident chunk the piece reads is still in the cache at the address its table holds (HaloFeed::run, the
//     only way to a piece's table).
//   - The helper thread's copy of piece p + 1 starts before piece p's decode and is always joined before feed_pieces returns, on
//     error paths too: it holds references to the caller's frame (run_pieces, engine.h).
//   - The first dev_decompress of a call starts the stage times (add_times false), every later one adds to them.
//   - The compressed bytes of the missing chunks lie in E.h_in in chunk order, at mcoff[] (FeedPlan::layout: the run-joined rule of
//     codec_plan.h, which the decoded-chunk cache stages by as well).
namespace {

// the chunks of a call as every entry point receives them.  bad: a pointer the table needs is null -- the entry's own check,
// which answers after a cache that does not exist and before everything else
struct ChunkTable {
    DevCache *cache;
    const long *keys;
    const u8 *cdata;
    bool on_device;
    const long *c_off, *c_len, *row0, *n_rows;
    int n_chunks, nc, sz, flags;
    bool bad;
};

// (the arguments in the order of the host entries of include/mtscomp_hip.h; reduce_entry fills in the cache)
ChunkTable host_table(long cache_id, int n_chunks, const long *keys, const long *row0, const u8 *cdata, const long *c_off, const long *c_len,
                      const long *n_rows, int nc, int sz, int flags, const int *status)
{
    const bool bad = n_chunks > 0 && (!row0 || !c_off || !c_len || !n_rows || !status || (cache_id && !keys));
    return {nullptr, keys, cdata, false, c_off, c_len, row0, n_rows, n_chunks, nc, sz, flags, bad};
}

// (the arguments in the order of the device entries)
ChunkTable dev_table(const u8 *d_cdata, const long *c_off, const long *c_len, const long *row0, const long *n_rows, int n_chunks, int nc, int sz,
                     int flags, const int *status)
{
    const bool bad = n_chunks > 0 && (!d_cdata || !row0 || !c_off || !c_len || !n_rows || !status);
    return {nullptr, nullptr, d_cdata, true, c_off, c_len, row0, n_rows, n_chunks, nc, sz, flags, bad};
}

// ---- the entries of the reductions: the cache (host entries; the device entries have none, cache_id 0), the engine and its lock,
// the device, then run(engine, table)
template <class Run>
int reduce_entry(int device, long cache_id, ChunkTable T, Run &&run)
{
    if (cache_id) {
        int cdev = 0;
        T.cache = find_cache(cache_id, &cdev);
        if (!T.cache || cdev != device) { set_error("cache %ld does not exist on device %d", cache_id, device); return MTS_E_ARG; }
    }
    if (T.bad) return MTS_E_ARG;
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(E->mu);
    if (T.cache && !cache_alive(cache_id, T.cache)) return MTS_E_ARG;      // (destroyed while this call waited for the engine)
    MTS_HIP(hipSetDevice(E->dev));
    if ((rc = check_items(T.sz, T.flags))) return rc;          // (the first check of every op)
    return run(*E, T);
}

// ---- the checks the ops share, in the order every op makes them: check_items (reduce_entry), the op's own, check_columns,
// check_chunk_table, check_cover, status_ok
int check_columns(const int *cols, int n_cols, int nc)
{
    for (int j = 0; j < n_cols; j++)
        if (cols[j] < 0 || cols[j] >= nc) { set_error("column %d out of range (%d channels)", cols[j], nc); return MTS_E_ARG; }
    return MTS_OK;
}

// adjacent: every chunk begins where the one before it ends (the halo family); else the chunks are in order, do not overlap and each
// holds a row of [row_begin, row_end) (the tile family)
int check_chunk_table(bool adjacent, const ChunkTable &T, long row_begin = 0, long row_end = 0)
{
    const long *c_len = T.c_len, *row0 = T.row0, *n_rows = T.n_rows;
    for (int i = 0; i < T.n_chunks; i++) {
        if (n_rows[i] <= 0 || row0[i] < 0 || c_len[i] < 0) { set_error("chunk %d: rows or bytes invalid", i); return MTS_E_ARG; }
        if (adjacent) {
            if (i && row0[i] != row0[i - 1] + n_rows[i - 1]) { set_error("chunk %d: chunks must be adjacent", i); return MTS_E_ARG; }
        } else {
            if (i && row0[i] < row0[i - 1] + n_rows[i - 1]) { set_error("chunk %d: rows out of order or overlapping", i); return MTS_E_ARG; }
            if (row0[i] >= row_end || row0[i] + n_rows[i] <= row_begin) { set_error("chunk %d holds no row of [%ld, %ld)", i, row_begin, row_end); return MTS_E_ARG; }
        }
        if (!T.cache && c_len[i] == 0) { set_error("chunk %d: no compressed bytes and no cache", i); return MTS_E_ARG; }
        if (c_len[i] && (u64)n_rows[i] * T.nc * T.sz >= (1ull << 31)) { set_error("chunk %d: chunks must be < 2 GiB", i); return MTS_E_ARG; }
    }
    return MTS_OK;
}

// the FIR taps of decimate and the z family
int check_taps(const char *op, int n_taps, const double *taps)
{
    if (n_taps < 1 || n_taps > MTS_DECIMATE_MAX_TAPS || !taps) { set_error("%s: %d taps (1 .. %d)", op, n_taps, MTS_DECIMATE_MAX_TAPS); return MTS_E_ARG; }
    for (int j = 0; j < n_taps; j++)
        if (!std::isfinite(taps[j])) { set_error("%s: tap %d is not finite", op, j); return MTS_E_ARG; }
    return MTS_OK;
}

// what the z family (detect, waveforms, mean_waveforms, waveform_features, localize, correlate, match_templates, residual, filtered_rank_hist, filtered_gram) filters: z[t, j] = sum_k taps[k] * x[t + half - k, cols[j]]
// in float32, x = 0 outside [vb, ve), minus the row's median over the columns with reference 1.  `op` names the entry in every message.
struct ZArgs { const char *op; long vb, ve; int n_taps; const double *taps; int n_cols; const int *cols; int reference; };

// the first checks of the z family.  max_cols 0: as many columns as a grid holds, in one message with the table (detect, waveforms, mean_waveforms);
// else that many, the count named (the template ops)
int check_zargs(const ChunkTable &T, const ZArgs &Z, int max_cols = 0)
{
    const bool bad_table = T.nc <= 0 || T.n_chunks < 0, bad_cols = Z.n_cols < 1 || Z.n_cols > (max_cols ? max_cols : 64 * 65535) || !Z.cols;
    if (!max_cols && (bad_table || bad_cols)) { set_error("%s: n_channels, n_chunks or columns invalid", Z.op); return MTS_E_ARG; }
    if (bad_table) { set_error("%s: n_channels or n_chunks invalid", Z.op); return MTS_E_ARG; }
    if (bad_cols) { set_error("%s: %d columns (1 .. %d)", Z.op, Z.n_cols, max_cols); return MTS_E_ARG; }
    if (const int rc = check_taps(Z.op, Z.n_taps, Z.taps)) return rc;
    if (Z.reference < 0 || Z.reference > 1) { set_error("%s: reference %d (0 none, 1 median)", Z.op, Z.reference); return MTS_E_ARG; }
    if (Z.reference && Z.n_cols > MTS_DETECT_MAX_REF_COLS) {
        set_error("%s: a median reference over %d columns (<= %d)", Z.op, Z.n_cols, MTS_DETECT_MAX_REF_COLS); return MTS_E_ARG;
    }
    if (Z.vb < 0 || Z.ve < Z.vb || Z.ve > (1l << 60)) { set_error("%s: rows invalid", Z.op); return MTS_E_ARG; }
    return MTS_OK;
}

// the templates (n_out, n_tau, n_cols) of correlate, match_templates and residual, row `before` of each laid on the event's row
int check_templates(const char *op, int n_cols, int before, int n_tau, int n_out, const float *templates)
{
    if (n_tau < 1 || n_tau > MTS_CORRELATE_MAX_T) { set_error("%s: templates of %d rows (1 .. %d)", op, n_tau, MTS_CORRELATE_MAX_T); return MTS_E_ARG; }
    if (before < 0 || before > n_tau) { set_error("%s: before %d (0 .. %d)", op, before, n_tau); return MTS_E_ARG; }
    if (n_out < 1 || n_out > MTS_CORRELATE_MAX_OUT || !templates) { set_error("%s: %d templates (1 .. %d)", op, n_out, MTS_CORRELATE_MAX_OUT); return MTS_E_ARG; }
    const long per = (long)n_tau * n_cols;
    for (long e = 0; e < (long)n_out * per; e++)
        if (!std::isfinite(templates[e])) { set_error("%s: template entry (%ld, %ld, %ld) is not finite", op, e / per, e % per / n_cols, e % n_cols); return MTS_E_ARG; }
    return MTS_OK;
}

// a slab bound from the environment (MTS_<OP>_SLAB_BYTES: tests and tools set them); anything but a positive number is the default
u64 env_bytes(const char *name, u64 otherwise)
{
    const char *e = getenv(name);
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (u64)v : otherwise;
}

// the (adjacent) chunks hold the rows [lo, hi) that the op reads; nothing to hold when the range is empty
int check_cover(const char *op, const ChunkTable &T, long lo, long hi)
{
    if (lo < hi && (T.n_chunks == 0 || T.row0[0] > lo || T.row0[T.n_chunks - 1] + T.n_rows[T.n_chunks - 1] < hi)) {
        set_error("%s: the chunks do not cover rows [%ld, %ld)", op, lo, hi); return MTS_E_ARG;
    }
    return MTS_OK;
}

// (a chunk that is not decoded -- resident, or read by no unit -- is good)
void status_ok(const ChunkTable &T, int *status)
{
    for (int i = 0; i < T.n_chunks; i++) status[i] = MTS_CHUNK_OK;
}

// which chunks of a call are resident, where the bytes of the others lie (FeedPlan), and their way into E.h_out
struct ChunkFeed : FeedPlan {
    DevCache *cache;
    const long *keys;
    const u8 *cdata;
    int nc, sz;
    int dflags;                                               // (the decoder compares the transform flags as a whole)
    std::vector<char> copied;
    std::vector<uintptr_t> res_base;                          // the address of each resident entry that the tables and tiles hold
    bool first_decode = true;

    explicit ChunkFeed(const ChunkTable &T)
        : FeedPlan(T.c_off, T.c_len, T.row0, T.n_rows, T.n_chunks, (u64)T.nc * T.sz, T.on_device), cache(T.cache), keys(T.keys), cdata(T.cdata),
          nc(T.nc), sz(T.sz), dflags(T.flags & ~MTS_FLAG_UNSIGNED), copied(T.n_chunks, 0), res_base(T.n_chunks, 0) {}

    const CacheEntry *entry_of(int i) const                   // chunk i whole in the cache, or nullptr
    {
        if (!cache) return nullptr;
        auto it = cache->map.find(keys[i]);
        if (it == cache->map.end()) return nullptr;
        const CacheEntry &e = it->second;
        return e.rows == n_rows[i] && e.cols == nc && e.size == chunk_bytes(i) ? &e : nullptr;
    }
    long key_of(int i) const { return keys ? keys[i] : (long)i; }
    const u8 *src(Engine &E) const { return on_device ? cdata : E.h_in.as<u8>(); }

    // resident or missing (a missing chunk without bytes: MTS_E_MISS), and the layout of the missing chunks' bytes in E.h_in
    int classify()
    {
        for (int i = 0; i < n_chunks; i++) resident[i] = entry_of(i) != nullptr;
        const int i = layout();
        if (i >= 0) { set_error("chunk key %ld is not resident and no compressed bytes were given", key_of(i)); return MTS_E_MISS; }
        return MTS_OK;
    }

    // the last allocations of the call (after the op's own), then the resident entries once more: their addresses hold from here
    // to the next decode
    int ensure(Engine &E, u64 piece_cap)
    {
        int rc;
        if (any_miss && !on_device && (rc = E.h_in.ensure(ctot + 256))) return rc;
        if (piece_cap && (rc = E.h_out.ensure(piece_cap + 256))) return rc;
        for (int i = 0; i < n_chunks; i++) {
            if (!resident[i]) continue;
            const CacheEntry *e = entry_of(i);
            if (!e) { set_error("chunk key %ld was dropped from the cache during the call", key_of(i)); return MTS_E_MISS; }
            res_base[i] = (uintptr_t)e->d;
        }
        return MTS_OK;
    }

    // the compressed bytes of `chunks` (ascending, missing) into E.h_in, each chunk once in a call; runs on the helper thread
    int copy_in(Engine &E, const std::vector<int> &chunks)
    {
        if (on_device) return MTS_OK;
        MTS_HIP(hipSetDevice(E.dev));
        for (const StageCopy &c : run_copies(c_off, c_len, mcoff.data(), chunks.data(), (int)chunks.size(), copied.data()))
            if (const int rc = staged_h2d(E, E.h_in.as<u8>() + c.dst, cdata + c.src, (size_t)c.len)) return rc;
        return MTS_OK;
    }

    // a piece's missing chunks into E.h_out; status[] of each of them
    int decode(Engine &E, hipStream_t st, const FeedPiece &P, int *status)
    {
        const int nm = (int)P.miss.size();
        if (!nm) return MTS_OK;
        std::vector<long> co(nm), cl(nm), nr(nm);
        std::vector<int> mst(nm, MTS_CHUNK_CORRUPT);
        for (int z = 0; z < nm; z++) { co[z] = mcoff[P.miss[z]]; cl[z] = c_len[P.miss[z]]; nr[z] = n_rows[P.miss[z]]; }
        const int rc = dev_decompress(E, st, src(E), co.data(), cl.data(), nr.data(), nm, nc, sz, dflags, E.h_out.as<u8>(), P.ooff.data(), mst.data(),
                                      0, !first_decode);
        first_decode = false;
        if (!rc) for (int z = 0; z < nm; z++) status[P.miss[z]] = mst[z];
        return rc;
    }

    // after a piece's decode: every resident chunk its table points at is still in the cache at that address
    int still_placed(const FeedPiece &P) const
    {
        for (int i = P.c0; i <= P.c1; i++) {
            if (!resident[i]) continue;
            const CacheEntry *e = entry_of(i);
            if (!e || (uintptr_t)e->d != res_base[i]) { set_error("chunk key %ld was dropped from the cache during the call", key_of(i)); return MTS_E_MISS; }
        }
        return MTS_OK;
    }
};

// piece after piece: the next piece's bytes are copied beside this piece's decode and launch(p)
template <class Launch>
int feed_pieces(ChunkFeed &F, Engine &E, hipStream_t st, const std::vector<FeedPiece> &pieces, int *status, Launch &&launch)
{
    return run_pieces((int)pieces.size(), [&](int p) -> int { return F.copy_in(E, pieces[p].miss); },
                      [&](int p) -> int { const int rc = F.decode(E, st, pieces[p], status); return rc ? rc : launch(p); });
}

// ---- halo family: the device side of a HaloPlan, in three steps with the op's own regions, uploads and kernel between them:
//   plan(the op's map) -> the op takes its regions from L, table_bytes() for the tables ->  place()  -> the op's uploads ->  run(launch).
// place() allocates in the order that keeps the resident entries' addresses good, and run() is the only way to a piece's table.
struct PieceSegs { const u8 *const *base; const long *row0; int ns; };   // a piece's table on the device: ns bases, ns + 1 first rows

struct HaloFeed {
    ChunkFeed F;
    WsLayout L;
    std::optional<HaloPlan> P;
    std::vector<long> seg;                                    // (the source of an asynchronous copy: it lives as long as the call)
    const long *d_seg = nullptr;

    HaloFeed(const ChunkTable &T, bool out_on_host) : F(T), L{out_on_host} {}

    // sorts the chunks and cuts the units into pieces (first, rows: see HaloPlan)
    template <class First, class Rows>
    int plan(long n_units, First &&first, Rows &&rows)
    {
        const int rc = F.classify();
        if (!rc) P.emplace(F, pipe_piece_bytes(), n_units, first, rows);
        return rc;
    }
    u64 table_bytes() const { return 8 * (u64)(P->seg_at.back() + 1); }

    // the op's own workspace `own` (laid out in L, the tables at o_table), then the feed's allocations, then the tables: they hold
    // the resident entries' addresses
    int place(Engine &E, hipStream_t st, DBuf &own, size_t o_table)
    {
        int rc;
        if ((rc = own.ensure(L.end + 256))) return rc;
        if ((rc = F.ensure(E, P->piece_cap))) return rc;
        seg = P->tables(F, F.res_base.data(), (uintptr_t)E.h_out.p);
        d_seg = (const long *)(own.as<u8>() + o_table);
        MTS_HIP(hipMemcpyAsync((void *)d_seg, seg.data(), 8 * seg.size(), hipMemcpyHostToDevice, st));
        return MTS_OK;
    }

    // piece after piece: launch(piece, its table), once the piece is decoded and its resident chunks are known to be where the
    // table says
    template <class Launch>
    int run(Engine &E, hipStream_t st, int *status, Launch &&launch)
    {
        return feed_pieces(F, E, st, P->pieces, status, [&](int p) {
            const FeedPiece &Q = P->pieces[p];
            const int rc = F.still_placed(Q);
            if (rc) return rc;
            const long *sb = d_seg + P->seg_at[p];
            const int ns = std::max(0, Q.c1 - Q.c0 + 1);
            return launch(Q, PieceSegs{(const u8 *const *)sb, sb + ns, ns});
        });
    }
};

// ---- z family: what detect, waveforms, mean_waveforms, waveform_features, localize, correlate, match_templates, residual, filtered_rank_hist and filtered_gram share around their own slab loops.  Each run reads
// top to bottom as the halo family's sequence: plan -> regions (ZStage first, the op's, EventTail's) -> StreamGuard -> place ->
// uploads -> run -> tail.
//
// The rule for leaving early, for all of them: from the first asynchronous upload out of host memory that the call owns (HaloFeed::seg,
// ZStage::h_taps, the repacked templates, SubEvents::namp, the parts of mean_waveforms, the basis image of waveform_features) no path returns before the stream has been waited for -- a failed
// H.run, a failed MTS_HIP.  The guard is declared after those vectors and before H.place, so it goes before they do; the tails'
// own wait() disarms it, so the normal path waits no more often than it has to.
struct StreamGuard {
    hipStream_t st;
    bool waited = false;
    ~StreamGuard() { if (!waited) (void)hipStreamSynchronize(st); }
    int wait() { MTS_HIP(hipStreamSynchronize(st)); waited = true; return MTS_OK; }
};

// the filter stage: the taps (rounded once to float32) and the columns on the device, and z of the rows [a, b) into a float32 slab --
// the same launches with the same arguments in every op, so the same bytes
struct ZStage {
    const ZArgs &Z;
    const long half;
    const size_t o_taps, o_cols;
    std::vector<float> h_taps;                                // (the source of an asynchronous copy: it lives as long as the call)
    const void *d_taps = nullptr;
    const int *d_cols = nullptr;

    // (the first two regions of the op's workspace)
    ZStage(const ZArgs &Z_, WsLayout &L) : Z(Z_), half((Z_.n_taps - 1) / 2), o_taps(L.take(4 * (u64)Z_.n_taps)), o_cols(L.take(4 * (u64)Z_.n_cols)) {}

    // (after H.place: ws is the op's workspace)
    int upload(hipStream_t st, u8 *ws)
    {
        h_taps.resize((size_t)Z.n_taps);
        for (int j = 0; j < Z.n_taps; j++) h_taps[j] = (float)Z.taps[j];
        d_taps = ws + o_taps; d_cols = (const int *)(ws + o_cols);
        MTS_HIP(hipMemcpyAsync(ws + o_taps, h_taps.data(), 4 * (size_t)Z.n_taps, hipMemcpyHostToDevice, st));
        MTS_HIP(hipMemcpyAsync(ws + o_cols, Z.cols, 4 * (size_t)Z.n_cols, hipMemcpyHostToDevice, st));
        return MTS_OK;
    }

    // d_y[t - a] = z[t] for t in [a, b): output k = t of a decimation by 1 whose newest row is half + k (nothing valid to read,
    // ns == 0: every row is 0), then the median
    int filter(hipStream_t st, const ChunkTable &T, const PieceSegs &Sg, long a, long b, float *d_y) const
    {
        const int r = launch_decimate(st, T.sz, T.flags, 4, Sg.base, Sg.row0, Sg.ns, T.nc, d_cols, Z.n_cols, d_taps, Z.n_taps, 1, half, a, b,
                                      Sg.ns ? Z.vb : 0, Sg.ns ? Z.ve : 0, d_y);
        return !r && Z.reference ? launch_row_median(st, d_y, b - a, Z.n_cols) : r;
    }
};

// the events of detect and match_templates: their count on the device, carried from slab to slab and piece to piece, and the first
// max_events of them in three arrays of 8-, 4- and 4-byte items
struct EventTail {
    const size_t o_total;
    u64 *d_total = nullptr;

    explicit EventTail(WsLayout &L) : o_total(L.take(8)) {}
    int begin(hipStream_t st, u8 *ws) { d_total = (u64 *)(ws + o_total); MTS_HIP(hipMemsetAsync(d_total, 0, 8, st)); return MTS_OK; }
    int finish(StreamGuard &G, long max_events, bool out_on_host, long *n_events, void *out8, const void *d8, void *out4a, const void *d4a, void *out4b,
               const void *d4b)
    {
        u64 total = 0;
        MTS_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, G.st));
        if (const int rc = G.wait()) return rc;
        *n_events = (long)total;
        const size_t n_w = (size_t)std::min<u64>(total, (u64)max_events);
        if (out_on_host && n_w) {
            MTS_HIP(hipMemcpyAsync(out8, d8, 8 * n_w, hipMemcpyDeviceToHost, G.st));
            MTS_HIP(hipMemcpyAsync(out4a, d4a, 4 * n_w, hipMemcpyDeviceToHost, G.st));
            MTS_HIP(hipMemcpyAsync(out4b, d4b, 4 * n_w, hipMemcpyDeviceToHost, G.st));
            MTS_HIP(hipStreamSynchronize(G.st));
        }
        return MTS_OK;
    }
};

// the dense float32 result of correlate and residual
int dense_tail(StreamGuard &G, bool out_on_host, float *out, const float *d_out, u64 n_items)
{
    if (out_on_host) MTS_HIP(hipMemcpyAsync(out, d_out, 4 * n_items, hipMemcpyDeviceToHost, G.st));
    return G.wait();
}

// ---- tile family: what the two ops share between their checks and their outputs, in three steps with the op's own regions,
// uploads and kernel between them:  plan() -> the op takes its regions from L ->  place()  -> the op's uploads ->  run(launch).
// The workspace E.stats begins with the tile descriptors, the tiles' windows (with_tile_win), the launch order, the chunks' ok flags
// and the columns.
struct TileFeed {
    ChunkFeed F;
    WsLayout L;
    std::optional<TilePlan<StatTile>> P;
    long n_tiles = 0;
    bool with_tile_win = false;
    size_t o_tiles = 0, o_tw = 0, o_ids = 0, o_ok = 0, o_cols = 0;
    std::vector<int> ok;                                      // per chunk: its rows count (resident, or decoded and good)
    u8 *ws = nullptr;
    StatTile *d_tiles = nullptr;
    long *d_tw = nullptr;
    int *d_ids = nullptr, *d_ok = nullptr, *d_cols = nullptr;

    TileFeed(const ChunkTable &T, bool out_on_host) : F(T), L{out_on_host}, ok(T.n_chunks + 1, 0) {}

    // zeroes count[], sorts the chunks, cuts the tiles and takes the shared regions
    int plan(long row_begin, long row_end, long window_rows, long tile_rows, bool with_tile_win_, int n_cols, long *count)
    {
        const long n_win = (row_end - row_begin + window_rows - 1) / window_rows;
        for (long w = 0; w < n_win; w++) count[w] = 0;
        const int rc = F.classify();
        if (rc) return rc;
        P.emplace(F, pipe_piece_bytes(), row_begin, row_end, window_rows, tile_rows);
        n_tiles = (long)P->tiles.size();
        with_tile_win = with_tile_win_;
        o_tiles = L.take(sizeof(StatTile) * (n_tiles + 1));
        if (with_tile_win) o_tw = L.take(8 * (u64)(n_tiles + 1));
        o_ids = L.take(4 * (u64)(n_tiles + 1)); o_ok = L.take(4 * (u64)ok.size()); o_cols = L.take(4 * (u64)n_cols);
        return MTS_OK;
    }

    // the workspace, then the feed's allocations, then the tiles' bases (resident chunks are ok and their status is set) and the uploads
    int place(Engine &E, hipStream_t st, int n_cols, const int *cols, int *status)
    {
        int rc;
        if ((rc = E.stats.ensure(L.end + 256))) return rc;
        if ((rc = F.ensure(E, P->piece_cap))) return rc;
        ws = E.stats.as<u8>();
        d_tiles = (StatTile *)(ws + o_tiles); d_tw = (long *)(ws + o_tw);
        d_ids = (int *)(ws + o_ids); d_ok = (int *)(ws + o_ok); d_cols = (int *)(ws + o_cols);
        P->place(F, F.res_base.data(), (uintptr_t)E.h_out.p);
        for (int i = 0; i < F.n_chunks; i++) if (F.resident[i]) { ok[i] = 1; status[i] = MTS_CHUNK_OK; }
        // (pageable sources: hipMemcpyAsync has staged them when it returns; the vectors live to the end of the call anyway)
        if (n_tiles) MTS_HIP(hipMemcpyAsync(d_tiles, P->tiles.data(), sizeof(StatTile) * n_tiles, hipMemcpyHostToDevice, st));
        if (n_tiles && with_tile_win) MTS_HIP(hipMemcpyAsync(d_tw, P->tile_win.data(), 8 * (size_t)n_tiles, hipMemcpyHostToDevice, st));
        if (n_tiles) MTS_HIP(hipMemcpyAsync(d_ids, P->ids.data(), 4 * (size_t)n_tiles, hipMemcpyHostToDevice, st));
        MTS_HIP(hipMemcpyAsync(d_ok, ok.data(), 4 * ok.size(), hipMemcpyHostToDevice, st));
        MTS_HIP(hipMemcpyAsync(d_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
        return MTS_OK;
    }

    // launch(d_ids of the launch, n): the resident chunks' tiles first, then piece after piece
    template <class Launch>
    int run(Engine &E, hipStream_t st, int *status, Launch &&launch)
    {
        const std::vector<long> &l0 = P->launch0;
        int rc;
        // resident chunks: reduced and waited for before any decode
        if (l0[1] > 0) {
            if ((rc = launch(d_ids, l0[1]))) return rc;
            MTS_HIP(hipStreamSynchronize(st));
        }
        // the other chunks: after a piece's decode the kernel is told which of its chunks are good (tiles of the others are identities)
        return feed_pieces(F, E, st, P->pieces, status, [&](int p) -> int {
            for (int i : P->pieces[p].miss) ok[i] = status[i] == MTS_CHUNK_OK;
            const hipError_t e = hipMemcpyAsync(d_ok, ok.data(), 4 * ok.size(), hipMemcpyHostToDevice, st);
            if (e != hipSuccess) { set_error("hipMemcpyAsync: %s", hipGetErrorString(e)); return MTS_E_HIP; }
            return launch(d_ids + l0[1 + p], l0[2 + p] - l0[1 + p]);
        });
    }
};

// the checks of the windows that the two tile ops begin with
int check_windows(const char *op, const ChunkTable &T, long row_begin, long row_end, long window_rows, int n_cols, const int *cols)
{
    if (T.nc <= 0 || T.n_chunks < 0 || n_cols < 1 || !cols) { set_error("%s: n_channels, n_chunks or columns invalid", op); return MTS_E_ARG; }
    if (window_rows < 1) { set_error("window_rows %ld < 1", window_rows); return MTS_E_ARG; }
    if (row_begin < 0 || row_end < row_begin) { set_error("row range [%ld, %ld) invalid", row_begin, row_end); return MTS_E_ARG; }
    return MTS_OK;
}

}  // namespace

// ---- per-window statistics (mts_window_stats, mts_dev_window_stats) ---------------------------------
// Tiles of STAT_TILE_ROWS rows (stats.hip), one partial per (tile, column); one combine launch at the end takes the tiles of
// window w, [win_tiles[w], win_tiles[w + 1]), in row order.
static int window_stats_run(Engine &E, hipStream_t st, const ChunkTable &T, long row_begin, long row_end, long window_rows, int n_cols,
                            const int *cols, void *o_min, void *o_max, void *o_sum, void *o_sq, bool out_on_host, long *count, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const int nc = T.nc, sz = T.sz, flags = T.flags;
    int rc;
    if ((rc = check_windows("window stats", T, row_begin, row_end, window_rows, n_cols, cols))) return rc;
    if ((rc = check_columns(cols, n_cols, nc))) return rc;
    const bool exact = !(flags & MTS_FLAG_FLOAT) && sz <= 2;
    const long span = row_end - row_begin;
    if (exact && (window_rows < span ? window_rows : span) > (1l << 31)) { set_error("windows of more than 2^31 rows on the exact path"); return MTS_E_ARG; }
    if ((rc = check_chunk_table(false, T, row_begin, row_end))) return rc;
    const long n_win = (span + window_rows - 1) / window_rows;
    if (n_win && (!o_min || !o_max || !o_sum || !o_sq || !count)) return MTS_E_ARG;
    if (n_win == 0) return MTS_OK;                           // (no chunk can hold a row of an empty range: n_chunks is 0)

    TileFeed R(T, out_on_host);
    if ((rc = R.plan(row_begin, row_end, window_rows, STAT_TILE_ROWS, false, n_cols, count))) return rc;
    const long n_tiles = R.n_tiles;
    std::vector<long> win_tiles(n_win + 1, 0);
    for (long t = 0; t < n_tiles; t++) win_tiles[R.P->tile_win[t] + 1]++;
    for (long w = 0; w < n_win; w++) win_tiles[w + 1] += win_tiles[w];

    // ---- workspace
    const u64 plane = (u64)n_tiles * n_cols * 8, n_items = (u64)n_win * n_cols;
    const size_t o_wt = R.L.take(8 * (u64)(n_win + 1)), o_slab = R.L.take(4 * plane), o_omin = R.L.take_out(n_items * sz),
                 o_omax = R.L.take_out(n_items * sz), o_osum = R.L.take_out(n_items * 8), o_osq = R.L.take_out(n_items * 8);
    if ((rc = R.place(E, st, n_cols, cols, status))) return rc;
    u8 *ws = R.ws;
    long *d_wt = (long *)(ws + o_wt);
    u8 *d_slab = ws + o_slab;
    MTS_HIP(hipMemcpyAsync(d_wt, win_tiles.data(), 8 * (size_t)(n_win + 1), hipMemcpyHostToDevice, st));
    rc = R.run(E, st, status, [&](const int *d_ids, long n) {
        return launch_stats_tiles(st, sz, flags, R.d_tiles, d_ids, (int)n, R.d_ok, R.d_cols, n_cols, nc, d_slab, n_tiles);
    });
    if (rc) return rc;
    // ---- windows: the tiles in order
    void *c_min = R.L.out(ws, o_omin, o_min), *c_max = R.L.out(ws, o_omax, o_max), *c_sum = R.L.out(ws, o_osum, o_sum), *c_sq = R.L.out(ws, o_osq, o_sq);
    if ((rc = launch_stats_combine(st, sz, flags, d_slab, n_tiles, d_wt, n_win, n_cols, c_min, c_max, c_sum, c_sq))) return rc;
    if (out_on_host) {                                        // the results, and nothing else, cross the bus
        MTS_HIP(hipMemcpyAsync(o_min, c_min, n_items * sz, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_max, c_max, n_items * sz, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_sum, c_sum, n_items * 8, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_sq, c_sq, n_items * 8, hipMemcpyDeviceToHost, st));
    }
    MTS_HIP(hipStreamSynchronize(st));
    R.P->add_counts(R.ok, count);                             // (after the last wait: count[] stays zero on every error)
    return MTS_OK;
}

// ---- one round of a radix select (mts_rank_hist, mts_dev_rank_hist) ---------------------------------
// Tiles of SEL_TILE_ROWS rows and no combine launch: every tile adds its counts to the histograms of its window with integer
// atomics (select.hip), so the outputs are the same whatever the order of the launches.
static int rank_hist_run(Engine &E, hipStream_t st, const ChunkTable &T, long row_begin, long row_end, long window_rows, int n_cols, const int *cols,
                         int mode, const double *center, const unsigned long long *sel_prefix, const int *sel_shift, unsigned int *o_hist,
                         unsigned long long *o_kmin, unsigned long long *o_kmax, bool out_on_host, long *count, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const int nc = T.nc, sz = T.sz, flags = T.flags;
    int rc;
    if ((rc = check_windows("rank hist", T, row_begin, row_end, window_rows, n_cols, cols))) return rc;
    if (mode < 0 || mode > 2) { set_error("rank hist: mode %d (0, 1 or 2)", mode); return MTS_E_ARG; }
    if ((rc = check_columns(cols, n_cols, nc))) return rc;
    const long span = row_end - row_begin;
    if ((window_rows < span ? window_rows : span) >= (1l << 32)) { set_error("windows of 2^32 rows or more"); return MTS_E_ARG; }
    if ((rc = check_chunk_table(false, T, row_begin, row_end))) return rc;
    const long n_win = (span + window_rows - 1) / window_rows;
    if (n_win && (!o_hist || !o_kmin || !o_kmax || !count || !sel_prefix || !sel_shift || (mode && !center))) {
        set_error("rank hist: selectors, center or outputs missing"); return MTS_E_ARG;
    }
    const int key_bits = mode ? 64 : 8 * sz;
    const u64 n_sel = (u64)n_win * MTS_RANK_SELECTORS * n_cols;
    for (u64 e = 0; e < n_sel; e++) {
        const int sh = sel_shift[e];
        if (sh < 0) continue;
        const int above = key_bits - sh - MTS_RANK_BITS;     // bits of the key above the digit
        if (above < 0) { set_error("rank hist: shift %d above key_bits - %d", sh, MTS_RANK_BITS); return MTS_E_ARG; }
        if (above < 64 && (sel_prefix[e] >> above)) { set_error("rank hist: a prefix of more than %d bits at shift %d", above, sh); return MTS_E_ARG; }
    }
    if (n_win == 0) return MTS_OK;                           // (no chunk can hold a row of an empty range: n_chunks is 0)

    TileFeed R(T, out_on_host);
    if ((rc = R.plan(row_begin, row_end, window_rows, SEL_TILE_ROWS, true, n_cols, count))) return rc;

    // ---- workspace
    const u64 n_cells = (u64)n_win * n_cols, hist_bytes = n_sel * (4ull << MTS_RANK_BITS), k_bytes = n_sel * 8;
    const size_t o_cen = R.L.take(mode ? 8 * n_cells : 0), o_pre = R.L.take(k_bytes), o_shf = R.L.take(n_sel * 4), w_hist = R.L.take_out(hist_bytes),
                 w_kmin = R.L.take_out(k_bytes), w_kmax = R.L.take_out(k_bytes);
    if ((rc = R.place(E, st, n_cols, cols, status))) return rc;
    u8 *ws = R.ws;
    int *d_shf = (int *)(ws + o_shf);
    double *d_cen = (double *)(ws + o_cen);
    u64 *d_pre = (u64 *)(ws + o_pre);
    u32 *d_hist = R.L.out(ws, w_hist, (u32 *)o_hist);
    u64 *d_kmin = R.L.out(ws, w_kmin, (u64 *)o_kmin), *d_kmax = R.L.out(ws, w_kmax, (u64 *)o_kmax);
    if (mode) MTS_HIP(hipMemcpyAsync(d_cen, center, 8 * (size_t)n_cells, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_pre, sel_prefix, (size_t)k_bytes, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_shf, sel_shift, 4 * (size_t)n_sel, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemsetAsync(d_hist, 0, (size_t)hist_bytes, st));
    MTS_HIP(hipMemsetAsync(d_kmin, 0xff, (size_t)k_bytes, st));
    MTS_HIP(hipMemsetAsync(d_kmax, 0, (size_t)k_bytes, st));
    rc = R.run(E, st, status, [&](const int *d_ids, long n) {
        return launch_rank_hist(st, sz, flags, mode, R.d_tiles, R.d_tw, d_ids, (int)n, R.d_ok, R.d_cols, n_cols, nc, d_cen, d_pre, d_shf, d_hist, d_kmin,
                                d_kmax);
    });
    if (rc) return rc;
    if (out_on_host) {                                        // the histograms, and nothing else, cross the bus
        MTS_HIP(hipMemcpyAsync(o_hist, d_hist, (size_t)hist_bytes, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_kmin, d_kmin, (size_t)k_bytes, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_kmax, d_kmax, (size_t)k_bytes, hipMemcpyDeviceToHost, st));
    }
    MTS_HIP(hipStreamSynchronize(st));
    R.P->add_counts(R.ok, count);                             // (after the last wait: count[] stays zero on every error)
    return MTS_OK;
}

// ---- decimation (mts_decimate, mts_dev_decimate) ---------------------------------------------------------------------------
// The unit is an output.  Piece p owns the outputs whose newest row (first_row + k * q) lies in its chunks; their support reaches
// L - 1 rows further down, so a piece reads its own chunks and those of the halo below.  Every output is computed once, from the
// same rows, in the same order: the result does not depend on the pieces.
static int decimate_run(Engine &E, hipStream_t st, const ChunkTable &T, long vb, long ve, long first_row, long n_out, int q, int n_taps,
                        const double *taps, int osz, int n_cols, const int *cols, void *out, bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const int nc = T.nc, sz = T.sz, flags = T.flags;
    int rc;
    if (nc <= 0 || T.n_chunks < 0 || n_cols < 1 || n_cols > 64 * 65535 || !cols) { set_error("decimate: n_channels, n_chunks or columns invalid"); return MTS_E_ARG; }
    if (q < 1) { set_error("decimate: q %d < 1", q); return MTS_E_ARG; }
    if ((rc = check_taps("decimate", n_taps, taps))) return rc;
    if (osz != 4 && osz != 8) { set_error("decimate: output itemsize %d (4 or 8)", osz); return MTS_E_ARG; }
    if (vb < 0 || ve < vb || n_out < 0 || n_out > (1l << 40) || first_row < -(1l << 60) || first_row > (1l << 60)) {
        set_error("decimate: rows or outputs invalid"); return MTS_E_ARG;
    }
    if (n_out && !out) { set_error("decimate: no output buffer"); return MTS_E_ARG; }
    if ((rc = check_columns(cols, n_cols, nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    // the rows that outputs [u0, u1) read: support ∩ valid range
    auto rows = [&](long u0, long u1, long *lo, long *hi) {
        *lo = std::max(vb, first_row + u0 * q - (n_taps - 1)); *hi = std::min(ve, first_row + (u1 - 1) * q + 1);
    };
    long need_lo = 0, need_hi = 0;
    if (n_out) rows(0, n_out, &need_lo, &need_hi);
    if ((rc = check_cover("decimate", T, need_lo, need_hi))) return rc;
    status_ok(T, status);
    if (n_out == 0) return MTS_OK;

    HaloFeed H(T, out_on_host);
    // the first output whose newest row is at or after row r
    if ((rc = H.plan(n_out, [&](long r) { return r <= first_row ? 0 : (r - first_row + q - 1) / q; }, rows))) return rc;
    // ---- workspace
    const u64 n_items = (u64)n_out * n_cols;
    WsLayout &L = H.L;
    const size_t o_taps = L.take(8 * (u64)n_taps), o_cols = L.take(4 * (u64)n_cols), o_seg = L.take(H.table_bytes()), o_out = L.take_out(n_items * osz);
    if ((rc = H.place(E, st, E.dec, o_seg))) return rc;
    u8 *ws = E.dec.as<u8>();
    std::vector<u8> h_taps(8 * (size_t)n_taps);
    for (int j = 0; j < n_taps; j++) {
        if (osz == 4) { const float f = (float)taps[j]; memcpy(h_taps.data() + 4 * j, &f, 4); }
        else memcpy(h_taps.data() + 8 * j, &taps[j], 8);
    }
    MTS_HIP(hipMemcpyAsync(ws + o_taps, h_taps.data(), (size_t)osz * n_taps, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    void *d_out = L.out(ws, o_out, out);
    rc = H.run(E, st, status, [&](const FeedPiece &G, const PieceSegs &S) {
        // (nothing valid to read, ns == 0: every row is 0)
        return launch_decimate(st, sz, flags, osz, S.base, S.row0, S.ns, nc, (const int *)(ws + o_cols), n_cols, ws + o_taps, n_taps, q, first_row, G.u0,
                               G.u1, S.ns ? vb : 0, S.ns ? ve : 0, (u8 *)d_out + (u64)G.u0 * n_cols * osz);
    });
    if (rc) return rc;
    if (out_on_host) MTS_HIP(hipMemcpyAsync(out, d_out, n_items * osz, hipMemcpyDeviceToHost, st));
    MTS_HIP(hipStreamSynchronize(st));
    return MTS_OK;
}

// ---- channel-mixing products (mts_project, mts_dev_project) --------------------------------------------------------------------
// The unit is a row of [row_begin, row_end) and the halo is empty: piece p owns the rows in its chunks and reads those chunks alone,
// so no chunk is decoded twice and chunks outside the range are not read.  A row's outputs depend on that row only: the result does
// not depend on the pieces.
static int project_run(Engine &E, hipStream_t st, const ChunkTable &T, long row_begin, long row_end, int n_cols, const int *cols, const double *offset,
                       int n_out, const double *weights, int osz, void *out, bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const int nc = T.nc, sz = T.sz, flags = T.flags;
    int rc;
    if (nc <= 0 || T.n_chunks < 0) { set_error("project: n_channels or n_chunks invalid"); return MTS_E_ARG; }
    if (n_cols < 1 || n_cols > MTS_PROJECT_MAX_COLS || !cols) { set_error("project: %d columns (1 .. %d)", n_cols, MTS_PROJECT_MAX_COLS); return MTS_E_ARG; }
    if (n_out < 1 || n_out > MTS_PROJECT_MAX_OUT || !weights) { set_error("project: %d outputs (1 .. %d)", n_out, MTS_PROJECT_MAX_OUT); return MTS_E_ARG; }
    if (osz != 4 && osz != 8) { set_error("project: output itemsize %d (4 or 8)", osz); return MTS_E_ARG; }
    for (long e = 0; e < (long)n_cols * n_out; e++)
        if (!std::isfinite(weights[e])) { set_error("project: weight (%ld, %ld) is not finite", e / n_out, e % n_out); return MTS_E_ARG; }
    for (int j = 0; offset && j < n_cols; j++)
        if (!std::isfinite(offset[j])) { set_error("project: offset %d is not finite", j); return MTS_E_ARG; }
    if (row_begin < 0 || row_end < row_begin || row_end - row_begin > (1l << 40)) { set_error("project: rows [%ld, %ld) invalid", row_begin, row_end); return MTS_E_ARG; }
    if (row_end > row_begin && !out) { set_error("project: no output buffer"); return MTS_E_ARG; }
    if ((rc = check_columns(cols, n_cols, nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    if ((rc = check_cover("project", T, row_begin, row_end))) return rc;
    status_ok(T, status);
    if (row_begin == row_end) return MTS_OK;

    HaloFeed H(T, out_on_host);
    rc = H.plan(row_end - row_begin, [&](long r) { return r - row_begin; },
                [&](long u0, long u1, long *lo, long *hi) { *lo = row_begin + u0; *hi = row_begin + u1; });
    if (rc) return rc;
    // ---- workspace: weights (padded with zeros to multiples of PROJECT_PAD rows and columns), offsets, columns, segment tables, output
    const int kp = (int)align_up((u64)n_cols, PROJECT_PAD), wp = (int)align_up((u64)n_out, PROJECT_PAD);
    const u64 n_items = (u64)(row_end - row_begin) * n_out;
    WsLayout &L = H.L;
    const size_t o_w = L.take((u64)osz * kp * wp), o_off = L.take((u64)osz * n_cols), o_cols = L.take(4 * (u64)n_cols), o_seg = L.take(H.table_bytes()),
                 o_out = L.take_out(n_items * osz);
    if ((rc = H.place(E, st, E.proj, o_seg))) return rc;
    u8 *ws = E.proj.as<u8>();
    // weights and offsets rounded once to the compute type
    std::vector<u8> h_w((size_t)osz * kp * wp + (size_t)osz * n_cols, 0);
    u8 *h_off = h_w.data() + (size_t)osz * kp * wp;
    for (int j = 0; j < n_cols; j++) {
        if (osz == 4) {
            float *d = (float *)h_w.data() + (size_t)j * wp;
            for (int k = 0; k < n_out; k++) d[k] = (float)weights[(size_t)j * n_out + k];
            ((float *)h_off)[j] = offset ? (float)offset[j] : 0.0f;
        } else {
            memcpy(h_w.data() + 8 * (size_t)j * wp, weights + (size_t)j * n_out, 8 * (size_t)n_out);
            ((double *)h_off)[j] = offset ? offset[j] : 0.0;
        }
    }
    MTS_HIP(hipMemcpyAsync(ws + o_w, h_w.data(), (size_t)osz * kp * wp, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_off, h_off, (size_t)osz * n_cols, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    void *d_out = L.out(ws, o_out, out);
    rc = H.run(E, st, status, [&](const FeedPiece &P, const PieceSegs &S) {
        return launch_project(st, sz, flags, osz, S.base, S.row0, S.ns, nc, (const int *)(ws + o_cols), ws + o_off, n_cols, ws + o_w, wp, n_out,
                              row_begin + P.u0, row_begin + P.u1, (u8 *)d_out + (u64)P.u0 * n_out * osz);
    });
    if (rc) { (void)hipStreamSynchronize(st); return rc; }   // (h_w has been read before it goes)
    if (out_on_host) MTS_HIP(hipMemcpyAsync(out, d_out, n_items * osz, hipMemcpyDeviceToHost, st));
    MTS_HIP(hipStreamSynchronize(st));
    return MTS_OK;
}

// ---- peak detection (mts_detect, mts_dev_detect) -------------------------------------------------------------------------------
// The unit is a row of [row_begin, row_end).  Piece p owns the rows in its chunks; their events need the detection value R rows either
// side, and that the filter's support: the rows [u0, u1) read the file rows from u0 - R + half - (L - 1) to u1 - 1 + R + half,
// within the valid range.  A piece's rows go through the float32 workspace in slabs that keep it <= the slab bound
// (filter -> median -> mask -> count / scan / emit on the stream); the write position is carried on the device from slab to slab and
// piece to piece.  Every value is computed from the same rows in the same order whatever the pieces and slabs.
static const u64 DETECT_SLAB_BYTES = 256ull << 20;
static const long DETECT_SLAB_MAX_ROWS = 1l << 22;                  // (bounds the bitmap of narrow selections: <= 32 MiB up to 64 columns)

static int detect_run(Engine &E, hipStream_t st, const ChunkTable &T, const ZArgs &Z, long row_begin, long row_end, const float *threshold, int sign,
                      int R, int S, long max_events, long *out_row, int *out_pos, float *out_amp, bool out_on_host, long *n_events, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const long vb = Z.vb, ve = Z.ve;
    const int n_cols = Z.n_cols;
    int rc;
    if ((rc = check_zargs(T, Z))) return rc;
    if (!threshold) { set_error("detect: no thresholds"); return MTS_E_ARG; }
    for (int j = 0; j < n_cols; j++)
        if (!std::isfinite(threshold[j]) || !(threshold[j] > 0)) { set_error("detect: threshold %d is not a finite positive number", j); return MTS_E_ARG; }
    if (sign < 0 || sign > 2) { set_error("detect: sign %d (0 neg, 1 pos, 2 both)", sign); return MTS_E_ARG; }
    if (R < 0 || R > MTS_DETECT_MAX_EXCLUDE || S < 0 || S > MTS_DETECT_MAX_SPREAD) {
        set_error("detect: exclude_rows %d (0 .. %d) or exclude_cols %d (0 .. %d)", R, MTS_DETECT_MAX_EXCLUDE, S, MTS_DETECT_MAX_SPREAD); return MTS_E_ARG;
    }
    if (row_begin < vb || row_end < row_begin || row_end > ve) { set_error("detect: rows invalid"); return MTS_E_ARG; }
    if (max_events < 0 || max_events > (1l << 40) || !n_events) { set_error("detect: max_events invalid or no n_events"); return MTS_E_ARG; }
    if (max_events && (!out_row || !out_pos || !out_amp)) { set_error("detect: no output buffers"); return MTS_E_ARG; }
    if ((rc = check_columns(Z.cols, n_cols, T.nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    const long half = (Z.n_taps - 1) / 2, n_units = row_end - row_begin;
    // the rows that the events of rows [u0, u1) read: (rows + R either side)'s support ∩ valid range
    auto rows = [&](long u0, long u1, long *lo, long *hi) {
        *lo = std::max(vb, row_begin + u0 - R + half - (Z.n_taps - 1)); *hi = std::min(ve, row_begin + u1 + R + half);
    };
    long need_lo = 0, need_hi = 0;
    if (n_units) rows(0, n_units, &need_lo, &need_hi);
    if ((rc = check_cover("detect", T, need_lo, need_hi))) return rc;
    status_ok(T, status);
    *n_events = 0;
    if (!n_units) return MTS_OK;

    HaloFeed H(T, out_on_host);
    if ((rc = H.plan(n_units, [&](long r) { return r - row_begin; }, rows))) return rc;
    // rows a slab owns: the workspace holds them and R rows either side
    const long cap_rows = (long)std::min<u64>(env_bytes("MTS_DETECT_SLAB_BYTES", DETECT_SLAB_BYTES) / (4 * (u64)n_cols), (u64)DETECT_SLAB_MAX_ROWS);
    const long own = std::min(n_units, std::max(1l, cap_rows - 2l * R));
    const long max_words = detect_bitmap_words(own, n_cols), max_blocks = detect_blocks(max_words);
    // ---- workspace
    WsLayout &L = H.L;
    ZStage F(Z, L);
    const size_t o_thr = L.take(4 * (u64)n_cols), o_seg = L.take(H.table_bytes());
    EventTail EV(L);
    const size_t o_y = L.take(4 * (u64)(own + 2l * R) * n_cols), o_bits = L.take(8 * (u64)max_words), o_cnt = L.take(4 * (u64)max_blocks),
                 o_offs = L.take(8 * (u64)max_blocks), o_row = L.take_out(8 * (u64)max_events), o_pos = L.take_out(4 * (u64)max_events),
                 o_amp = L.take_out(4 * (u64)max_events);
    StreamGuard G{st};
    if ((rc = H.place(E, st, E.det, o_seg))) return rc;
    u8 *ws = E.det.as<u8>();
    if ((rc = F.upload(st, ws))) return rc;
    MTS_HIP(hipMemcpyAsync(ws + o_thr, threshold, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    if ((rc = EV.begin(st, ws))) return rc;
    long *d_row = L.out(ws, o_row, out_row);
    int *d_pos = L.out(ws, o_pos, out_pos);
    float *d_amp = L.out(ws, o_amp, out_amp);
    float *d_y = (float *)(ws + o_y);
    u64 *d_bits = (u64 *)(ws + o_bits);
    rc = H.run(E, st, status, [&](const FeedPiece &Pc, const PieceSegs &Sg) {
        const long p0 = row_begin + Pc.u0, p1 = row_begin + Pc.u1;
        int r = MTS_OK;
        for (long s0 = p0; !r && s0 < p1; s0 += own) {
            const long s1 = std::min(p1, s0 + own), a = std::max(vb, s0 - R), b = std::min(ve, s1 + R);
            r = F.filter(st, T, Sg, a, b, d_y);
            if (!r) r = launch_detect_mask(st, d_y, a, b - a, n_cols, (const float *)(ws + o_thr), sign, R, S, s0, s1, d_bits);
            if (!r) r = launch_detect_emit(st, d_bits, detect_bitmap_words(s1 - s0, n_cols), (u32 *)(ws + o_cnt), (u64 *)(ws + o_offs), EV.d_total, d_y,
                                           a, n_cols, s0, max_events, d_row, d_pos, d_amp);
        }
        return r;
    });
    if (rc) return rc;
    return EV.finish(G, max_events, out_on_host, n_events, out_row, d_row, out_pos, d_pos, out_amp, d_amp);
}

// ---- snippets around events (mts_waveforms, mts_dev_waveforms) -----------------------------------------------------------------
// The unit is an event; the events come by ascending row.  Piece p owns the events whose rows lie in its chunks; event e reads
// z[ev_row[e] - before, ev_row[e] + after), and that the filter's support: the events [u0, u1) read the file rows from
// ev_row[u0] - before + half - (L - 1) to ev_row[u1 - 1] + after + half, within the valid range.  A piece's events go through the
// float32 workspace in slabs (SnippetPlan: at most the slab bound, and cut where events lie further apart than the gap, so that the
// rows between them are not filtered): filter -> median -> gather.  Every value is computed from the same rows in the same order
// whatever the pieces, slabs and gap.
static const u64 WAVEFORMS_SLAB_BYTES = 256ull << 20;
static const long WAVEFORMS_GAP_ROWS = 4096;                        // (swept at 1024 / 4096 / 16384 / never: profiles/waveforms.json)

static long waveforms_gap_rows()                                     // (negative: never cut at a gap)
{
    const char *e = getenv("MTS_WAVEFORMS_GAP_ROWS");
    return e && *e ? (long)atoll(e) : WAVEFORMS_GAP_ROWS;
}

// ---- what waveforms, mean_waveforms, waveform_features and localize share: the snippet arguments and their checks, the events' pieces and slabs, the slab loop
struct SnipArgs { long n_events; const long *ev_row; const int *ev_col0; int before, after, width; };

// the first checks, in order: the filter's, the snippet's shape, the event list's pointers
static int check_snippet_shape(const ChunkTable &T, const ZArgs &Z, const SnipArgs &A)
{
    if (const int rc = check_zargs(T, Z)) return rc;
    const long n_snip = (long)A.before + (long)A.after;
    if (A.before < 0 || A.after < 0 || n_snip < 1 || n_snip > MTS_WAVEFORMS_MAX_ROWS) {
        set_error("%s: before %d, after %d (both >= 0, 1 .. %d rows in all)", Z.op, A.before, A.after, MTS_WAVEFORMS_MAX_ROWS); return MTS_E_ARG;
    }
    if (A.width < 1 || A.width > MTS_WAVEFORMS_MAX_WIDTH) { set_error("%s: width %d (1 .. %d)", Z.op, A.width, MTS_WAVEFORMS_MAX_WIDTH); return MTS_E_ARG; }
    if (A.n_events < 0 || A.n_events > (1l << 40)) { set_error("%s: %ld events (0 .. 2^40)", Z.op, A.n_events); return MTS_E_ARG; }
    if (A.n_events && (!A.ev_row || !A.ev_col0)) { set_error("%s: no events", Z.op); return MTS_E_ARG; }
    return MTS_OK;
}

// the rows that the events [u0, u1) read: their snippets' support ∩ valid range
struct SnipRows {
    const ZArgs &Z;
    const SnipArgs &A;
    void operator()(long u0, long u1, long *lo, long *hi) const
    {
        const long half = (Z.n_taps - 1) / 2;
        *lo = std::max(Z.vb, A.ev_row[u0] - A.before + half - (Z.n_taps - 1)); *hi = std::min(Z.ve, A.ev_row[u1 - 1] + A.after + half);
    }
};

// the last checks: the events' rows, the columns, the chunk table and what it covers
static int check_snippet_events(const ChunkTable &T, const ZArgs &Z, const SnipArgs &A)
{
    int rc;
    for (long e = 0; e < A.n_events; e++) {
        if (A.ev_row[e] < Z.vb || A.ev_row[e] >= Z.ve) { set_error("%s: event %ld at row %ld outside [%ld, %ld)", Z.op, e, A.ev_row[e], Z.vb, Z.ve); return MTS_E_ARG; }
        if (e && A.ev_row[e] < A.ev_row[e - 1]) { set_error("%s: event %ld: the rows must ascend", Z.op, e); return MTS_E_ARG; }
    }
    if ((rc = check_columns(Z.cols, Z.n_cols, T.nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    long need_lo = 0, need_hi = 0;
    if (A.n_events) SnipRows{Z, A}(0, A.n_events, &need_lo, &need_hi);
    return check_cover(Z.op, T, need_lo, need_hi);
}

// the events' pieces (HaloFeed) and every piece's slabs (SnippetPlan), then the slab loop: filter -> median -> the op's gather.
// report: what mts_waveforms_last_plan tells
struct SnippetFeed {
    HaloFeed H;
    std::vector<SnippetPlan> slabs;
    std::vector<long> slab0;                                  // piece p's slabs are the call's slabs [slab0[p], slab0[p + 1])
    long max_rows = 0, report[4] = {0, 0, 0, 0};
    bool timed = false;
    double gather_ms = 0;

    SnippetFeed(const ChunkTable &T, bool out_on_host) : H(T, out_on_host) {}

    int plan(Engine &E, const ZArgs &Z, const SnipArgs &A)
    {
        // the first event at or after row r
        const int rc = H.plan(A.n_events, [&](long r) { return (long)(std::lower_bound(A.ev_row, A.ev_row + A.n_events, r) - A.ev_row); }, SnipRows{Z, A});
        if (rc) return rc;
        // every piece's slabs: the workspace holds the longest
        const long cap_rows = (long)std::min<u64>(env_bytes("MTS_WAVEFORMS_SLAB_BYTES", WAVEFORMS_SLAB_BYTES) / (4 * (u64)Z.n_cols), (u64)1 << 40);
        const long gap_rows = waveforms_gap_rows();
        report[0] = (long)H.P->pieces.size();
        slab0.push_back(0);
        for (const FeedPiece &Pc : H.P->pieces) {
            slabs.emplace_back(A.ev_row, Pc.u0, Pc.u1, A.before, A.after, Z.vb, Z.ve, cap_rows, gap_rows);
            max_rows = std::max(max_rows, slabs.back().max_rows);
            report[1] += (long)slabs.back().slabs.size(); report[2] += slabs.back().gap_cuts;
            slab0.push_back(report[1]);
        }
        timed = getenv("MTS_WAVEFORMS_TIME") != nullptr;          // the gather kernel's time, slab by slab (tools/waveforms_bench.py)
        if (timed && !E.wav_ev[0]) { MTS_HIP(hipEventCreate(&E.wav_ev[0])); MTS_HIP(hipEventCreate(&E.wav_ev[1])); }
        return MTS_OK;
    }

    // gather(slab, its number in the call) after the slab's rows are filtered into d_y
    template <class Gather>
    int run(Engine &E, hipStream_t st, const ChunkTable &T, const ZStage &F, float *d_y, int *status, Gather &&gather)
    {
        return H.run(E, st, status, [&](const FeedPiece &Pc, const PieceSegs &Sg) {
            int r = MTS_OK;
            const size_t p = (size_t)(&Pc - H.P->pieces.data());
            long k = slab0[p];
            for (const SnippetSlab &S : slabs[p].slabs) {
                r = F.filter(st, T, Sg, S.a, S.b, d_y);
                if (!r && timed) (void)hipEventRecord(E.wav_ev[0], st);
                if (!r) r = gather(S, k++);
                if (!r && timed) {
                    float ms = 0;
                    (void)hipEventRecord(E.wav_ev[1], st);
                    (void)hipEventSynchronize(E.wav_ev[1]);
                    (void)hipEventElapsedTime(&ms, E.wav_ev[0], E.wav_ev[1]);
                    gather_ms += ms;
                }
                if (r) break;
            }
            return r;
        });
    }

    void done(Engine &E)
    {
        report[3] = (long)(gather_ms * 1e3);
        memcpy(E.wav_plan, report, sizeof report);
    }
};

static int waveforms_run(Engine &E, hipStream_t st, const ChunkTable &T, const ZArgs &Z, long n_events, const long *ev_row, const int *ev_col0,
                         int before, int after, int width, float *out_wave, float *out_min, int *out_argmin, float *out_max, int *out_argmax,
                         bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const long vb = Z.vb, ve = Z.ve;
    const int n_cols = Z.n_cols;
    const SnipArgs A{n_events, ev_row, ev_col0, before, after, width};
    int rc;
    if ((rc = check_snippet_shape(T, Z, A))) return rc;
    if (!out_min || !out_argmin || !out_max || !out_argmax) { set_error("waveforms: no extrema buffers"); return MTS_E_ARG; }
    if ((rc = check_snippet_events(T, Z, A))) return rc;
    status_ok(T, status);
    if (n_events == 0) return MTS_OK;

    SnippetFeed S(T, out_on_host);
    HaloFeed &H = S.H;
    if ((rc = S.plan(E, Z, A))) return rc;
    // ---- workspace
    const u64 n_item = (u64)((long)before + after) * width;
    WsLayout &L = H.L;
    ZStage F(Z, L);
    const size_t o_seg = L.take(H.table_bytes()), o_erow = L.take(8 * (u64)n_events), o_ecol = L.take(4 * (u64)n_events),
                 o_y = L.take(4 * (u64)S.max_rows * n_cols), o_wave = out_wave ? L.take_out(4 * (u64)n_events * n_item) : 0,
                 o_min = L.take_out(4 * (u64)n_events), o_amin = L.take_out(4 * (u64)n_events), o_max = L.take_out(4 * (u64)n_events),
                 o_amax = L.take_out(4 * (u64)n_events);
    StreamGuard G{st};
    if ((rc = H.place(E, st, E.wav, o_seg))) return rc;
    u8 *ws = E.wav.as<u8>();
    if ((rc = F.upload(st, ws))) return rc;
    MTS_HIP(hipMemcpyAsync(ws + o_erow, ev_row, 8 * (size_t)n_events, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_ecol, ev_col0, 4 * (size_t)n_events, hipMemcpyHostToDevice, st));
    float *d_wave = out_wave ? L.out(ws, o_wave, out_wave) : nullptr;
    float *d_min = L.out(ws, o_min, out_min), *d_max = L.out(ws, o_max, out_max);
    int *d_amin = L.out(ws, o_amin, out_argmin), *d_amax = L.out(ws, o_amax, out_argmax);
    float *d_y = (float *)(ws + o_y);
    rc = S.run(E, st, T, F, d_y, status, [&](const SnippetSlab &B, long) {
        return launch_waveforms(st, d_y, B.a, B.b - B.a, n_cols, vb, ve, (const long *)(ws + o_erow), (const int *)(ws + o_ecol), B.e0, B.e1, before,
                                after, width, d_wave, d_min, d_amin, d_max, d_amax);
    });
    if (rc) return rc;
    if (out_on_host) {
        if (out_wave) MTS_HIP(hipMemcpyAsync(out_wave, d_wave, 4 * (size_t)n_events * n_item, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_min, d_min, 4 * (size_t)n_events, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_argmin, d_amin, 4 * (size_t)n_events, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_max, d_max, 4 * (size_t)n_events, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_argmax, d_amax, 4 * (size_t)n_events, hipMemcpyDeviceToHost, st));
    }
    if ((rc = G.wait())) return rc;
    S.done(E);
    return MTS_OK;
}

// ---- snippets projected on a temporal basis (mts_waveform_features, mts_dev_waveform_features) ---------------------------------------
// waveforms' events, pieces, slabs and filter stage; the gather is k_waveform_features (features.hip), which reads the same entries of z
// and keeps n_comp numbers of every T: one thread owns a chain from +0 to its store, so the bytes depend on no cut made here.
static int waveform_features_run(Engine &E, hipStream_t st, const ChunkTable &T, const ZArgs &Z, long n_events, const long *ev_row,
                                 const int *ev_col0, int before, int after, int width, int n_comp, const float *basis, float *out_feat,
                                 bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const long vb = Z.vb, ve = Z.ve;
    const int n_cols = Z.n_cols;
    const SnipArgs A{n_events, ev_row, ev_col0, before, after, width};
    int rc;
    if ((rc = check_snippet_shape(T, Z, A))) return rc;
    const long n_snip = (long)before + after;
    if (n_comp < 1 || n_comp > MTS_FEATURES_MAX_COMPONENTS) {
        set_error("waveform_features: %d components (1 .. %d)", n_comp, MTS_FEATURES_MAX_COMPONENTS); return MTS_E_ARG;
    }
    if ((long)n_comp * n_snip > MTS_FEATURES_MAX_BASIS) {
        set_error("waveform_features: %d components x %ld rows (<= %d entries in all)", n_comp, n_snip, MTS_FEATURES_MAX_BASIS); return MTS_E_ARG;
    }
    if (!basis) { set_error("waveform_features: no basis"); return MTS_E_ARG; }
    if (!out_feat) { set_error("waveform_features: no output buffer"); return MTS_E_ARG; }
    const size_t n_basis = (size_t)n_comp * (size_t)n_snip;
    for (size_t k = 0; k < n_basis; k++)
        if (!std::isfinite(basis[k])) {
            set_error("waveform_features: basis[%d, %ld] is not finite", (int)(k / (size_t)n_snip), (long)(k % (size_t)n_snip)); return MTS_E_ARG;
        }
    if ((rc = check_snippet_events(T, Z, A))) return rc;
    status_ok(T, status);
    if (n_events == 0) return MTS_OK;

    SnippetFeed S(T, out_on_host);
    HaloFeed &H = S.H;
    if ((rc = S.plan(E, Z, A))) return rc;
    std::vector<float> image(n_basis);                             // the basis as the kernel stages it
    features_basis_image(basis, n_comp, (int)n_snip, image.data());
    // ---- workspace
    const u64 n_item = (u64)n_comp * width;
    WsLayout &L = H.L;
    ZStage F(Z, L);
    const size_t o_seg = L.take(H.table_bytes()), o_erow = L.take(8 * (u64)n_events), o_ecol = L.take(4 * (u64)n_events),
                 o_basis = L.take(4 * (u64)n_basis), o_y = L.take(4 * (u64)S.max_rows * n_cols), o_feat = L.take_out(4 * (u64)n_events * n_item);
    StreamGuard G{st};
    if ((rc = H.place(E, st, E.wav, o_seg))) return rc;
    u8 *ws = E.wav.as<u8>();
    if ((rc = F.upload(st, ws))) return rc;
    MTS_HIP(hipMemcpyAsync(ws + o_erow, ev_row, 8 * (size_t)n_events, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_ecol, ev_col0, 4 * (size_t)n_events, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_basis, image.data(), 4 * n_basis, hipMemcpyHostToDevice, st));
    float *d_feat = L.out(ws, o_feat, out_feat);
    float *d_y = (float *)(ws + o_y);
    rc = S.run(E, st, T, F, d_y, status, [&](const SnippetSlab &B, long) {
        return launch_waveform_features(st, d_y, B.a, B.b - B.a, n_cols, vb, ve, (const long *)(ws + o_erow), (const int *)(ws + o_ecol), B.e0, B.e1,
                                        before, after, width, n_comp, (const float *)(ws + o_basis), d_feat);
    });
    if (rc) return rc;
    if (out_on_host) MTS_HIP(hipMemcpyAsync(out_feat, d_feat, 4 * (size_t)n_events * n_item, hipMemcpyDeviceToHost, st));
    if ((rc = G.wait())) return rc;
    S.done(E);
    return MTS_OK;
}

// ---- channel amplitudes and amplitude-weighted position sums of snippets (mts_localize, mts_dev_localize) ---------------------------
// waveforms' events, pieces, slabs and filter stage; the gather is k_localize (localize.hip), which reads the same entries of z and keeps
// width + n_dims + 2 numbers of an event: one thread owns an event's chains from +0 to their stores, so the bytes depend on no cut made here.
static int localize_run(Engine &E, hipStream_t st, const ChunkTable &T, const ZArgs &Z, long n_events, const long *ev_row, const int *ev_col0,
                        int before, int after, int width, int mode, int n_dims, const float *positions, float *out_amp, float *out_weight,
                        float *out_moment, int *out_best, bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const long vb = Z.vb, ve = Z.ve;
    const int n_cols = Z.n_cols;
    const SnipArgs A{n_events, ev_row, ev_col0, before, after, width};
    int rc;
    if ((rc = check_snippet_shape(T, Z, A))) return rc;
    if (mode < MTS_LOCALIZE_PTP || mode > MTS_LOCALIZE_ABS) { set_error("localize: mode %d (0 .. 3)", mode); return MTS_E_ARG; }
    if (n_dims < 1 || n_dims > MTS_LOCALIZE_MAX_DIMS) { set_error("localize: %d dimensions (1 .. %d)", n_dims, MTS_LOCALIZE_MAX_DIMS); return MTS_E_ARG; }
    if (!positions) { set_error("localize: no positions"); return MTS_E_ARG; }
    if (!out_weight || !out_moment || !out_best) { set_error("localize: no weight, moment or best buffer"); return MTS_E_ARG; }
    const size_t n_pos = (size_t)n_cols * (size_t)n_dims;
    for (size_t k = 0; k < n_pos; k++)
        if (!std::isfinite(positions[k])) {
            set_error("localize: positions[%ld, %d] is not finite", (long)(k / (size_t)n_dims), (int)(k % (size_t)n_dims)); return MTS_E_ARG;
        }
    if ((rc = check_snippet_events(T, Z, A))) return rc;
    status_ok(T, status);
    if (n_events == 0) return MTS_OK;

    SnippetFeed S(T, out_on_host);
    HaloFeed &H = S.H;
    if ((rc = S.plan(E, Z, A))) return rc;
    // ---- workspace
    WsLayout &L = H.L;
    ZStage F(Z, L);
    const size_t o_seg = L.take(H.table_bytes()), o_erow = L.take(8 * (u64)n_events), o_ecol = L.take(4 * (u64)n_events),
                 o_pos = L.take(4 * (u64)n_pos), o_y = L.take(4 * (u64)S.max_rows * n_cols),
                 o_amp = out_amp ? L.take_out(4 * (u64)n_events * width) : 0, o_wgt = L.take_out(4 * (u64)n_events),
                 o_mom = L.take_out(4 * (u64)n_events * n_dims), o_best = L.take_out(4 * (u64)n_events);
    StreamGuard G{st};
    if ((rc = H.place(E, st, E.wav, o_seg))) return rc;
    u8 *ws = E.wav.as<u8>();
    if ((rc = F.upload(st, ws))) return rc;
    MTS_HIP(hipMemcpyAsync(ws + o_erow, ev_row, 8 * (size_t)n_events, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_ecol, ev_col0, 4 * (size_t)n_events, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_pos, positions, 4 * n_pos, hipMemcpyHostToDevice, st));
    float *d_amp = out_amp ? L.out(ws, o_amp, out_amp) : nullptr;
    float *d_wgt = L.out(ws, o_wgt, out_weight), *d_mom = L.out(ws, o_mom, out_moment);
    int *d_best = L.out(ws, o_best, out_best);
    float *d_y = (float *)(ws + o_y);
    rc = S.run(E, st, T, F, d_y, status, [&](const SnippetSlab &B, long) {
        return launch_localize(st, d_y, B.a, B.b - B.a, n_cols, vb, ve, (const long *)(ws + o_erow), (const int *)(ws + o_ecol), B.e0, B.e1, before,
                               after, width, mode, n_dims, (const float *)(ws + o_pos), d_amp, d_wgt, d_mom, d_best);
    });
    if (rc) return rc;
    if (out_on_host) {
        if (out_amp) MTS_HIP(hipMemcpyAsync(out_amp, d_amp, 4 * (size_t)n_events * width, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_weight, d_wgt, 4 * (size_t)n_events, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_moment, d_mom, 4 * (size_t)n_events * n_dims, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_best, d_best, 4 * (size_t)n_events, hipMemcpyDeviceToHost, st));
    }
    if ((rc = G.wait())) return rc;
    S.done(E);
    return MTS_OK;
}

// ---- per-label sums of snippets (mts_mean_waveforms, mts_dev_mean_waveforms) -----------------------------------------------------
// waveforms' events, pieces, slabs and filter stage; the gather is a segmented reduction: every slab's events are grouped by label and
// cut into parts of MTS_MEAN_PART_EVENTS events (MeanParts: a plan made for all slabs before the first upload), and k_mean_waveforms
// adds each part's entries in fixed point to the label's sums and counts with integer atomics (meanwave.hip).  Integer sums do not
// depend on the order: the same bytes whatever the pieces, slabs, gap and parts.
static const long MEAN_PART_EVENTS = 64;                            // (swept at 16 / 64 / 256: profiles/mean_waveforms.json)
static const long MEAN_MAX_LABEL_EVENTS = 1l << 21;                 // of one label in a call: |sum| < 2^21 * 2^42

static long mean_part_events()
{
    const char *e = getenv("MTS_MEAN_PART_EVENTS");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (long)std::min<long long>(v, 1 << 20) : MEAN_PART_EVENTS;
}

static int mean_waveforms_run(Engine &E, hipStream_t st, const ChunkTable &T, const ZArgs &Z, long n_events, const long *ev_row, const int *ev_col0,
                              const int *ev_label, int n_labels, int before, int after, int width, double resolution, long long *out_sum,
                              int *out_count, long *out_skipped, bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const long vb = Z.vb, ve = Z.ve;
    const int n_cols = Z.n_cols;
    const SnipArgs A{n_events, ev_row, ev_col0, before, after, width};
    int rc;
    if ((rc = check_snippet_shape(T, Z, A))) return rc;
    const u64 n_item = (u64)((long)before + after) * width;
    if (n_labels < 1 || n_labels > MTS_MEAN_MAX_LABELS) { set_error("mean_waveforms: %d labels (1 .. %d)", n_labels, MTS_MEAN_MAX_LABELS); return MTS_E_ARG; }
    if ((u64)n_labels * n_item > (u64)MTS_MEAN_MAX_ENTRIES) {
        set_error("mean_waveforms: %d labels x %llu entries (<= %ld in all)", n_labels, (unsigned long long)n_item, (long)MTS_MEAN_MAX_ENTRIES); return MTS_E_ARG;
    }
    int expo = 0;
    if (!(resolution > 0) || !std::isfinite(resolution) || std::frexp(resolution, &expo) != 0.5 || expo - 1 < -60 || expo - 1 > 60) {
        set_error("mean_waveforms: resolution %g (a power of two in [2^-60, 2^60])", resolution); return MTS_E_ARG;
    }
    if (!out_sum || !out_count || !out_skipped) { set_error("mean_waveforms: no output buffers"); return MTS_E_ARG; }
    if (n_events && !ev_label) { set_error("mean_waveforms: no labels"); return MTS_E_ARG; }
    {
        std::vector<long> per((size_t)n_labels, 0);
        for (long e = 0; e < n_events; e++) {
            if (ev_label[e] < 0 || ev_label[e] >= n_labels) { set_error("mean_waveforms: event %ld: label %d outside [0, %d)", e, ev_label[e], n_labels); return MTS_E_ARG; }
            if (++per[(size_t)ev_label[e]] > MEAN_MAX_LABEL_EVENTS) {
                set_error("mean_waveforms: label %d has more than %ld events", ev_label[e], MEAN_MAX_LABEL_EVENTS); return MTS_E_ARG;
            }
        }
    }
    if ((rc = check_snippet_events(T, Z, A))) return rc;
    status_ok(T, status);
    const size_t n_sum = (size_t)n_labels * (size_t)n_item;
    if (n_events == 0) {                                           // zeros, and no gather
        if (out_on_host) { memset(out_sum, 0, 8 * n_sum); memset(out_count, 0, 4 * n_sum); memset(out_skipped, 0, 8 * (size_t)n_labels); return MTS_OK; }
        MTS_HIP(hipMemsetAsync(out_sum, 0, 8 * n_sum, st));
        MTS_HIP(hipMemsetAsync(out_count, 0, 4 * n_sum, st));
        MTS_HIP(hipMemsetAsync(out_skipped, 0, 8 * (size_t)n_labels, st));
        MTS_HIP(hipStreamSynchronize(st));
        return MTS_OK;
    }

    SnippetFeed S(T, out_on_host);
    HaloFeed &H = S.H;
    if ((rc = S.plan(E, Z, A))) return rc;
    // every slab's parts, one behind the other: slab k's are parts [part0[k], part0[k + 1]); the perms make one array of n_events
    std::vector<long> perm((size_t)n_events), part0 = {0};
    std::vector<MeanPart> parts;
    const long part_events = mean_part_events();
    for (const SnippetPlan &Sp : S.slabs)
        for (const SnippetSlab &B : Sp.slabs) {
            const MeanParts M(ev_label, B.e0, B.e1, part_events);
            std::copy(M.perm.begin(), M.perm.end(), perm.begin() + B.e0);
            parts.insert(parts.end(), M.parts.begin(), M.parts.end());
            part0.push_back((long)parts.size());
        }
    // ---- workspace
    WsLayout &L = H.L;
    ZStage F(Z, L);
    const size_t o_seg = L.take(H.table_bytes()), o_erow = L.take(8 * (u64)n_events), o_ecol = L.take(4 * (u64)n_events),
                 o_perm = L.take(8 * (u64)n_events), o_parts = L.take(sizeof(MeanPart) * (u64)parts.size()), o_y = L.take(4 * (u64)S.max_rows * n_cols),
                 o_sum = L.take_out(8 * (u64)n_sum), o_count = L.take_out(4 * (u64)n_sum), o_skip = L.take_out(8 * (u64)n_labels);
    StreamGuard G{st};
    if ((rc = H.place(E, st, E.wav, o_seg))) return rc;
    u8 *ws = E.wav.as<u8>();
    if ((rc = F.upload(st, ws))) return rc;
    MTS_HIP(hipMemcpyAsync(ws + o_erow, ev_row, 8 * (size_t)n_events, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_ecol, ev_col0, 4 * (size_t)n_events, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_perm, perm.data(), 8 * (size_t)n_events, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_parts, parts.data(), sizeof(MeanPart) * parts.size(), hipMemcpyHostToDevice, st));
    long long *d_sum = L.out(ws, o_sum, out_sum);
    int *d_count = L.out(ws, o_count, out_count);
    long *d_skip = L.out(ws, o_skip, out_skipped);
    MTS_HIP(hipMemsetAsync(d_sum, 0, 8 * n_sum, st));
    MTS_HIP(hipMemsetAsync(d_count, 0, 4 * n_sum, st));
    MTS_HIP(hipMemsetAsync(d_skip, 0, 8 * (size_t)n_labels, st));
    float *d_y = (float *)(ws + o_y);
    const MeanPart *d_parts = (const MeanPart *)(ws + o_parts);
    rc = S.run(E, st, T, F, d_y, status, [&](const SnippetSlab &B, long k) {
        return launch_mean_waveforms(st, d_y, B.a, B.b - B.a, n_cols, vb, ve, (const long *)(ws + o_erow), (const int *)(ws + o_ecol),
                                     (const long *)(ws + o_perm), d_parts + part0[(size_t)k], part0[(size_t)k + 1] - part0[(size_t)k], before, after,
                                     width, resolution, d_sum, d_count, d_skip);
    });
    if (rc) return rc;
    if (out_on_host) {
        MTS_HIP(hipMemcpyAsync(out_sum, d_sum, 8 * n_sum, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_count, d_count, 4 * n_sum, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_skipped, d_skip, 8 * (size_t)n_labels, hipMemcpyDeviceToHost, st));
    }
    if ((rc = G.wait())) return rc;
    S.done(E);
    return MTS_OK;
}

// ---- template scores (mts_correlate, mts_dev_correlate) ------------------------------------------------------------------------
// The unit is a row of [row_begin, row_end).  Piece p owns the rows in its chunks; their scores need z from `before` rows before to
// T - before - 1 rows after, and that the filter's support: the rows [u0, u1) read the file rows from u0 - before + half - (L - 1) to
// u1 + T - before - 1 + half, within the valid range.  A piece's rows go through the float32 workspace in slabs of owned rows that
// keep it (own + T - 1 rows) <= the slab bound: filter -> median -> k_correlate.  The templates are repacked once per call into the
// kernel's layout (correlate.hip: group-major, padded with zeros).  Every score is computed from the same rows in the same order
// whatever the pieces and slabs.
static const u64 CORRELATE_SLAB_BYTES = 256ull << 20;

// the templates (n_out, T, n_cols) in k_correlate's layout: row (g / 4 * T + tau) * 4 + c holds K[0 .. kp, tau, g + c], +0 past n_cols and n_out
static std::vector<float> repack_templates(const float *templates, int n_out, int n_tau, int n_cols, int kp)
{
    std::vector<float> h_tpl(align_up((u64)n_cols, 4) * n_tau * kp, 0.0f);
    for (int k = 0; k < n_out; k++)
        for (int tau = 0; tau < n_tau; tau++) {
            const float *src = templates + ((size_t)k * n_tau + tau) * n_cols;
            for (int j = 0; j < n_cols; j++) h_tpl[(((size_t)(j >> 2) * n_tau + tau) * 4 + (j & 3)) * kp + k] = src[j];
        }
    return h_tpl;
}

static int correlate_run(Engine &E, hipStream_t st, const ChunkTable &T, const ZArgs &Z, long row_begin, long row_end, int before, int n_tau,
                         int n_out, const float *templates, float *out, bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const long vb = Z.vb, ve = Z.ve;
    const int n_cols = Z.n_cols, n_taps = Z.n_taps;
    int rc;
    if ((rc = check_zargs(T, Z, MTS_CORRELATE_MAX_COLS))) return rc;
    if ((rc = check_templates("correlate", n_cols, before, n_tau, n_out, templates))) return rc;
    if (row_begin < vb || row_end < row_begin || row_end > ve || row_end - row_begin > (1l << 40)) { set_error("correlate: rows invalid"); return MTS_E_ARG; }
    if (row_end > row_begin && !out) { set_error("correlate: no output buffer"); return MTS_E_ARG; }
    if ((rc = check_columns(Z.cols, n_cols, T.nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    const long half = (n_taps - 1) / 2, n_units = row_end - row_begin, after = n_tau - before;
    // the rows that the scores of rows [u0, u1) read: (rows - before .. rows + after - 1)'s support ∩ valid range
    auto rows = [&](long u0, long u1, long *lo, long *hi) {
        *lo = std::max(vb, row_begin + u0 - before + half - (n_taps - 1)); *hi = std::min(ve, row_begin + u1 + after - 1 + half);
    };
    long need_lo = 0, need_hi = 0;
    if (n_units) rows(0, n_units, &need_lo, &need_hi);
    if ((rc = check_cover("correlate", T, need_lo, need_hi))) return rc;
    status_ok(T, status);
    if (!n_units) return MTS_OK;

    HaloFeed H(T, out_on_host);
    if ((rc = H.plan(n_units, [&](long r) { return r - row_begin; }, rows))) return rc;
    // rows a slab owns: the workspace holds them and their T - 1 neighbours
    const long cap_rows = (long)std::min<u64>(env_bytes("MTS_CORRELATE_SLAB_BYTES", CORRELATE_SLAB_BYTES) / (4 * (u64)n_cols), (u64)1 << 40);
    const long own = std::min(n_units, std::max(1l, cap_rows - (n_tau - 1)));
    // ---- workspace: taps, columns, segment tables, templates (group-major: row (g / 4 * T + tau) * 4 + c holds K[., tau, g + c], zeros
    // past n_cols and n_out), the filtered slab, the output
    const int n4 = (int)align_up((u64)n_cols, 4), kp = (int)align_up((u64)n_out, CORRELATE_PAD);
    const u64 tpl_items = (u64)n4 * n_tau * kp, n_items = (u64)n_units * n_out;
    WsLayout &L = H.L;
    ZStage F(Z, L);
    const size_t o_seg = L.take(H.table_bytes()), o_tpl = L.take(4 * tpl_items), o_y = L.take(4 * (u64)(own + n_tau - 1) * n_cols),
                 o_out = L.take_out(4 * n_items);
    const std::vector<float> h_tpl = repack_templates(templates, n_out, n_tau, n_cols, kp);
    StreamGuard G{st};
    if ((rc = H.place(E, st, E.cor, o_seg))) return rc;
    u8 *ws = E.cor.as<u8>();
    if ((rc = F.upload(st, ws))) return rc;
    MTS_HIP(hipMemcpyAsync(ws + o_tpl, h_tpl.data(), 4 * (size_t)tpl_items, hipMemcpyHostToDevice, st));
    float *d_out = L.out(ws, o_out, out);
    float *d_y = (float *)(ws + o_y);
    rc = H.run(E, st, status, [&](const FeedPiece &Pc, const PieceSegs &Sg) {
        const long p0 = row_begin + Pc.u0, p1 = row_begin + Pc.u1;
        int r = MTS_OK;
        for (long s0 = p0; !r && s0 < p1; s0 += own) {
            const long s1 = std::min(p1, s0 + own), a = std::max(vb, s0 - before), b = std::max(a, std::min(ve, s1 + after - 1));
            if (b > a) r = F.filter(st, T, Sg, a, b, d_y);
            if (!r) r = launch_correlate(st, d_y, a, b - a, n_cols, vb, ve, (const float *)(ws + o_tpl), kp, n_tau, before, n_out, s0, s1,
                                         d_out + (u64)(s0 - row_begin) * n_out);
        }
        return r;
    });
    if (rc) return rc;
    return dense_tail(G, out_on_host, out, d_out, n_items);
}

// ---- subtracted events (mts_residual, mts_match_residual and their device variants) ---------------------------------------------
// The list that both ops take: n_sub events (row, template, amplitude), non-decreasing in row.  Checked with the other arguments; on
// the device as (row, template, -amplitude), beside the plain (K, T, n_cols) templates that k_subtract reads -- both only when there
// is something to subtract.
static int check_sub_events(const char *op, long n_sub, const long *sub_row, const int *sub_tpl, const float *sub_amp, long vb, long ve, int n_out)
{
    if (n_sub < 0 || n_sub > (1l << 30)) { set_error("%s: %ld subtracted events (0 .. 2^30)", op, n_sub); return MTS_E_ARG; }
    if (n_sub && (!sub_row || !sub_tpl || !sub_amp)) { set_error("%s: no subtracted events given", op); return MTS_E_ARG; }
    for (long e = 0; e < n_sub; e++) {
        if (sub_row[e] < vb || sub_row[e] >= ve) { set_error("%s: subtracted event %ld at row %ld outside [%ld, %ld)", op, e, sub_row[e], vb, ve); return MTS_E_ARG; }
        if (e && sub_row[e] < sub_row[e - 1]) { set_error("%s: subtracted event %ld at row %ld follows one at row %ld (rows must not decrease)", op, e, sub_row[e], sub_row[e - 1]); return MTS_E_ARG; }
        if (sub_tpl[e] < 0 || sub_tpl[e] >= n_out) { set_error("%s: subtracted event %ld names template %d (%d templates)", op, e, sub_tpl[e], n_out); return MTS_E_ARG; }
        if (!std::isfinite(sub_amp[e])) { set_error("%s: the amplitude of subtracted event %ld is not finite", op, e); return MTS_E_ARG; }
    }
    return MTS_OK;
}

struct SubEvents {
    long n = 0;
    size_t o_row = 0, o_tpl = 0, o_namp = 0, o_plain = 0;
    std::vector<float> namp;                                  // (the source of an asynchronous copy: it lives as long as the call)
    const long *d_row = nullptr;
    const int *d_tpl = nullptr;
    const float *d_namp = nullptr, *d_plain = nullptr;

    // (no events: no bytes)
    void take(WsLayout &L, long n_sub, u64 tpl_items)
    {
        n = n_sub;
        o_row = L.take(8 * (u64)n); o_tpl = L.take(4 * (u64)n); o_namp = L.take(4 * (u64)n); o_plain = L.take(n ? 4 * tpl_items : 0);
    }
    int upload(hipStream_t st, u8 *ws, const long *sub_row, const int *sub_tpl, const float *sub_amp, const float *templates, u64 tpl_items)
    {
        if (!n) return MTS_OK;
        namp.resize((size_t)n);
        for (long e = 0; e < n; e++) namp[e] = -sub_amp[e];
        d_row = (const long *)(ws + o_row); d_tpl = (const int *)(ws + o_tpl); d_namp = (const float *)(ws + o_namp); d_plain = (const float *)(ws + o_plain);
        MTS_HIP(hipMemcpyAsync(ws + o_row, sub_row, 8 * (size_t)n, hipMemcpyHostToDevice, st));
        MTS_HIP(hipMemcpyAsync(ws + o_tpl, sub_tpl, 4 * (size_t)n, hipMemcpyHostToDevice, st));
        MTS_HIP(hipMemcpyAsync(ws + o_namp, namp.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
        MTS_HIP(hipMemcpyAsync(ws + o_plain, templates, 4 * (size_t)tpl_items, hipMemcpyHostToDevice, st));
        return MTS_OK;
    }
};

// ---- residual (mts_residual, mts_dev_residual) ---------------------------------------------------------------------------------
// The unit is a row of [row_begin, row_end) and the halo is the filter's support alone: the rows [u0, u1) read the file rows from u0 +
// half - (L - 1) to u1 + half, within the valid range -- decimate with q = 1.  A piece's rows go through the float32 workspace in
// slabs of owned rows with no neighbours: filter -> median -> k_subtract, which writes the slab's rows of the output (a NaN as
// 0x7fc00000, with an empty list too).  The subtraction reads no row of the recording: whatever the pieces and slabs, every entry is
// the same chain over the same events.
static const u64 RESIDUAL_SLAB_BYTES = 256ull << 20;

static int residual_run(Engine &E, hipStream_t st, const ChunkTable &T, const ZArgs &Z, long row_begin, long row_end, int before, int n_tau,
                        int n_out, const float *templates, long n_sub, const long *sub_row, const int *sub_tpl, const float *sub_amp, float *out,
                        bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const long vb = Z.vb, ve = Z.ve;
    const int n_cols = Z.n_cols, n_taps = Z.n_taps;
    int rc;
    if ((rc = check_zargs(T, Z, MTS_CORRELATE_MAX_COLS))) return rc;
    if ((rc = check_templates("residual", n_cols, before, n_tau, n_out, templates))) return rc;
    if (row_begin < vb || row_end < row_begin || row_end > ve || row_end - row_begin > (1l << 40)) { set_error("residual: rows invalid"); return MTS_E_ARG; }
    if ((rc = check_sub_events("residual", n_sub, sub_row, sub_tpl, sub_amp, vb, ve, n_out))) return rc;
    if (row_end > row_begin && !out) { set_error("residual: no output buffer"); return MTS_E_ARG; }
    if ((rc = check_columns(Z.cols, n_cols, T.nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    const long half = (n_taps - 1) / 2, n_units = row_end - row_begin;
    // the rows that the rows [u0, u1) read: their filter support ∩ valid range
    auto rows = [&](long u0, long u1, long *lo, long *hi) {
        *lo = std::max(vb, row_begin + u0 + half - (n_taps - 1)); *hi = std::min(ve, row_begin + u1 + half);
    };
    long need_lo = 0, need_hi = 0;
    if (n_units) rows(0, n_units, &need_lo, &need_hi);
    if ((rc = check_cover("residual", T, need_lo, need_hi))) return rc;
    status_ok(T, status);
    if (!n_units) return MTS_OK;

    HaloFeed H(T, out_on_host);
    if ((rc = H.plan(n_units, [&](long r) { return r - row_begin; }, rows))) return rc;
    // rows a slab owns: the workspace holds them and nothing else
    const u64 cap_rows = std::min<u64>(env_bytes("MTS_RESIDUAL_SLAB_BYTES", RESIDUAL_SLAB_BYTES) / (4 * (u64)n_cols), (u64)1 << 40);
    const long own = std::min(n_units, std::max(1l, (long)cap_rows));
    // ---- workspace: taps, columns, segment tables, the events, the plain templates, the filtered slab, the output
    const u64 tpl_items = (u64)n_out * n_tau * n_cols, n_items = (u64)n_units * n_cols;
    WsLayout &L = H.L;
    ZStage F(Z, L);
    const size_t o_seg = L.take(H.table_bytes());
    SubEvents SE;
    SE.take(L, n_sub, tpl_items);
    const size_t o_y = L.take(4 * (u64)own * n_cols), o_out = L.take_out(4 * n_items);
    StreamGuard G{st};
    if ((rc = H.place(E, st, E.res, o_seg))) return rc;
    u8 *ws = E.res.as<u8>();
    if ((rc = F.upload(st, ws))) return rc;
    if ((rc = SE.upload(st, ws, sub_row, sub_tpl, sub_amp, templates, tpl_items))) return rc;
    float *d_out = L.out(ws, o_out, out);
    float *d_y = (float *)(ws + o_y);
    rc = H.run(E, st, status, [&](const FeedPiece &Pc, const PieceSegs &Sg) {
        const long p0 = row_begin + Pc.u0, p1 = row_begin + Pc.u1;
        int r = MTS_OK;
        for (long s0 = p0; !r && s0 < p1; s0 += own) {
            const long s1 = std::min(p1, s0 + own);
            r = F.filter(st, T, Sg, s0, s1, d_y);
            if (!r) r = launch_subtract(st, d_y, s0, s1 - s0, n_cols, SE.d_row, SE.d_tpl, SE.d_namp, SE.n, SE.d_plain, n_tau, before,
                                        d_out + (u64)(s0 - row_begin) * n_cols);
        }
        return r;
    });
    if (rc) return rc;
    return dense_tail(G, out_on_host, out, d_out, n_items);
}

// ---- one round of a radix select over the filtered signal (mts_filtered_rank_hist, mts_dev_filtered_rank_hist) -----------------
// The unit is a row of the count range [count_begin, count_end), a part of the window grid (row_begin, row_end, window_rows).  Piece p
// owns the rows in its chunks; they read their filter support and nothing else (no exclusion radius: a slab is the rows it owns).  A
// piece's rows go through the float32 workspace in slabs (filter -> median -> k_zrank_hist on the stream).  The histograms, kmin and
// kmax are zeroed / initialised once per call, accumulated with integer atomics across slabs and pieces on the device and copied out
// once: the same bytes whatever the pieces and slabs.  The items are float32, so the keys have 32 bits in mode 0.
static const u64 ZRANK_SLAB_BYTES = 256ull << 20;

static int filtered_rank_hist_run(Engine &E, hipStream_t st, const ChunkTable &T, const ZArgs &Z, long row_begin, long row_end, long window_rows,
                                  long count_begin, long count_end, int mode, const double *center, const unsigned long long *sel_prefix,
                                  const int *sel_shift, unsigned int *o_hist, unsigned long long *o_kmin, unsigned long long *o_kmax,
                                  bool out_on_host, long *count, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const long vb = Z.vb, ve = Z.ve;
    const int n_cols = Z.n_cols, n_taps = Z.n_taps;
    int rc;
    if ((rc = check_zargs(T, Z))) return rc;
    if (window_rows < 1) { set_error("window_rows %ld < 1", window_rows); return MTS_E_ARG; }
    if (row_begin < vb || row_end < row_begin || row_end > ve) { set_error("filtered rank hist: rows invalid"); return MTS_E_ARG; }
    if (count_begin < row_begin || count_end < count_begin || count_end > row_end) {
        set_error("filtered rank hist: count range [%ld, %ld) outside the grid [%ld, %ld)", count_begin, count_end, row_begin, row_end); return MTS_E_ARG;
    }
    if (mode < 0 || mode > 2) { set_error("filtered rank hist: mode %d (0, 1 or 2)", mode); return MTS_E_ARG; }
    const long span = row_end - row_begin;
    if ((window_rows < span ? window_rows : span) >= (1l << 32)) { set_error("windows of 2^32 rows or more"); return MTS_E_ARG; }
    const long n_win = (span + window_rows - 1) / window_rows;
    if (n_win && (!o_hist || !o_kmin || !o_kmax || !count || !sel_prefix || !sel_shift || (mode && !center))) {
        set_error("filtered rank hist: selectors, center or outputs missing"); return MTS_E_ARG;
    }
    const int key_bits = mode ? 64 : 32;                     // (a float32 item)
    const u64 n_sel = (u64)n_win * MTS_RANK_SELECTORS * n_cols;
    for (u64 e = 0; e < n_sel; e++) {
        const int sh = sel_shift[e];
        if (sh < 0) continue;
        const int above = key_bits - sh - MTS_RANK_BITS;     // bits of the key above the digit
        if (above < 0) { set_error("filtered rank hist: shift %d above key_bits - %d", sh, MTS_RANK_BITS); return MTS_E_ARG; }
        if (above < 64 && (sel_prefix[e] >> above)) { set_error("filtered rank hist: a prefix of more than %d bits at shift %d", above, sh); return MTS_E_ARG; }
    }
    if ((rc = check_columns(Z.cols, n_cols, T.nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    const long half = (n_taps - 1) / 2, n_units = count_end - count_begin;
    // the rows that the rows [u0, u1) read: their filter support ∩ valid range
    auto rows = [&](long u0, long u1, long *lo, long *hi) {
        *lo = std::max(vb, count_begin + u0 + half - (n_taps - 1)); *hi = std::min(ve, count_begin + u1 + half);
    };
    long need_lo = 0, need_hi = 0;
    if (n_units) rows(0, n_units, &need_lo, &need_hi);
    if ((rc = check_cover("filtered rank hist", T, need_lo, need_hi))) return rc;
    status_ok(T, status);
    for (long w = 0; w < n_win; w++) count[w] = 0;
    if (!n_win) return MTS_OK;
    const u64 n_cells = (u64)n_win * n_cols, hist_bytes = n_sel * (4ull << MTS_RANK_BITS), k_bytes = n_sel * 8;
    if (!n_units) {                                          // nothing to count: the identities
        if (out_on_host) { memset(o_hist, 0, (size_t)hist_bytes); memset(o_kmin, 0xff, (size_t)k_bytes); memset(o_kmax, 0, (size_t)k_bytes); return MTS_OK; }
        MTS_HIP(hipMemsetAsync(o_hist, 0, (size_t)hist_bytes, st));
        MTS_HIP(hipMemsetAsync(o_kmin, 0xff, (size_t)k_bytes, st));
        MTS_HIP(hipMemsetAsync(o_kmax, 0, (size_t)k_bytes, st));
        MTS_HIP(hipStreamSynchronize(st));
        return MTS_OK;
    }

    HaloFeed H(T, out_on_host);
    if ((rc = H.plan(n_units, [&](long r) { return r - count_begin; }, rows))) return rc;
    // rows a slab owns: the workspace holds them and nothing else
    const u64 cap_rows = std::min<u64>(env_bytes("MTS_ZRANK_SLAB_BYTES", ZRANK_SLAB_BYTES) / (4 * (u64)n_cols), (u64)1 << 40);
    const long own = std::min(n_units, std::max(1l, (long)cap_rows));
    const long block_rows = (long)std::min<u64>(env_bytes("MTS_ZRANK_BLOCK_ROWS", (u64)ZSEL_BLOCK_ROWS), (u64)1 << 40);      // (the bench sweeps it)
    // ---- workspace: taps, columns, segment tables, centers, selectors, the filtered slab, the outputs
    WsLayout &L = H.L;
    ZStage F(Z, L);
    const size_t o_seg = L.take(H.table_bytes()), o_cen = L.take(mode ? 8 * n_cells : 0), o_pre = L.take(k_bytes), o_shf = L.take(n_sel * 4),
                 o_y = L.take(4 * (u64)own * n_cols), w_hist = L.take_out(hist_bytes), w_kmin = L.take_out(k_bytes), w_kmax = L.take_out(k_bytes);
    StreamGuard G{st};
    if ((rc = H.place(E, st, E.zrank, o_seg))) return rc;
    u8 *ws = E.zrank.as<u8>();
    if ((rc = F.upload(st, ws))) return rc;
    double *d_cen = (double *)(ws + o_cen);
    u64 *d_pre = (u64 *)(ws + o_pre);
    int *d_shf = (int *)(ws + o_shf);
    float *d_y = (float *)(ws + o_y);
    u32 *d_hist = L.out(ws, w_hist, (u32 *)o_hist);
    u64 *d_kmin = L.out(ws, w_kmin, (u64 *)o_kmin), *d_kmax = L.out(ws, w_kmax, (u64 *)o_kmax);
    if (mode) MTS_HIP(hipMemcpyAsync(d_cen, center, 8 * (size_t)n_cells, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_pre, sel_prefix, (size_t)k_bytes, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_shf, sel_shift, 4 * (size_t)n_sel, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemsetAsync(d_hist, 0, (size_t)hist_bytes, st));
    MTS_HIP(hipMemsetAsync(d_kmin, 0xff, (size_t)k_bytes, st));
    MTS_HIP(hipMemsetAsync(d_kmax, 0, (size_t)k_bytes, st));
    rc = H.run(E, st, status, [&](const FeedPiece &Pc, const PieceSegs &Sg) {
        const long p0 = count_begin + Pc.u0, p1 = count_begin + Pc.u1;
        int r = MTS_OK;
        for (long s0 = p0; !r && s0 < p1; s0 += own) {
            const long s1 = std::min(p1, s0 + own);
            r = F.filter(st, T, Sg, s0, s1, d_y);
            if (!r) r = launch_zrank_hist(st, mode, d_y, s0, s1, block_rows, n_cols, row_begin, window_rows, d_cen, d_pre, d_shf, d_hist, d_kmin, d_kmax);
        }
        return r;
    });
    if (rc) return rc;
    if (out_on_host) {                                        // the histograms, and nothing else, cross the bus
        MTS_HIP(hipMemcpyAsync(o_hist, d_hist, (size_t)hist_bytes, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_kmin, d_kmin, (size_t)k_bytes, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_kmax, d_kmax, (size_t)k_bytes, hipMemcpyDeviceToHost, st));
    }
    if ((rc = G.wait())) return rc;
    for (long w = (count_begin - row_begin) / window_rows; w < n_win && row_begin + w * window_rows < count_end; w++)      // (after the last wait)
        count[w] = std::min(count_end, row_begin + std::min(span, (w + 1) * window_rows)) - std::max(count_begin, row_begin + w * window_rows);
    return MTS_OK;
}

// ---- template events (mts_match_templates, mts_dev_match_templates) ------------------------------------------------------------
// The unit is a row of [row_begin, row_end).  Piece p owns the rows in its chunks; their events need the scores R rows either side,
// those z from `before` rows before to T - before - 1 rows after, and that the filter's support: the rows [u0, u1) read the file rows
// from u0 - R - before + half - (L - 1) to u1 + R + T - before - 1 + half, within the valid range.  A piece's rows go through slabs of
// owned rows [s0, s1): the scores of [sa, sb) = [max(vb, s0 - R), min(ve, s1 + R)) from z of [max(vb, sa - before), min(ve, sb + after
// - 1)) -- filter -> median -> k_correlate into the score slab -> row maxima -> mask -> count / scan / emit, all on the stream; the
// write position is carried on the device from slab to slab and piece to piece.  `own` keeps both the z slab and the score slab within
// the slab bound, and is never less than one row with its neighbours.  launch_decimate, launch_row_median and launch_correlate are
// correlate_run's, so every score has correlate's bits whatever the pieces and slabs.  With subtracted events (mts_match_residual, n_sub
// > 0) k_subtract works in place on the z slab between the median and k_correlate; without them nothing differs.
static const u64 TMATCH_SLAB_BYTES = 256ull << 20;
static const long TMATCH_SLAB_MAX_ROWS = 1l << 22;                  // (bounds the row maxima and the bitmap of a call with few templates)

static int tmatch_run(Engine &E, hipStream_t st, const ChunkTable &T, const ZArgs &Z, long row_begin, long row_end, int before, int n_tau, int n_out,
                      const float *templates, const float *threshold, int R, long max_events, long *out_row, int *out_tpl, float *out_score,
                      bool out_on_host, long *n_events, int *status, long n_sub = 0, const long *sub_row = nullptr, const int *sub_tpl = nullptr,
                      const float *sub_amp = nullptr)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const long vb = Z.vb, ve = Z.ve;
    const int n_cols = Z.n_cols, n_taps = Z.n_taps;
    int rc;
    if ((rc = check_zargs(T, Z, MTS_CORRELATE_MAX_COLS))) return rc;
    if ((rc = check_templates("match_templates", n_cols, before, n_tau, n_out, templates))) return rc;
    if (!threshold) { set_error("match_templates: no thresholds"); return MTS_E_ARG; }
    for (int k = 0; k < n_out; k++)
        if (!std::isfinite(threshold[k])) { set_error("match_templates: threshold %d is not finite", k); return MTS_E_ARG; }
    if (R < 0 || R > MTS_TMATCH_MAX_EXCLUDE) { set_error("match_templates: exclude_rows %d (0 .. %d)", R, MTS_TMATCH_MAX_EXCLUDE); return MTS_E_ARG; }
    if (row_begin < vb || row_end < row_begin || row_end > ve) { set_error("match_templates: rows invalid"); return MTS_E_ARG; }
    if (max_events < 0 || max_events > (1l << 40) || !n_events) { set_error("match_templates: max_events invalid or no n_events"); return MTS_E_ARG; }
    if (max_events && (!out_row || !out_tpl || !out_score)) { set_error("match_templates: no output buffers"); return MTS_E_ARG; }
    if ((rc = check_sub_events("match_templates", n_sub, sub_row, sub_tpl, sub_amp, vb, ve, n_out))) return rc;
    if ((rc = check_columns(Z.cols, n_cols, T.nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    const long half = (n_taps - 1) / 2, n_units = row_end - row_begin, after = n_tau - before;
    // the rows that the events of rows [u0, u1) read: ((rows + R either side) - before .. + after - 1)'s support ∩ valid range
    auto rows = [&](long u0, long u1, long *lo, long *hi) {
        *lo = std::max(vb, row_begin + u0 - R - before + half - (n_taps - 1)); *hi = std::min(ve, row_begin + u1 + R + after - 1 + half);
    };
    long need_lo = 0, need_hi = 0;
    if (n_units) rows(0, n_units, &need_lo, &need_hi);
    if ((rc = check_cover("match_templates", T, need_lo, need_hi))) return rc;
    status_ok(T, status);
    *n_events = 0;
    if (!n_units) return MTS_OK;

    HaloFeed H(T, out_on_host);
    if ((rc = H.plan(n_units, [&](long r) { return r - row_begin; }, rows))) return rc;
    // rows a slab owns: the z slab holds them, R either side and their T - 1 neighbours; the score slab them and R either side (reduce_plan.h)
    const TmatchSlabs SL(n_units, R, before, n_tau, vb, ve, n_cols, n_out, env_bytes("MTS_TMATCH_SLAB_BYTES", TMATCH_SLAB_BYTES), TMATCH_SLAB_MAX_ROWS);
    const long own = SL.own, sc_rows = SL.sc_rows, z_rows = SL.z_rows;
    const long max_words = tmatch_bitmap_words(own), max_blocks = detect_blocks(max_words);
    // ---- workspace
    const int n4 = (int)align_up((u64)n_cols, 4), kp = (int)align_up((u64)n_out, CORRELATE_PAD);
    const u64 tpl_items = (u64)n4 * n_tau * kp, plain_items = (u64)n_out * n_tau * n_cols;
    WsLayout &L = H.L;
    ZStage F(Z, L);
    const size_t o_thr = L.take(4 * (u64)n_out), o_seg = L.take(H.table_bytes());
    EventTail EV(L);
    const size_t o_tpl = L.take(4 * tpl_items), o_y = L.take(4 * (u64)z_rows * n_cols), o_sc = L.take(4 * (u64)sc_rows * n_out),
                 o_best = L.take(4 * (u64)sc_rows), o_arg = L.take(4 * (u64)sc_rows), o_bits = L.take(8 * (u64)max_words),
                 o_cnt = L.take(4 * (u64)max_blocks), o_offs = L.take(8 * (u64)max_blocks), o_row = L.take_out(8 * (u64)max_events),
                 o_k = L.take_out(4 * (u64)max_events), o_val = L.take_out(4 * (u64)max_events);
    SubEvents SE;
    SE.take(L, n_sub, plain_items);
    const std::vector<float> h_tpl = repack_templates(templates, n_out, n_tau, n_cols, kp);
    StreamGuard G{st};
    if ((rc = H.place(E, st, E.tm, o_seg))) return rc;
    u8 *ws = E.tm.as<u8>();
    if ((rc = F.upload(st, ws))) return rc;
    MTS_HIP(hipMemcpyAsync(ws + o_thr, threshold, 4 * (size_t)n_out, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_tpl, h_tpl.data(), 4 * (size_t)tpl_items, hipMemcpyHostToDevice, st));
    if ((rc = EV.begin(st, ws))) return rc;
    if ((rc = SE.upload(st, ws, sub_row, sub_tpl, sub_amp, templates, plain_items))) return rc;
    long *d_row = L.out(ws, o_row, out_row);
    int *d_k = L.out(ws, o_k, out_tpl);
    float *d_val = L.out(ws, o_val, out_score);
    float *d_y = (float *)(ws + o_y), *d_sc = (float *)(ws + o_sc), *d_best = (float *)(ws + o_best);
    int *d_arg = (int *)(ws + o_arg);
    u64 *d_bits = (u64 *)(ws + o_bits);
    rc = H.run(E, st, status, [&](const FeedPiece &Pc, const PieceSegs &Sg) {
        const long p0 = row_begin + Pc.u0, p1 = row_begin + Pc.u1;
        int r = MTS_OK;
        for (long s0 = p0; !r && s0 < p1; s0 += own) {
            const TmatchSlab S = SL.at(s0, p1);
            const long s1 = S.s1, sa = S.sa, sb = S.sb, a = S.a, b = S.b;
            if (b > a) r = F.filter(st, T, Sg, a, b, d_y);
            if (!r && SE.n && b > a) r = launch_subtract(st, d_y, a, b - a, n_cols, SE.d_row, SE.d_tpl, SE.d_namp, SE.n, SE.d_plain, n_tau, before, d_y);
            if (!r) r = launch_correlate(st, d_y, a, b - a, n_cols, vb, ve, (const float *)(ws + o_tpl), kp, n_tau, before, n_out, sa, sb, d_sc);
            if (!r) r = launch_tmatch_best(st, d_sc, sb - sa, n_out, d_best, d_arg);
            if (!r) r = launch_tmatch_mask(st, d_best, d_arg, sa, sb - sa, (const float *)(ws + o_thr), R, s0, s1, d_bits);
            if (!r) r = launch_tmatch_emit(st, d_bits, tmatch_bitmap_words(s1 - s0), (u32 *)(ws + o_cnt), (u64 *)(ws + o_offs), EV.d_total, d_best, d_arg,
                                           sa, s0, max_events, d_row, d_k, d_val);
        }
        return r;
    });
    if (rc) return rc;
    return EV.finish(G, max_events, out_on_host, n_events, out_row, d_row, out_tpl, d_k, out_score, d_val);
}

// ---- Welch PSD (mts_welch, mts_dev_welch) ------------------------------------------------------------------------------------
// The call's segments are cut into blocks of B (WELCH_BLOCK_SEGMENTS) and groups of G; the unit is a block.  Piece p owns the blocks
// whose first row lies in its chunks.  A piece's blocks are launched in runs that keep the partial slab <= WELCH_SLAB_BYTES, each
// followed by the combine that adds them to their groups' sums in block order: every group sum is the same sequence of additions
// whatever the pieces and runs.
static const u64 WELCH_SLAB_BYTES = 256ull << 20;

// exp(-2 pi i q / n) for q < n: the first octant in extended precision, the rest by exact symmetries (q = 0 gives exactly 1)
static void welch_twiddle(long q, long n, long double *re, long double *im)
{
    const long n4 = n / 4, quad = q / n4;
    long r = q % n4;
    const bool flip = 2 * r > n4;                                // cos(pi/2 - a) = sin(a)
    if (flip) r = n4 - r;
    const long double a = 2.0L * 3.14159265358979323846264338327950288L * (long double)r / (long double)n;
    long double c = r ? cosl(a) : 1.0L, s = r ? sinl(a) : 0.0L;
    if (flip) std::swap(c, s);
    long double cr, sr;                                          // cos, sin of the whole angle
    switch (quad) {
    case 0: cr = c; sr = s; break;
    case 1: cr = -s; sr = c; break;
    case 2: cr = -c; sr = -s; break;
    default: cr = s; sr = -c; break;
    }
    *re = cr; *im = -sr;
}

static int welch_run(Engine &E, hipStream_t st, const ChunkTable &T, long row_seg0, long seg_begin, long seg_end, int nperseg, long step,
                     const double *taper, int detrend, int csize, int n_cols, const int *cols, double *out, bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const int nc = T.nc, sz = T.sz, flags = T.flags;
    int rc;
    if (nc <= 0 || T.n_chunks < 0 || n_cols < 1 || n_cols > (1 << 24) || !cols) { set_error("welch: n_channels, n_chunks or columns invalid"); return MTS_E_ARG; }
    if (nperseg < 16 || nperseg > MTS_WELCH_MAX_NPERSEG || (nperseg & (nperseg - 1))) {
        set_error("welch: nperseg %d is not a power of two in [16, %d]", nperseg, MTS_WELCH_MAX_NPERSEG); return MTS_E_ARG;
    }
    if (step < 1 || step > nperseg) { set_error("welch: step %ld outside [1, %d]", step, nperseg); return MTS_E_ARG; }
    if (!taper) { set_error("welch: no taper"); return MTS_E_ARG; }
    for (int j = 0; j < nperseg; j++)
        if (!std::isfinite(taper[j])) { set_error("welch: taper value %d is not finite", j); return MTS_E_ARG; }
    if (csize != 4 && csize != 8) { set_error("welch: compute itemsize %d (4 or 8)", csize); return MTS_E_ARG; }
    const long B = WELCH_BLOCK_SEGMENTS, GR = WELCH_GROUP_ROWS;
    const long G = B * ((GR + step * B - 1) / (step * B));         // segments per group
    if (seg_begin < 0 || seg_end <= seg_begin || seg_end - seg_begin > (1l << 40) || seg_begin % G || row_seg0 < 0 || row_seg0 > (1l << 60)) {
        set_error("welch: segments [%ld, %ld) invalid or not aligned to groups of %ld", seg_begin, seg_end, G); return MTS_E_ARG;
    }
    if (!out) { set_error("welch: no output buffer"); return MTS_E_ARG; }
    if ((rc = check_columns(cols, n_cols, nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    const long n_seg = seg_end - seg_begin, n_blocks = (n_seg + B - 1) / B, GB = G / B, n_groups = (n_seg + G - 1) / G;
    // the rows that blocks [u0, u1) (call-local) read
    auto rows = [&](long u0, long u1, long *lo, long *hi) {
        *lo = row_seg0 + (seg_begin + u0 * B) * step; *hi = row_seg0 + (std::min(seg_end, seg_begin + u1 * B) - 1) * step + nperseg;
    };
    long need_lo, need_hi;
    rows(0, n_blocks, &need_lo, &need_hi);
    if ((rc = check_cover("welch", T, need_lo, need_hi))) return rc;
    status_ok(T, status);
    int log2n = 0;
    while ((1 << log2n) < nperseg) log2n++;
    const long b_first = seg_begin / B;                              // the call's block 0 (absolute)
    const long n_elems = (long)(nperseg / 2 + 1) * n_cols;

    HaloFeed H(T, out_on_host);
    // the first block whose first row is at or after row r
    const long block_rows = step * B, row_b0 = row_seg0 + seg_begin * step; // first row of call block 0
    if ((rc = H.plan(n_blocks, [&](long r) { return r <= row_b0 ? 0 : (r - row_b0 + block_rows - 1) / block_rows; }, rows))) return rc;
    // blocks per launch: the slab of partials stays <= WELCH_SLAB_BYTES (at least one block)
    const u64 blk_bytes = 8 * (u64)n_elems;
    long run_blocks = (long)std::max<u64>(1, WELCH_SLAB_BYTES / blk_bytes);
    run_blocks = std::min(run_blocks, std::min(n_blocks, 65535l));
    // ---- workspace
    WsLayout &L = H.L;
    const size_t o_taper = L.take((u64)csize * nperseg), o_tw = L.take(2 * (u64)csize * nperseg), o_cols = L.take(4 * (u64)n_cols),
                 o_seg = L.take(H.table_bytes()), o_part = L.take(blk_bytes * run_blocks), o_acc = L.take_out(8 * (u64)n_groups * n_elems);
    if ((rc = H.place(E, st, E.welch, o_seg))) return rc;
    u8 *ws = E.welch.as<u8>();
    // taper and twiddles, rounded once to the compute type
    std::vector<u8> h_tt((size_t)csize * 3 * nperseg);
    for (int j = 0; j < nperseg; j++) {
        long double re, im;
        welch_twiddle(j, nperseg, &re, &im);
        if (csize == 4) {
            const float w = (float)taper[j], tr = (float)re, ti = (float)im;
            memcpy(h_tt.data() + 4 * j, &w, 4);
            memcpy(h_tt.data() + 4 * nperseg + 8 * j, &tr, 4);
            memcpy(h_tt.data() + 4 * nperseg + 8 * j + 4, &ti, 4);
        } else {
            const double tr = (double)re, ti = (double)im;
            memcpy(h_tt.data() + 8 * j, &taper[j], 8);
            memcpy(h_tt.data() + 8 * nperseg + 16 * j, &tr, 8);
            memcpy(h_tt.data() + 8 * nperseg + 16 * j + 8, &ti, 8);
        }
    }
    MTS_HIP(hipMemcpyAsync(ws + o_taper, h_tt.data(), (size_t)csize * nperseg, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_tw, h_tt.data() + (size_t)csize * nperseg, 2 * (size_t)csize * nperseg, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    double *d_acc = L.out(ws, o_acc, out);
    MTS_HIP(hipMemsetAsync(d_acc, 0, 8 * (size_t)n_groups * n_elems, st));
    double *d_part = (double *)(ws + o_part);
    rc = H.run(E, st, status, [&](const FeedPiece &Pc, const PieceSegs &S) {
        int r = MTS_OK;
        for (long lb = Pc.u0; !r && lb < Pc.u1; lb += run_blocks) {
            const long lb1 = std::min(Pc.u1, lb + run_blocks);
            r = launch_welch(st, sz, flags, csize, log2n, S.base, S.row0, S.ns, nc, (const int *)(ws + o_cols), n_cols, ws + o_taper, ws + o_tw, row_seg0,
                             step, seg_end, b_first + lb, lb1 - lb, detrend ? 1 : 0, d_part);
            if (!r) r = launch_welch_combine(st, d_part, lb, lb1, GB, n_elems, d_acc);
        }
        return r;
    });
    if (rc) return rc;
    if (out_on_host) MTS_HIP(hipMemcpyAsync(out, d_acc, 8 * (size_t)n_groups * n_elems, hipMemcpyDeviceToHost, st));
    MTS_HIP(hipStreamSynchronize(st));
    return MTS_OK;
}

// ---- Gram matrices (mts_gram, mts_dev_gram) ----------------------------------------------------------------------------------
// The call's groups are cut into slabs of GRAM_SLAB_ROWS rows; the unit is a group.  Piece p owns the groups whose first row lies in
// its chunks.  A piece's slabs are launched in runs that keep the partial slab <= GRAM_SLAB_BYTES, each followed by the combine that
// adds them to their groups' accumulators in slab order: every group sum is the same sequence of additions whatever the pieces and runs.
static const u64 GRAM_SLAB_BYTES = 256ull << 20;

static int gram_run(Engine &E, hipStream_t st, const ChunkTable &T, long range_begin, long range_end, long window_rows, long group_begin,
                    long group_end, int n_cols, const int *cols, void *out_gram, void *out_sum, bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const int nc = T.nc, sz = T.sz, flags = T.flags;
    int rc;
    if (nc <= 0 || T.n_chunks < 0 || n_cols < 1 || n_cols > MTS_GRAM_MAX_COLS || !cols) {
        set_error("gram: n_channels, n_chunks or columns invalid (1 <= n_cols <= %d)", MTS_GRAM_MAX_COLS); return MTS_E_ARG;
    }
    if (window_rows < 1) { set_error("gram: window_rows %ld < 1", window_rows); return MTS_E_ARG; }
    if (range_begin < 0 || range_end <= range_begin || range_end > (1l << 60)) { set_error("gram: range [%ld, %ld) invalid", range_begin, range_end); return MTS_E_ARG; }
    const long GR = GRAM_GROUP_ROWS, SR = GRAM_SLAB_ROWS;
    const long K = (window_rows + GR - 1) / GR;                   // groups per whole window
    const long n_range = range_end - range_begin, n_full = n_range / window_rows, tail = n_range % window_rows;
    const long total_groups = n_full * K + (tail + GR - 1) / GR;
    if (group_begin < 0 || group_end <= group_begin || group_end > total_groups) {
        set_error("gram: groups [%ld, %ld) empty or outside the %ld groups of the range", group_begin, group_end, total_groups); return MTS_E_ARG;
    }
    if (!out_gram || !out_sum) { set_error("gram: no output buffer"); return MTS_E_ARG; }
    if ((rc = check_columns(cols, n_cols, nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    // the groups' rows: group g -> [grow[g], grow_end(g))
    const long n_groups = group_end - group_begin;
    if (n_groups > (1l << 31)) { set_error("gram: too many groups in one call"); return MTS_E_ARG; }
    auto group_rows = [&](long g, long *lo, long *hi) {
        const long w = g / K, k = g % K, w0 = range_begin + w * window_rows;
        const long w1 = std::min(w0 + window_rows, range_end);
        *lo = w0 + k * GR;
        *hi = std::min(*lo + GR, w1);
    };
    // the rows that groups [u0, u1) (call-local) read
    auto rows = [&](long u0, long u1, long *lo, long *hi) {
        long tmp;
        group_rows(group_begin + u0, lo, &tmp);
        group_rows(group_begin + u1 - 1, &tmp, hi);
    };
    long need_lo, need_hi;
    rows(0, n_groups, &need_lo, &need_hi);
    if ((rc = check_cover("gram", T, need_lo, need_hi))) return rc;
    status_ok(T, status);
    // slabs of the call: slab_rows (2 per slab), gfirst[g] the first slab of call group g
    std::vector<long> gfirst(n_groups + 1, 0), glo(n_groups), slab_rows;
    for (long g = 0; g < n_groups; g++) {
        long hi;
        group_rows(group_begin + g, &glo[g], &hi);
        gfirst[g] = (long)slab_rows.size() / 2;
        for (long r = glo[g]; r < hi; r += SR) { slab_rows.push_back(r); slab_rows.push_back(std::min(r + SR, hi)); }
    }
    const long n_slabs = gfirst[n_groups] = (long)slab_rows.size() / 2;

    HaloFeed H(T, out_on_host);
    // the first group whose first row is at or after row r
    if ((rc = H.plan(n_groups, [&](long r) { return std::lower_bound(glo.begin(), glo.end(), r) - glo.begin(); }, rows))) return rc;
    // slabs per launch: the partials stay <= GRAM_SLAB_BYTES (at least one slab)
    const u64 slab_bytes = (u64)gram_slab_bytes(n_cols);
    long run_slabs = (long)std::max<u64>(1, GRAM_SLAB_BYTES / slab_bytes);
    run_slabs = std::min(run_slabs, std::min(n_slabs, 65535l));
    const u64 nn = (u64)n_cols * n_cols;
    // ---- workspace
    WsLayout &L = H.L;
    const size_t o_cols = L.take(4 * (u64)n_cols), o_slab = L.take(16 * (u64)n_slabs), o_gf = L.take(8 * (u64)(n_groups + 1)), o_seg = L.take(H.table_bytes()),
                 o_part = L.take((u64)run_slabs * gram_pairs(n_cols) * 64 * 64 * 8), o_psum = L.take((u64)run_slabs * 8 * n_cols),
                 o_acc = L.take_out(8 * (u64)n_groups * nn), o_accs = L.take_out(8 * (u64)n_groups * n_cols);
    if ((rc = H.place(E, st, E.gram, o_seg))) return rc;
    u8 *ws = E.gram.as<u8>();
    MTS_HIP(hipMemcpyAsync(ws + o_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_slab, slab_rows.data(), 16 * (size_t)n_slabs, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_gf, gfirst.data(), 8 * (size_t)(n_groups + 1), hipMemcpyHostToDevice, st));
    double *d_gram = L.out(ws, o_acc, (double *)out_gram);
    u64 *d_sum = L.out(ws, o_accs, (u64 *)out_sum);
    MTS_HIP(hipMemsetAsync(d_gram, 0, 8 * (size_t)n_groups * nn, st));
    MTS_HIP(hipMemsetAsync(d_sum, 0, 8 * (size_t)n_groups * n_cols, st));
    double *d_part = (double *)(ws + o_part);
    u64 *d_psum = (u64 *)(ws + o_psum);
    const long *d_slab = (const long *)(ws + o_slab), *d_gf = (const long *)(ws + o_gf);
    const bool exact = !(flags & MTS_FLAG_FLOAT) && sz <= 2;
    const int float_sum = (flags & MTS_FLAG_FLOAT) ? 1 : 0;
    rc = H.run(E, st, status, [&](const FeedPiece &Pc, const PieceSegs &S) {
        int r = MTS_OK;
        const long p_s0 = gfirst[Pc.u0], p_s1 = gfirst[Pc.u1];
        for (long s = p_s0; !r && s < p_s1; s += run_slabs) {
            const long s1 = std::min(p_s1, s + run_slabs);
            r = launch_gram(st, sz, flags, S.base, S.row0, S.ns, nc, (const int *)(ws + o_cols), n_cols, d_slab, s, s1 - s, d_part, d_psum);
            // the groups the slabs [s, s1) belong to
            const long g0 = std::upper_bound(gfirst.begin(), gfirst.end(), s) - gfirst.begin() - 1;
            const long g1 = std::lower_bound(gfirst.begin(), gfirst.end(), s1) - gfirst.begin();
            for (long ga = g0; !r && ga < g1; ga += 65535)
                r = launch_gram_combine(st, d_part, d_psum, s, s1, ga, std::min(g1, ga + 65535), d_gf, n_cols, float_sum, d_gram, d_sum);
        }
        return r;
    });
    if (rc) return rc;
    if (exact && (rc = launch_gram_finish(st, d_gram, n_groups * (long)nn))) return rc;
    if (out_on_host) {
        MTS_HIP(hipMemcpyAsync(out_gram, d_gram, 8 * (size_t)n_groups * nn, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_sum, d_sum, 8 * (size_t)n_groups * n_cols, hipMemcpyDeviceToHost, st));
    }
    MTS_HIP(hipStreamSynchronize(st));
    return MTS_OK;
}

// ---- Gram matrices of the filtered signal (mts_filtered_gram, mts_dev_filtered_gram) --------------------------------------------
// mts_gram of a float32 recording whose items are z.  The grid, the groups, the Gram slabs and the accumulators are gram_run's; the
// unit is a group, and piece p owns the groups whose first row lies in its chunks.  Their rows read their filter support.  A piece's
// Gram slabs go through the float32 workspace in z slabs (filter -> median -> k_zgram -> the combine, on the stream): a z slab holds
// whole Gram slabs of one or more groups (zgram_slabs, reduce_plan.h), at most MTS_ZGRAM_SLAB_BYTES of z and GRAM_SLAB_BYTES of
// partials.  The combine adds a z slab's partials to their groups' accumulators in slab order, so every group sum is the same
// sequence of additions whatever the z slabs, pieces and calls.
static const u64 ZGRAM_SLAB_BYTES = 256ull << 20;

static int filtered_gram_run(Engine &E, hipStream_t st, const ChunkTable &T, const ZArgs &Z, long range_begin, long range_end, long window_rows,
                             long group_begin, long group_end, double *out_gram, double *out_sum, bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    const long vb = Z.vb, ve = Z.ve;
    const int n_cols = Z.n_cols, n_taps = Z.n_taps;
    int rc;
    if ((rc = check_zargs(T, Z, MTS_GRAM_MAX_COLS))) return rc;
    if (window_rows < 1) { set_error("filtered gram: window_rows %ld < 1", window_rows); return MTS_E_ARG; }
    if (range_begin < vb || range_end <= range_begin || range_end > ve) {
        set_error("filtered gram: range [%ld, %ld) empty or outside the valid rows [%ld, %ld)", range_begin, range_end, vb, ve); return MTS_E_ARG;
    }
    const long GR = GRAM_GROUP_ROWS, SR = GRAM_SLAB_ROWS;
    const long K = (window_rows + GR - 1) / GR;                   // groups per whole window
    const long n_range = range_end - range_begin, n_full = n_range / window_rows, tail = n_range % window_rows;
    const long total_groups = n_full * K + (tail + GR - 1) / GR;
    if (group_begin < 0 || group_end <= group_begin || group_end > total_groups) {
        set_error("filtered gram: groups [%ld, %ld) empty or outside the %ld groups of the range", group_begin, group_end, total_groups); return MTS_E_ARG;
    }
    if (!out_gram || !out_sum) { set_error("filtered gram: no output buffer"); return MTS_E_ARG; }
    if ((rc = check_columns(Z.cols, n_cols, T.nc))) return rc;
    if ((rc = check_chunk_table(true, T))) return rc;
    const long n_groups = group_end - group_begin;
    if (n_groups > (1l << 31)) { set_error("filtered gram: too many groups in one call"); return MTS_E_ARG; }
    const long half = (n_taps - 1) / 2;
    // the rows that groups [u0, u1) (call-local) read: the filter support of theirs ∩ valid range
    auto rows = [&](long u0, long u1, long *lo, long *hi) {
        long a, b, tmp;
        gram_group_rows(range_begin, range_end, window_rows, GR, group_begin + u0, &a, &tmp);
        gram_group_rows(range_begin, range_end, window_rows, GR, group_begin + u1 - 1, &tmp, &b);
        *lo = std::max(vb, a + half - (n_taps - 1)); *hi = std::min(ve, b + half);
    };
    long need_lo, need_hi;
    rows(0, n_groups, &need_lo, &need_hi);
    if ((rc = check_cover("filtered gram", T, need_lo, need_hi))) return rc;
    status_ok(T, status);
    // Gram slabs of the call: slab_rows (2 per slab), gfirst[g] the first slab of call group g
    std::vector<long> gfirst(n_groups + 1, 0), glo(n_groups), slab_rows;
    for (long g = 0; g < n_groups; g++) {
        long hi;
        gram_group_rows(range_begin, range_end, window_rows, GR, group_begin + g, &glo[g], &hi);
        gfirst[g] = (long)slab_rows.size() / 2;
        gram_cut_slabs(glo[g], hi, SR, slab_rows);
    }
    const long n_slabs = gfirst[n_groups] = (long)slab_rows.size() / 2;

    HaloFeed H(T, out_on_host);
    // the first group whose first row is at or after row r
    if ((rc = H.plan(n_groups, [&](long r) { return std::lower_bound(glo.begin(), glo.end(), r) - glo.begin(); }, rows))) return rc;
    // a z slab: whole Gram slabs, z <= MTS_ZGRAM_SLAB_BYTES (never less than one Gram slab), their partials <= GRAM_SLAB_BYTES
    const long cap_rows = zgram_cap_rows(env_bytes("MTS_ZGRAM_SLAB_BYTES", ZGRAM_SLAB_BYTES), n_cols, SR);
    const long cap_slabs = std::min(n_slabs, std::min(65535l, (long)std::max<u64>(1, GRAM_SLAB_BYTES / (u64)gram_slab_bytes(n_cols))));
    const long z_rows = std::min(cap_rows, std::min(cap_slabs * SR, slab_rows[2 * n_slabs - 1] - slab_rows[0]));
    const u64 nn = (u64)n_cols * n_cols;
    // ---- workspace: taps, columns, the slab tables, the segment tables, the filtered slab, the partials, the accumulators
    WsLayout &L = H.L;
    ZStage F(Z, L);
    const size_t o_slab = L.take(16 * (u64)n_slabs), o_gf = L.take(8 * (u64)(n_groups + 1)), o_seg = L.take(H.table_bytes()),
                 o_y = L.take(4 * (u64)z_rows * n_cols), o_part = L.take((u64)cap_slabs * gram_pairs(n_cols) * 64 * 64 * 8),
                 o_psum = L.take((u64)cap_slabs * 8 * n_cols), o_acc = L.take_out(8 * (u64)n_groups * nn),
                 o_accs = L.take_out(8 * (u64)n_groups * n_cols);
    StreamGuard G{st};
    if ((rc = H.place(E, st, E.zgram, o_seg))) return rc;
    u8 *ws = E.zgram.as<u8>();
    if ((rc = F.upload(st, ws))) return rc;
    MTS_HIP(hipMemcpyAsync(ws + o_slab, slab_rows.data(), 16 * (size_t)n_slabs, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_gf, gfirst.data(), 8 * (size_t)(n_groups + 1), hipMemcpyHostToDevice, st));
    double *d_gram = L.out(ws, o_acc, out_gram);
    u64 *d_sum = L.out(ws, o_accs, (u64 *)out_sum);
    MTS_HIP(hipMemsetAsync(d_gram, 0, 8 * (size_t)n_groups * nn, st));
    MTS_HIP(hipMemsetAsync(d_sum, 0, 8 * (size_t)n_groups * n_cols, st));
    float *d_y = (float *)(ws + o_y);
    double *d_part = (double *)(ws + o_part);
    u64 *d_psum = (u64 *)(ws + o_psum);
    const long *d_slab = (const long *)(ws + o_slab), *d_gf = (const long *)(ws + o_gf);
    rc = H.run(E, st, status, [&](const FeedPiece &Pc, const PieceSegs &Sg) {
        int r = MTS_OK;
        for (const ZgramSlab &zs : zgram_slabs(slab_rows.data(), gfirst[Pc.u0], gfirst[Pc.u1], cap_rows, cap_slabs)) {
            const long a = slab_rows[2 * zs.s0], b = slab_rows[2 * zs.s1 - 1];
            if ((r = F.filter(st, T, Sg, a, b, d_y))) break;
            if ((r = launch_zgram(st, d_y, a, n_cols, d_slab, zs.s0, zs.s1 - zs.s0, d_part, d_psum))) break;
            // the groups the slabs [s0, s1) belong to
            const long g0 = std::upper_bound(gfirst.begin(), gfirst.end(), zs.s0) - gfirst.begin() - 1;
            const long g1 = std::lower_bound(gfirst.begin(), gfirst.end(), zs.s1) - gfirst.begin();
            for (long ga = g0; !r && ga < g1; ga += 65535)
                r = launch_gram_combine(st, d_part, d_psum, zs.s0, zs.s1, ga, std::min(g1, ga + 65535), d_gf, n_cols, 1, d_gram, d_sum);
            if (r) break;
        }
        return r;
    });
    if (rc) return rc;
    if (out_on_host) {                                        // the accumulators, and nothing else, cross the bus
        MTS_HIP(hipMemcpyAsync(out_gram, d_gram, 8 * (size_t)n_groups * nn, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_sum, d_sum, 8 * (size_t)n_groups * n_cols, hipMemcpyDeviceToHost, st));
    }
    return G.wait();
}

// The chunk table has the same names in every host entry and in every device entry of include/mtscomp_hip.h: `call` is the op's run
// on (Engine &E, const ChunkTable &T).
#define HOST_ENTRY(call)                                                                                                                     \
    reduce_entry(device, cache_id,                                                                                                           \
               host_table(cache_id, n_chunks, chunk_keys, chunk_row0, cdata, c_offsets, c_lengths, n_rows, n_channels, itemsize, flags, chunk_status), \
               [&](Engine &E, const ChunkTable &T) { return call; })
#define DEV_ENTRY(call)                                                                                                                      \
    reduce_entry(device, 0, dev_table(d_cdata, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels, itemsize, flags, chunk_status), \
              [&](Engine &E, const ChunkTable &T) { return call; })
// (so have the filter arguments in every entry of the z family)
#define Z_ARGS(op) ZArgs{op, valid_begin, valid_end, n_taps, taps, n_cols, cols, reference}

extern "C" {

int mts_window_stats(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                     const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_begin,
                     long row_end, long window_rows, int n_cols, const int *cols, void *out_min, void *out_max, void *out_sum, void *out_sumsq,
                     long *out_count, int *chunk_status)
{
    return HOST_ENTRY(window_stats_run(E, nullptr, T, row_begin, row_end, window_rows, n_cols, cols, out_min, out_max, out_sum, out_sumsq, true,
                      out_count, chunk_status));
}

int mts_dev_window_stats(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                         const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_begin,
                         long row_end, long window_rows, int n_cols, const int *cols, void *d_min, void *d_max, void *d_sum, void *d_sumsq,
                         long *count, int *chunk_status)
{
    return DEV_ENTRY(window_stats_run(E, (hipStream_t)stream, T, row_begin, row_end, window_rows, n_cols, cols, d_min, d_max, d_sum, d_sumsq, false,
                     count, chunk_status));
}

int mts_rank_hist(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                  const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_begin,
                  long row_end, long window_rows, int n_cols, const int *cols, int mode, const double *center,
                  const unsigned long long *sel_prefix, const int *sel_shift, unsigned int *out_hist, unsigned long long *out_kmin,
                  unsigned long long *out_kmax, long *out_count, int *chunk_status)
{
    return HOST_ENTRY(rank_hist_run(E, nullptr, T, row_begin, row_end, window_rows, n_cols, cols, mode, center, sel_prefix, sel_shift, out_hist,
                      out_kmin, out_kmax, true, out_count, chunk_status));
}

int mts_dev_rank_hist(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                      const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_begin,
                      long row_end, long window_rows, int n_cols, const int *cols, int mode, const double *center,
                      const unsigned long long *sel_prefix, const int *sel_shift, unsigned int *d_hist, unsigned long long *d_kmin,
                      unsigned long long *d_kmax, long *count, int *chunk_status)
{
    return DEV_ENTRY(rank_hist_run(E, (hipStream_t)stream, T, row_begin, row_end, window_rows, n_cols, cols, mode, center, sel_prefix, sel_shift,
                     d_hist, d_kmin, d_kmax, false, count, chunk_status));
}

int mts_filtered_rank_hist(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                           const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags,
                           long valid_begin, long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                           long row_begin, long row_end, long window_rows, long count_begin, long count_end, int mode, const double *center,
                           const unsigned long long *sel_prefix, const int *sel_shift, unsigned int *out_hist, unsigned long long *out_kmin,
                           unsigned long long *out_kmax, long *out_count, int *chunk_status)
{
    return HOST_ENTRY(filtered_rank_hist_run(E, nullptr, T, Z_ARGS("filtered rank hist"), row_begin, row_end, window_rows, count_begin, count_end,
                      mode, center, sel_prefix, sel_shift, out_hist, out_kmin, out_kmax, true, out_count, chunk_status));
}

int mts_dev_filtered_rank_hist(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                               const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags,
                               long valid_begin, long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                               long row_begin, long row_end, long window_rows, long count_begin, long count_end, int mode,
                               const double *center, const unsigned long long *sel_prefix, const int *sel_shift, unsigned int *d_hist,
                               unsigned long long *d_kmin, unsigned long long *d_kmax, long *count, int *chunk_status)
{
    return DEV_ENTRY(filtered_rank_hist_run(E, (hipStream_t)stream, T, Z_ARGS("filtered rank hist"), row_begin, row_end, window_rows, count_begin,
                     count_end, mode, center, sel_prefix, sel_shift, d_hist, d_kmin, d_kmax, false, count, chunk_status));
}

int mts_filtered_gram(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                      const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                      long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long range_begin, long range_end,
                      long window_rows, long group_begin, long group_end, double *out_gram, double *out_sum, int *chunk_status)
{
    return HOST_ENTRY(filtered_gram_run(E, nullptr, T, Z_ARGS("filtered gram"), range_begin, range_end, window_rows, group_begin, group_end, out_gram,
                      out_sum, true, chunk_status));
}

int mts_dev_filtered_gram(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                          const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                          long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long range_begin,
                          long range_end, long window_rows, long group_begin, long group_end, double *d_gram, double *d_sum, int *chunk_status)
{
    return DEV_ENTRY(filtered_gram_run(E, (hipStream_t)stream, T, Z_ARGS("filtered gram"), range_begin, range_end, window_rows, group_begin,
                     group_end, d_gram, d_sum, false, chunk_status));
}

int mts_decimate(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                 const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                 long valid_end, long first_row, long n_out, int q, int n_taps, const double *taps, int out_itemsize, int n_cols, const int *cols,
                 void *out, int *chunk_status)
{
    return HOST_ENTRY(decimate_run(E, nullptr, T, valid_begin, valid_end, first_row, n_out, q, n_taps, taps, out_itemsize, n_cols, cols, out, true,
                      chunk_status));
}

int mts_dev_decimate(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths, const long *chunk_row0,
                     const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin, long valid_end, long first_row,
                     long n_out, int q, int n_taps, const double *taps, int out_itemsize, int n_cols, const int *cols, void *d_out,
                     int *chunk_status)
{
    return DEV_ENTRY(decimate_run(E, (hipStream_t)stream, T, valid_begin, valid_end, first_row, n_out, q, n_taps, taps, out_itemsize, n_cols, cols,
                     d_out, false, chunk_status));
}

int mts_project(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_begin,
                long row_end, int n_cols, const int *cols, const double *offset, int n_out, const double *weights, int out_itemsize, void *out,
                int *chunk_status)
{
    return HOST_ENTRY(project_run(E, nullptr, T, row_begin, row_end, n_cols, cols, offset, n_out, weights, out_itemsize, out, true, chunk_status));
}

int mts_dev_project(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths, const long *chunk_row0,
                    const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_begin, long row_end, int n_cols,
                    const int *cols, const double *offset, int n_out, const double *weights, int out_itemsize, void *d_out, int *chunk_status)
{
    return DEV_ENTRY(project_run(E, (hipStream_t)stream, T, row_begin, row_end, n_cols, cols, offset, n_out, weights, out_itemsize, d_out, false,
                     chunk_status));
}

int mts_detect(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
               const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
               long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols,
               const float *threshold, int sign, int reference, int exclude_rows, int exclude_cols, long max_events, long *out_row,
               int *out_pos, float *out_amp, long *n_events, int *chunk_status)
{
    return HOST_ENTRY(detect_run(E, nullptr, T, Z_ARGS("detect"), row_begin, row_end, threshold, sign, exclude_rows, exclude_cols, max_events,
                      out_row, out_pos, out_amp, true, n_events, chunk_status));
}

int mts_dev_detect(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                   const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                   long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols,
                   const float *threshold, int sign, int reference, int exclude_rows, int exclude_cols, long max_events, long *d_row,
                   int *d_pos, float *d_amp, long *n_events, int *chunk_status)
{
    return DEV_ENTRY(detect_run(E, (hipStream_t)stream, T, Z_ARGS("detect"), row_begin, row_end, threshold, sign, exclude_rows, exclude_cols,
                     max_events, d_row, d_pos, d_amp, false, n_events, chunk_status));
}

int mts_waveforms(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                  const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                  long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                  const long *ev_row, const int *ev_col0, int before, int after, int width, float *out_wave, float *out_min, int *out_argmin,
                  float *out_max, int *out_argmax, int *chunk_status)
{
    return HOST_ENTRY(waveforms_run(E, nullptr, T, Z_ARGS("waveforms"), n_events, ev_row, ev_col0, before, after, width, out_wave, out_min,
                      out_argmin, out_max, out_argmax, true, chunk_status));
}

int mts_dev_waveforms(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                      const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                      long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                      const long *ev_row, const int *ev_col0, int before, int after, int width, float *d_wave, float *d_min, int *d_argmin,
                      float *d_max, int *d_argmax, int *chunk_status)
{
    return DEV_ENTRY(waveforms_run(E, (hipStream_t)stream, T, Z_ARGS("waveforms"), n_events, ev_row, ev_col0, before, after, width, d_wave, d_min,
                     d_argmin, d_max, d_argmax, false, chunk_status));
}

int mts_mean_waveforms(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                       const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                       long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                       const long *ev_row, const int *ev_col0, const int *ev_label, int n_labels, int before, int after, int width,
                       double resolution, long long *out_sum, int *out_count, long *out_skipped, int *chunk_status)
{
    return HOST_ENTRY(mean_waveforms_run(E, nullptr, T, Z_ARGS("mean_waveforms"), n_events, ev_row, ev_col0, ev_label, n_labels, before, after, width,
                      resolution, out_sum, out_count, out_skipped, true, chunk_status));
}

int mts_dev_mean_waveforms(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                           const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                           long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                           const long *ev_row, const int *ev_col0, const int *ev_label, int n_labels, int before, int after, int width,
                           double resolution, long long *d_sum, int *d_count, long *d_skipped, int *chunk_status)
{
    return DEV_ENTRY(mean_waveforms_run(E, (hipStream_t)stream, T, Z_ARGS("mean_waveforms"), n_events, ev_row, ev_col0, ev_label, n_labels, before,
                     after, width, resolution, d_sum, d_count, d_skipped, false, chunk_status));
}

int mts_waveform_features(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                          const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                          long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                          const long *ev_row, const int *ev_col0, int before, int after, int width, int n_comp, const float *basis, float *out_feat,
                          int *chunk_status)
{
    return HOST_ENTRY(waveform_features_run(E, nullptr, T, Z_ARGS("waveform_features"), n_events, ev_row, ev_col0, before, after, width, n_comp, basis,
                      out_feat, true, chunk_status));
}

int mts_dev_waveform_features(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                              const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                              long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                              const long *ev_row, const int *ev_col0, int before, int after, int width, int n_comp, const float *basis,
                              float *d_feat, int *chunk_status)
{
    return DEV_ENTRY(waveform_features_run(E, (hipStream_t)stream, T, Z_ARGS("waveform_features"), n_events, ev_row, ev_col0, before, after, width,
                     n_comp, basis, d_feat, false, chunk_status));
}

int mts_localize(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                 const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                 long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                 const long *ev_row, const int *ev_col0, int before, int after, int width, int mode, int n_dims, const float *positions,
                 float *out_amp, float *out_weight, float *out_moment, int *out_best, int *chunk_status)
{
    return HOST_ENTRY(localize_run(E, nullptr, T, Z_ARGS("localize"), n_events, ev_row, ev_col0, before, after, width, mode, n_dims, positions,
                      out_amp, out_weight, out_moment, out_best, true, chunk_status));
}

int mts_dev_localize(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                     const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                     long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                     const long *ev_row, const int *ev_col0, int before, int after, int width, int mode, int n_dims, const float *positions,
                     float *d_amp, float *d_weight, float *d_moment, int *d_best, int *chunk_status)
{
    return DEV_ENTRY(localize_run(E, (hipStream_t)stream, T, Z_ARGS("localize"), n_events, ev_row, ev_col0, before, after, width, mode, n_dims,
                     positions, d_amp, d_weight, d_moment, d_best, false, chunk_status));
}

int mts_waveforms_last_plan(int device, long *out)
{
    Engine *E;
    if (!out) return MTS_E_ARG;
    const int rc = get_engine(device, &E);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(E->mu);
    memcpy(out, E->wav_plan, sizeof E->wav_plan);
    return MTS_OK;
}

int mts_correlate(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                  const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                  long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                  int before, int T_, int n_out, const float *templates, float *out, int *chunk_status)
{
    return HOST_ENTRY(correlate_run(E, nullptr, T, Z_ARGS("correlate"), row_begin, row_end, before, T_, n_out, templates, out, true, chunk_status));
}

int mts_dev_correlate(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                      const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                      long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                      int before, int T_, int n_out, const float *templates, float *d_out, int *chunk_status)
{
    return DEV_ENTRY(correlate_run(E, (hipStream_t)stream, T, Z_ARGS("correlate"), row_begin, row_end, before, T_, n_out, templates, d_out, false,
                     chunk_status));
}

int mts_match_templates(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                        const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags,
                        long valid_begin, long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols,
                        const int *cols, int reference, int before, int T_, int n_out, const float *templates, const float *threshold,
                        int exclude_rows, long max_events, long *out_row, int *out_template, float *out_score, long *n_events,
                        int *chunk_status)
{
    return HOST_ENTRY(tmatch_run(E, nullptr, T, Z_ARGS("match_templates"), row_begin, row_end, before, T_, n_out, templates, threshold, exclude_rows,
                      max_events, out_row, out_template, out_score, true, n_events, chunk_status));
}

int mts_dev_match_templates(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                            const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags,
                            long valid_begin, long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols,
                            const int *cols, int reference, int before, int T_, int n_out, const float *templates, const float *threshold,
                            int exclude_rows, long max_events, long *d_row, int *d_template, float *d_score, long *n_events,
                            int *chunk_status)
{
    return DEV_ENTRY(tmatch_run(E, (hipStream_t)stream, T, Z_ARGS("match_templates"), row_begin, row_end, before, T_, n_out, templates, threshold,
                     exclude_rows, max_events, d_row, d_template, d_score, false, n_events, chunk_status));
}

int mts_residual(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                 const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                 long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                 int before, int T_, int n_out, const float *templates, long n_sub, const long *sub_row, const int *sub_tpl, const float *sub_amp,
                 float *out, int *chunk_status)
{
    return HOST_ENTRY(residual_run(E, nullptr, T, Z_ARGS("residual"), row_begin, row_end, before, T_, n_out, templates, n_sub, sub_row, sub_tpl,
                      sub_amp, out, true, chunk_status));
}

int mts_dev_residual(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                     const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                     long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                     int before, int T_, int n_out, const float *templates, long n_sub, const long *sub_row, const int *sub_tpl,
                     const float *sub_amp, float *d_out, int *chunk_status)
{
    return DEV_ENTRY(residual_run(E, (hipStream_t)stream, T, Z_ARGS("residual"), row_begin, row_end, before, T_, n_out, templates, n_sub, sub_row,
                     sub_tpl, sub_amp, d_out, false, chunk_status));
}

int mts_match_residual(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                       const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags,
                       long valid_begin, long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols,
                       const int *cols, int reference, int before, int T_, int n_out, const float *templates, const float *threshold,
                       int exclude_rows, long max_events, long n_sub, const long *sub_row, const int *sub_tpl, const float *sub_amp,
                       long *out_row, int *out_template, float *out_score, long *n_events, int *chunk_status)
{
    return HOST_ENTRY(tmatch_run(E, nullptr, T, Z_ARGS("match_templates"), row_begin, row_end, before, T_, n_out, templates, threshold, exclude_rows,
                      max_events, out_row, out_template, out_score, true, n_events, chunk_status, n_sub, sub_row, sub_tpl, sub_amp));
}

int mts_dev_match_residual(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                           const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags,
                           long valid_begin, long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols,
                           const int *cols, int reference, int before, int T_, int n_out, const float *templates, const float *threshold,
                           int exclude_rows, long max_events, long n_sub, const long *sub_row, const int *sub_tpl, const float *sub_amp,
                           long *d_row, int *d_template, float *d_score, long *n_events, int *chunk_status)
{
    return DEV_ENTRY(tmatch_run(E, (hipStream_t)stream, T, Z_ARGS("match_templates"), row_begin, row_end, before, T_, n_out, templates, threshold,
                     exclude_rows, max_events, d_row, d_template, d_score, false, n_events, chunk_status, n_sub, sub_row, sub_tpl, sub_amp));
}

int mts_welch(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
              const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_seg0,
              long seg_begin, long seg_end, int nperseg, long step, const double *taper, int detrend, int csize, int n_cols,
              const int *cols, double *out, int *chunk_status)
{
    return HOST_ENTRY(welch_run(E, nullptr, T, row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend, csize, n_cols, cols, out, true,
                      chunk_status));
}

int mts_dev_welch(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths, const long *chunk_row0,
                  const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_seg0, long seg_begin, long seg_end,
                  int nperseg, long step, const double *taper, int detrend, int csize, int n_cols, const int *cols, double *d_out,
                  int *chunk_status)
{
    return DEV_ENTRY(welch_run(E, (hipStream_t)stream, T, row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend, csize, n_cols, cols, d_out,
                     false, chunk_status));
}

int mts_gram(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
             const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long range_begin,
             long range_end, long window_rows, long group_begin, long group_end, int n_cols, const int *cols, void *out_gram, void *out_sum,
             int *chunk_status)
{
    return HOST_ENTRY(gram_run(E, nullptr, T, range_begin, range_end, window_rows, group_begin, group_end, n_cols, cols, out_gram, out_sum, true,
                      chunk_status));
}

int mts_dev_gram(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths, const long *chunk_row0,
                 const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long range_begin, long range_end, long window_rows,
                 long group_begin, long group_end, int n_cols, const int *cols, void *d_gram, void *d_sum, int *chunk_status)
{
    return DEV_ENTRY(gram_run(E, (hipStream_t)stream, T, range_begin, range_end, window_rows, group_begin, group_end, n_cols, cols, d_gram, d_sum,
                     false, chunk_status));
}

}  // extern "C"
