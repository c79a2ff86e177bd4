// The codec's host side: the compress and inflate pipelines over one sub-batch (plan -> ensure -> upload -> launch; the plans are in
// codec_plan.h and know no device), the sub-batch drivers, their device and host entry points and the debug taps.
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "engine.h"
#include "reduce_plan.h"

namespace mts {

static const LevelCfg LEVELS[10] = {{0, 0, 0, 0},     {4, 4, 8, 4},       {4, 5, 16, 8},       {4, 6, 32, 32},
                                    {4, 4, 16, 16},   {8, 16, 32, 32},    {8, 16, 128, 128},   {8, 32, 128, 256},
                                    {32, 128, 258, 1024}, {32, 258, 258, 4096}};

constexpr int PARSE_PARALLEL_ROUNDS = 96;     // parallel correction rounds of the speculative parse (~40 us each) before the in-order pass:
                                              // chains of a few dozen segments (a dead channel) are cheaper in parallel, whole-chunk chains are not


// ------------------------------------------------------------------------------------------------
// compress pipeline over one sub-batch of chunks (device resident)
// ------------------------------------------------------------------------------------------------
struct DebugTap {              // optional host copies of intermediates (tests)
    unsigned *t_full = nullptr, *t_quarter = nullptr;
    unsigned short *tokens = nullptr;
    long *n_tokens = nullptr;
};

static int compress_batch(Engine &E, hipStream_t st, const u8 *d_raw, bool raw_is_stream, int nc, int sz,
                          const long *bounds, int n_chunks, int flags, int level, u8 *d_out, const long *slot_off,
                          long *out_sizes, bool accumulate_times, DebugTap *tap)
{
    const LevelCfg cfg = LEVELS[level];
    // ---- plan ----
    static const CompressDims dims = {hash_sort_ws_bytes, parse_marks_words, parse_cp_words(), sizeof(BlockRec), sizeof(ChunkOut), BLK_CODE_WORDS, BLK_HDR_WORDS, MATCH_SINK_BYTES};
    const CompressPlan P(bounds, n_chunks, (u64)nc * sz, raw_is_stream, slot_off, level, dims);
    if (P.error[0]) { set_error("%s", P.error); return MTS_E_ARG; }
    const std::vector<ChunkDesc> &cd = P.cd;
    const std::vector<TileDesc> &tiles = P.tiles;
    const u32 nseg = P.nseg, nblk = P.nblk, max_rows = P.max_rows, max_n = P.max_n, max_nseg = P.max_nseg;
    const size_t table_words = P.table_words;
    // ---- environment (per batch, but for the flag print) ----
    int force_ballot = getenv("MTS_SORT_INJECT_DISORDER") ? 2 : 0;      // (test hook: the first sort of the call is deliberately mis-ranked)
    const char *be = getenv("MTS_FAST_LIST_BYTES");           // (tests: a tiny budget = many phases)
    const u64 fast_list_budget = be ? strtoull(be, nullptr, 10) : (u64)8 << 30;
    const bool debug_addr = getenv("MTS_DEBUG_ADDR") != nullptr;        // (tools/m5_addr_times.py: does the match stage's time follow where its buffers lie?)
    static const bool debug_flags = getenv("MTS_DEBUG_FLAGS") != nullptr;      // (read once)
    // ---- workspace ----
    int rc;
    if (!raw_is_stream) { if ((rc = E.stream.ensure(P.stream_bytes))) return rc; }
    if ((rc = E.sort_a.ensure(P.sort_a))) return rc;
    if ((rc = E.sort_b.ensure(P.sort_b))) return rc;
    if ((rc = E.sort_ws.ensure(P.sort_ws))) return rc;
    if ((rc = E.tables.ensure(P.tables))) return rc;
    if ((rc = E.tokens.ensure(P.tokens))) return rc;
    if ((rc = E.segbuf.ensure(P.segbuf))) return rc;
    if ((rc = E.blk.ensure(P.blk))) return rc;
    if ((rc = E.blkcodes.ensure(P.blkcodes))) return rc;
    if ((rc = E.blkhdr.ensure(P.blkhdr))) return rc;
    if ((rc = E.desc.ensure(P.desc))) return rc;
    if ((rc = E.adler.ensure(P.adler))) return rc;
    if ((rc = E.init_events())) return rc;

    u8 *dp = E.desc.as<u8>();
    ChunkDesc *d_chunks = (ChunkDesc *)(dp + P.o_chunks);
    TileDesc *d_tiles = (TileDesc *)(dp + P.o_tiles);
    ChunkOut *d_cout = (ChunkOut *)(dp + P.o_cout);
    // per-segment arrays, the flag words, block arrays: where the plan says
    u32 *sg = E.segbuf.as<u32>();
    u8 *ad = E.adler.as<u8>(), *bk = E.blk.as<u8>();
    const ParseBufs pb = {sg + P.seg.entry, sg + P.seg.exit_a, sg + P.seg.exit_b, sg + P.seg.cnt, sg + P.seg.tokbase, sg + P.seg.cp, E.sort_a.as<u32>(),
                          sg + P.seg.seg_chunk, sg + P.seg.seg_start, (int *)(ad + P.ad.changed)};
    u32 *d_flags = (u32 *)(ad + P.ad.flags);                  // [0] bit 0: the match stage found a hash run out of position order
    BlockRec *d_blocks = (BlockRec *)(bk + P.bk.blocks);
    u32 *d_blk_chunk = (u32 *)(bk + P.bk.chunk), *d_blk_in_start = (u32 *)(bk + P.bk.in_start);

    // ---- upload ----
    MTS_HIP(hipMemcpyAsync(d_chunks, cd.data(), sizeof(ChunkDesc) * n_chunks, hipMemcpyHostToDevice, st));
    {
        // the index arrays depend on the chunk sizes only: kept on the device while the next batch has the same sizes and
        // the buffers have not moved
        std::vector<u32> sizes_now(n_chunks);
        for (int i = 0; i < n_chunks; i++) sizes_now[i] = cd[i].n;
        const bool same = sizes_now == E.geo_n && E.geo_seg == E.segbuf.gen && E.geo_blk == E.blk.gen && E.geo_desc == E.desc.gen;
        if (!same) {
            E.geo_n.clear();                                      // (not valid again until everything below is on its way)
            std::vector<u32> h_seg, h_blk_chunk;
            P.index_arrays(h_seg, h_blk_chunk);
            if (!tiles.empty()) MTS_HIP(hipMemcpyAsync(d_tiles, tiles.data(), sizeof(TileDesc) * tiles.size(), hipMemcpyHostToDevice, st));
            if (nseg) {
                MTS_HIP(hipMemcpyAsync(pb.seg_chunk, h_seg.data(), 4 * (size_t)nseg, hipMemcpyHostToDevice, st));
                MTS_HIP(hipMemcpyAsync(pb.seg_start, h_seg.data() + nseg, 4 * (size_t)nseg, hipMemcpyHostToDevice, st));
            }
            MTS_HIP(hipMemcpyAsync(d_blk_chunk, h_blk_chunk.data(), 4 * (size_t)nblk, hipMemcpyHostToDevice, st));
            // (pageable copies: staged before hipMemcpyAsync returns, so the vectors may go)
            E.geo_n = sizes_now; E.geo_seg = E.segbuf.gen; E.geo_blk = E.blk.gen; E.geo_desc = E.desc.gen;
        }
    }
    MTS_HIP(hipMemsetAsync(d_cout, 0, sizeof(ChunkOut) * n_chunks, st));
    MTS_HIP(hipMemsetAsync(pb.changed, 0, 8, st));           // + the match stage's flag word behind it
    // the host copies above must be complete before the std::vectors go away; they are pageable
    // copies, which hipMemcpyAsync finishes staging before returning.

    // ---- launch ----
    E.t_begin(st);
    const u8 *d_stream;
    u64 *d_adler = E.adler.as<u64>();
    std::vector<u64> so(n_chunks); std::vector<u32> nn(n_chunks);
    if (raw_is_stream) {
        // debug path: the caller's bytes already are the transformed stream (one chunk)
        d_stream = d_raw;
        for (int i = 0; i < n_chunks; i++) { so[i] = cd[i].stream_off; nn[i] = cd[i].n; }
        if ((rc = E.misc.ensure(P.misc))) return rc;
        u64 *d_so = (u64 *)(E.misc.as<u8>() + P.mi.so); u32 *d_nn = (u32 *)(E.misc.as<u8>() + P.mi.nn);
        MTS_HIP(hipMemcpyAsync(d_so, so.data(), 8 * (size_t)n_chunks, hipMemcpyHostToDevice, st));
        MTS_HIP(hipMemcpyAsync(d_nn, nn.data(), 4 * (size_t)n_chunks, hipMemcpyHostToDevice, st));
        if ((rc = launch_adler_stream(st, d_stream, d_so, d_nn, n_chunks, max_n, d_adler, nullptr, 0))) return rc;
    } else {
        if ((rc = launch_delta_transpose(st, d_raw, E.stream.p, d_chunks, n_chunks, max_rows, nc, sz, flags, d_adler))) return rc;
        d_stream = E.stream.as<u8>();
    }
    E.t_mark(st, "delta_transpose");
    u32 *tmp_k = E.sort_a.as<u32>(), *srt_k = E.sort_b.as<u32>();
    u32 *d_tables = E.tables.as<u32>(), *d_quarter = d_tables + table_words;
    u32 *d_tokens = E.tokens.as<u32>();
    const bool fast = level < 4;                              // deflate_fast: no candidate tables, the walk itself searches (deflate.hip, section F)
    u32 *d_inv = (u32 *)d_tables;                             // levels 1..3: the inverse map lives where the other levels keep the candidate tables
    int fix_rounds = 0;                                       // parallel fix rounds of the parse that counted (they say where the exits are)
    for (;;) {
        if ((rc = launch_hash_sort(st, d_stream, d_tiles, (int)tiles.size(), tmp_k, srt_k, force_ballot, E.sort_ws.p))) return rc;
        E.t_mark(st, force_ballot == 1 ? "hash_sort_retry" : "hash_sort");
        int round = 0;
        bool resort = false;
        if (fast) {
            // one in-order pass per chunk over candidate lists made a phase (W positions of every chunk) at a time
            if ((rc = launch_inverse_map(st, d_stream, d_tiles, (int)tiles.size(), srt_k, d_inv, d_flags))) return rc;
            E.t_mark(st, "inverse_map");
            const u64 K = (u64)fast_list_rows(level);
            // two list buffers: the lists of phase k + 1 are made on a second stream while phase k is walked (the walk keeps
            // one wave per chunk busy, the rest of the device is free)
            const u64 W = CompressPlan::phase_width(fast_list_budget, n_chunks, K, max_n);
            if (max_n) {
                const size_t list_words = (size_t)n_chunks * W * K;
                if ((rc = E.fast_lists.ensure(2 * list_words * 4))) return rc;
                if ((rc = E.fast_state.ensure(fast_seq_state_bytes(n_chunks)))) return rc;
                if ((rc = E.init_fast_streams())) return rc;
                u32 *lists[2] = {E.fast_lists.as<u32>(), E.fast_lists.as<u32>() + list_words};
                MTS_HIP(hipEventRecord(E.fast_ev[4], st));       // the sort and the inverse map
                MTS_HIP(hipStreamWaitEvent(E.fast_st, E.fast_ev[4], 0));
                for (u64 ph = 0; ph * W < max_n; ph++) {
                    const int b = (int)(ph & 1);
                    if (ph >= 2) MTS_HIP(hipStreamWaitEvent(E.fast_st, E.fast_ev[2 + b], 0));      // the walk that read this buffer
                    if ((rc = launch_fast_cands(E.fast_st, d_stream, d_chunks, d_tiles, srt_k, d_inv, lists[b], (u32)W, (u32)ph, n_chunks, level, cfg))) return rc;
                    MTS_HIP(hipEventRecord(E.fast_ev[b], E.fast_st));
                    MTS_HIP(hipStreamWaitEvent(st, E.fast_ev[b], 0));
                    if ((rc = launch_fast_seq(st, d_stream, d_chunks, d_tiles, srt_k, d_inv, lists[b], (u32)W, (u32)ph, E.fast_state.p, n_chunks, level, cfg,
                                              d_tokens, d_blk_in_start, d_cout))) return rc;
                    MTS_HIP(hipEventRecord(E.fast_ev[2 + b], st));
                }
            }
            int hflags[2] = {0, 0};                              // {-, sort-order flag}
            MTS_HIP(hipMemcpyAsync(hflags, pb.changed, 8, hipMemcpyDeviceToHost, st));
            MTS_HIP(hipStreamSynchronize(st));
            if (hflags[1] & 1) resort = true;
        } else {
        if (debug_addr)
            fprintf(stderr, "[addr] stream %p sorted %p tables %p quarter %p tiles %zu\n", (void *)d_stream, (void *)srt_k, (void *)d_tables, (void *)d_quarter, tiles.size());
        if ((rc = launch_match(st, d_stream, d_tiles, (int)tiles.size(), srt_k, d_tables, d_quarter, cfg, d_flags, tap && tap->t_full ? 1 : 0))) return rc;
        E.t_mark(st, "match");
        if ((rc = launch_parse_spec(st, d_tables, d_quarter, d_chunks, pb, (int)nseg, cfg, n_chunks, max_nseg))) return rc;
        for (;;) {
            if ((rc = launch_parse_fix(st, d_tables, d_quarter, d_chunks, pb, (int)nseg, cfg, round))) return rc;
            round++;
            int hflags[2] = {0, 0};                              // {changed, match-stage flags}
            MTS_HIP(hipMemcpyAsync(hflags, pb.changed, 8, hipMemcpyDeviceToHost, st));
            MTS_HIP(hipStreamSynchronize(st));
            if (debug_flags) fprintf(stderr, "[flags] level %d round %d changed %d match-flags %d force_ballot %d\n", level, round, hflags[0], hflags[1], force_ballot);
            if (hflags[1] & 1) { resort = true; break; }
            if (!hflags[0]) break;
            MTS_HIP(hipMemsetAsync(pb.changed, 0, 4, st));
            if (round >= PARSE_PARALLEL_ROUNDS) {            // (runs, periodic data: the parse does not re-synchronise) the rest in order
                if ((rc = launch_parse_fix_serial(st, d_tables, d_quarter, d_chunks, pb, n_chunks, cfg, round))) return rc;
                break;
            }
        }
        }
        fix_rounds = round;
        if (!resort) break;
        // The lane-ordered LDS ranking of the sort (deflate.hip: rank_pass) did not hold: byte identity with zlib needs
        // position-ordered chains, so the stage is repeated with the ballot ranking, which relies on nothing.
        if (force_ballot == 1) { set_error("hash sort: runs out of position order even with the ballot ranking"); return MTS_E_INTERNAL; }
        force_ballot = 1;
        MTS_HIP(hipMemsetAsync(pb.changed, 0, 8, st));
    }
    // after an odd number of fix rounds the current exits live in exit_b; nothing downstream needs them
    E.t_mark(st, fast ? "fast_walk" : "parse_fixpoint");
    if (!fast) {                                              // (levels 1..3: the in-order walk has written tokens and counts)
        if ((rc = launch_parse_count(st, d_tables, d_chunks, pb, (int)nseg, n_chunks, cfg, d_cout))) return rc;
        if ((rc = launch_parse_emit_marks(st, d_stream, d_tables, d_quarter, d_chunks, pb, fix_rounds, d_tokens, d_blk_in_start, d_cout, n_chunks, max_nseg))) return rc;
    }
    E.t_mark(st, "parse_emit");
    if ((rc = launch_block_trees(st, d_chunks, d_blk_chunk, (int)nblk, d_tokens, d_blk_in_start, d_cout, d_blocks,
                                 E.blkcodes.as<u32>(), E.blkhdr.as<u32>(), fast ? 1 : 0))) return rc;
    if ((rc = launch_block_layout(st, d_chunks, n_chunks, d_blocks, d_cout, d_adler))) return rc;
    if ((rc = launch_zero_edges(st, d_chunks, d_blk_chunk, (int)nblk, d_blocks, d_cout, d_out))) return rc;      // (the words the packer ORs into)
    E.t_mark(st, "block_trees");
    if ((rc = launch_block_pack(st, d_stream, d_chunks, d_blk_chunk, (int)nblk, d_tokens, d_blocks, E.blkcodes.as<u32>(),
                                E.blkhdr.as<u32>(), d_cout, d_out, level))) return rc;
    E.t_mark(st, "block_pack");
    std::vector<ChunkOut> h_cout(n_chunks);
    MTS_HIP(hipMemcpyAsync(h_cout.data(), d_cout, sizeof(ChunkOut) * n_chunks, hipMemcpyDeviceToHost, st));
    MTS_HIP(hipStreamSynchronize(st));
    E.t_collect(accumulate_times);
    for (int i = 0; i < n_chunks; i++) out_sizes[i] = (long)h_cout[i].nbytes;
    if (tap) {
        // single-chunk debug taps
        const u32 n = cd[0].n;
        if (tap->t_full && n) {
            // (the tap had the match stage write the side table for every position)
            std::vector<u32> hf(n), hq(n);
            MTS_HIP(hipMemcpy(hf.data(), d_tables + cd[0].stream_off, 4 * (size_t)n, hipMemcpyDeviceToHost));
            MTS_HIP(hipMemcpy(hq.data(), d_quarter + cd[0].stream_off, 4 * (size_t)n, hipMemcpyDeviceToHost));
            auto unpack = [](u32 e) -> unsigned { return (e & 0x7fffu) ? ((((e >> 15) & 0xffu) + MIN_MATCH) << 16) | (e & 0x7fffu) : 0u; };
            for (u32 i = 0; i < n; i++) {
                tap->t_full[i] = unpack(hf[i]);
                tap->t_quarter[i] = unpack(hq[i]);
                // the flags must say what the two results say
                const bool differs = hq[i] != (hf[i] & 0x7fffffu);
                const u32 fl = hf[i] >> 23;
                if ((fl != 0) != differs || (fl == 2) != (differs && (tap->t_quarter[i] >> 16) > (u32)cfg.good)) {
                    set_error("table entry %u: flags %u do not describe full %08x / quarter %08x", i, fl, hf[i], hq[i]);
                    return MTS_E_INTERNAL;
                }
            }
        }
        if (tap->tokens) {
            const u32 nt = h_cout[0].ntok;
            if (nt) MTS_HIP(hipMemcpy(tap->tokens, d_tokens + cd[0].tok_off, 4 * (size_t)nt, hipMemcpyDeviceToHost));
            *tap->n_tokens = nt;
        }
    }
    return MTS_OK;
}

// split a call into sub-batches that fit the workspace budget (stream bytes per sub-batch) and the grid (several kernels
// take the chunk index from blockIdx.y, which ends at 65535)
constexpr int MAX_BATCH_CHUNKS = 32768;
static size_t batch_budget_bytes(bool in_order_walk = false)
{
    const char *e = getenv("MTS_BATCH_BYTES");               // read per call: tests force small sub-batches with it
    // 3 GiB of stream -> ~75 GiB of workspace.  Levels 1..3: 6 GiB (17 bytes of workspace per byte + the candidate lists: ~110
    // GiB) -- their in-order walk takes as long for one chunk as for 256, so fewer, larger sub-batches are what counts there
    size_t v = e ? (size_t)atoll(e) : ((size_t)(in_order_walk ? 6 : 3) << 30);
    if (v < (1u << 20)) v = 1u << 20;
    return v;
}

static int dev_compress(Engine &E, hipStream_t st, const void *d_raw, int nc, int sz, const long *bounds, int n_chunks,
                        int flags, int level, u8 *d_out, const long *slot_off, long *out_sizes, bool add_times = false)
{
    if (level == -1) level = 6;
    if (level < 1 || level > 9) { set_error("level %d out of range", level); return MTS_E_ARG; }
    if (int rc = check_items(sz, flags)) return rc;
    if (nc <= 0 || n_chunks < 0) return MTS_E_ARG;
    MTS_HIP(hipSetDevice(E.dev));
    const size_t budget = batch_budget_bytes(level < 4);
    const u64 row_bytes = (u64)nc * sz;
    const std::vector<int> bb = cut_batches([&](int j) { return (size_t)(bounds[j + 1] - bounds[j]) * row_bytes; }, n_chunks, budget, MAX_BATCH_CHUNKS);
    for (size_t b = 0; b + 1 < bb.size(); b++) {
        const int i = bb[b], j = bb[b + 1];
        const u8 *raw = (const u8 *)d_raw + (u64)(bounds[i] - bounds[0]) * row_bytes;
        const int rc = compress_batch(E, st, raw, false, nc, sz, bounds + i, j - i, flags, level, d_out, slot_off + i, out_sizes + i,
                                      add_times || b > 0, nullptr);
        if (rc) return rc;
    }
    if (n_chunks == 0) E.n_stage_done = 0;
    return MTS_OK;
}


// ------------------------------------------------------------------------------------------------
// decompress pipeline over one sub-batch (device resident)
// ------------------------------------------------------------------------------------------------
static int decompress_batch(Engine &E, hipStream_t st, const u8 *d_cdata, const long *c_off, const long *c_len,
                            const long *n_rows, int n_chunks, int nc, int sz, int flags, u8 *d_out, const long *out_off,
                            int *status, int times /* 0: these stages replace the recorded ones, 1: are added, 2: are not recorded */,
                            u8 *stream_copy_host /* debug: first chunk's stream */,
                            int nc_full = 0 /* > nc: the chunks have nc_full channels and only the first nc are decoded */,
                            bool size_verdict = true /* a chunk of another size than expected gets its check value looked at */)
{
    if (nc_full <= nc) nc_full = 0;
    // ---- plan ----
    const InflatePlan P(c_off, c_len, n_rows, out_off, n_chunks, nc, sz, nc_full, sizeof(InfResult));
    if (P.error[0]) { set_error("%s", P.error); return MTS_E_ARG; }
    const InflateKnobs K = inflate_knobs();
    const InflateScratch L = inflate_scratch(P, K);
    const std::vector<u64> &so = P.so;
    const std::vector<u32> &nn = P.nn;
    const u32 max_rows = P.max_rows;
    // ---- workspace ----
    int rc;
    if ((rc = E.stream.ensure(P.stream_bytes()))) return rc;
    if ((rc = E.tokens.ensure(P.token_bytes()))) return rc;
    if ((rc = E.inf_desc.ensure(P.o_end + 256))) return rc;
    if ((rc = E.adler.ensure(sizeof(u64) * 2 * n_chunks + 256))) return rc;
    if ((rc = E.segsums.ensure(cumsum_scratch_bytes(n_chunks, max_rows, nc)))) return rc;
    if ((rc = E.init_events())) return rc;
    if ((rc = E.inf_scratch.ensure(L.end + 256))) return rc;      // (a batch's last allocation: where buffers lie has shown in stage times)
    u8 *dp = E.inf_desc.as<u8>();
    InfChunk *d_ic = (InfChunk *)(dp + P.o_ic);
    InfResult *d_res = (InfResult *)(dp + P.o_res);
    u64 *d_so = (u64 *)(dp + P.o_so);
    u64 *d_oo = (u64 *)(dp + P.o_oo);
    u32 *d_rows = (u32 *)(dp + P.o_rows);
    int *d_status = (int *)(dp + P.o_status);
    // ---- upload (what the host fills lies in a row: one copy) ----
    {
        std::vector<u8> &hst = E.host_stage[0];
        hst.assign(P.host_bytes, 0);
        P.fill(hst.data());
        MTS_HIP(hipMemcpyAsync(dp, hst.data(), P.host_bytes, hipMemcpyHostToDevice, st));
    }
    // ---- launch ----
    E.t_begin(st);
    if ((rc = launch_inflate(E, st, d_cdata, d_ic, P, L, K, E.stream.as<u8>(), E.tokens.as<u32>(), d_res, E.adler.as<u64>(), d_status))) return rc;
    if (d_out) {
        if ((rc = launch_cumsum_transpose(st, E.stream.p, d_out, d_so, d_oo, d_rows, d_status, n_chunks, max_rows, nc, sz, flags,
                                          E.segsums.p))) return rc;
        E.t_mark(st, "cumsum_transpose");
    }
    MTS_HIP(hipMemcpyAsync(status, d_status, 4 * (size_t)n_chunks, hipMemcpyDeviceToHost, st));
    MTS_HIP(hipStreamSynchronize(st));
    if (times != 2) E.t_collect(times == 1);
    if (stream_copy_host && nn[0]) MTS_HIP(hipMemcpy(stream_copy_host, E.stream.as<u8>() + so[0], nn[0], hipMemcpyDeviceToHost));
    // A stream that parses to its end, but to another size than the caller expects: the reference inflates it whole and has its
    // adler32 checked before it looks at the size (zlib.decompress raises at mtscomp.py:618-621, the assert comes at :628).  The
    // same order here: such a chunk is inflated once more, alone, at the size it really has, for its check value only -- a
    // valid stream keeps BADSIZE (the assert), a damaged one becomes CORRUPT (the IOError).  It never happens on a file the Writer
    // made; what it costs does not matter.
    if (size_verdict && !nc_full) {
        std::vector<std::pair<int, u32>> odd;
        for (int i = 0; i < n_chunks; i++)
            if (status[i] == MTS_CHUNK_BADSIZE) {
                InfResult r;
                MTS_HIP(hipMemcpy(&r, d_res + i, sizeof(r), hipMemcpyDeviceToHost));
                odd.push_back({i, r.n_out});
            }
        for (const auto &o : odd) {                                  // (from here on the engine's buffers are the verdict passes')
            const int i = o.first;
            if (o.second >= (1u << 31)) { status[i] = MTS_CHUNK_CORRUPT; continue; }     // beyond what a pass can hold: damage, by all odds
            const long rows1 = (long)o.second, off0 = 0;
            int st1 = MTS_CHUNK_CORRUPT;
            const int rc1 = decompress_batch(E, st, d_cdata, c_off + i, c_len + i, &rows1, 1, 1, 1, 0, nullptr, &off0, &st1, 2, nullptr, 0, false);
            if (rc1 == MTS_E_NOMEM) { status[i] = MTS_CHUNK_CORRUPT; continue; }         // (the same call: a size nobody wrote)
            if (rc1) return rc1;
            if (st1 != MTS_CHUNK_OK) status[i] = MTS_CHUNK_CORRUPT;
        }
    }
    return MTS_OK;
}

int dev_decompress(Engine &E, hipStream_t st, const u8 *d_cdata, const long *c_off, const long *c_len, const long *n_rows,
                   int n_chunks, int nc, int sz, int flags, u8 *d_out, const long *out_off, int *status, int nc_full, bool add_times)
{
    if (int rc = check_items(sz, flags)) return rc;
    if (nc <= 0 || n_chunks < 0) return MTS_E_ARG;
    for (int i = 0; i < n_chunks; i++)              // (K2 stores whole items; any multiple of the item size is allowed)
        if (((uintptr_t)d_out + (u64)out_off[i]) % (unsigned)sz) {
            set_error("chunk %d: output address (d_out + offset %ld) is not a multiple of the item size %d", i, out_off[i], sz);
            return MTS_E_ARG;
        }
    MTS_HIP(hipSetDevice(E.dev));
    const size_t budget = batch_budget_bytes() * 4;          // inflate needs ~5 bytes of workspace per byte
    const u64 row_bytes = (u64)(nc_full > nc ? nc_full : nc) * sz;
    const std::vector<int> bb = cut_batches([&](int j) { return (size_t)n_rows[j] * row_bytes; }, n_chunks, budget, MAX_BATCH_CHUNKS);
    for (size_t b = 0; b + 1 < bb.size(); b++) {
        const int i = bb[b], j = bb[b + 1];
        const int rc = decompress_batch(E, st, d_cdata, c_off + i, c_len + i, n_rows + i, j - i, nc, sz, flags, d_out, out_off + i,
                                        status + i, add_times || b > 0 ? 1 : 0, nullptr, nc_full);
        if (rc) return rc;
    }
    if (n_chunks == 0) E.n_stage_done = 0;
    return MTS_OK;
}

}  // namespace mts

using namespace mts;

// ================================================================================================
// extern "C"
// ================================================================================================
extern "C" {

int mts_dev_compress_chunks(int device, void *stream, const void *d_raw, int n_channels, int itemsize,
                            const long *chunk_bounds, int n_chunks, int flags, int level, unsigned char *d_out,
                            const long *out_slot_offsets, long *out_sizes)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(E->mu);                       // (dev_compress makes the device current, after its checks)
    return dev_compress(*E, (hipStream_t)stream, d_raw, n_channels, itemsize, chunk_bounds, n_chunks, flags, level, d_out,
                        out_slot_offsets, out_sizes);
}

// The host entry points work piece by piece (run_pieces, engine.h; the pieces: pipe_pieces): while the device compresses / inflates
// piece k, one host thread copies piece k + 1 in and another copies the result of piece k - 1 out.
int mts_compress_chunks(int device, const void *raw, int n_channels, int itemsize, const long *chunk_bounds, int n_chunks,
                        int flags, int level, unsigned char *out, const long *out_slot_offsets, long *out_sizes)
{
    EngineLock E;
    int rc = E.open(device);
    if (rc) return rc;
    if (n_chunks <= 0) return n_chunks == 0 ? MTS_OK : MTS_E_ARG;
    if ((rc = E.enter())) return rc;
    const u64 row_bytes = (u64)n_channels * itemsize;
    const u64 raw_bytes = (u64)(chunk_bounds[n_chunks] - chunk_bounds[0]) * row_bytes;
    std::vector<long> slots(n_chunks);
    u64 total = 0;
    for (int i = 0; i < n_chunks; i++) {
        slots[i] = (long)total;
        total += align_up((u64)compress_bound((long)((u64)(chunk_bounds[i + 1] - chunk_bounds[i]) * row_bytes)), 256);
    }
    if ((rc = E->h_in.ensure(raw_bytes + 256))) return rc;
    if ((rc = E->h_out.ensure(total + 256))) return rc;
    const std::vector<int> pb = pipe_pieces(chunk_bounds, true, n_chunks, row_bytes);
    const int dev = E->dev;
    auto raw_off = [&](int i) { return (u64)(chunk_bounds[i] - chunk_bounds[0]) * row_bytes; };
    return run_pieces((int)pb.size() - 1,
        [&](int k) -> int {                                      // the raw rows of piece k (on the calling or on a helper thread)
            MTS_HIP(hipSetDevice(dev));
            const u64 off = raw_off(pb[k]), len = raw_off(pb[k + 1]) - off;
            return len ? staged_h2d(*E, E->h_in.as<u8>() + off, (const u8 *)raw + off, len) : MTS_OK;
        },
        [&](int k) -> int {
            return dev_compress(*E, nullptr, E->h_in.as<u8>() + raw_off(pb[k]), n_channels, itemsize, chunk_bounds + pb[k], pb[k + 1] - pb[k], flags,
                                level, E->h_out.as<u8>(), slots.data() + pb[k], out_sizes + pb[k], k > 0);
        },
        [&](int k) -> int {                                      // the streams of piece k, each to its slot in the caller's buffer
            MTS_HIP(hipSetDevice(dev));
            std::vector<CopyItem> segs;
            for (int i = pb[k]; i < pb[k + 1]; i++)
                if (out_sizes[i] > 0) segs.push_back({out + out_slot_offsets[i], E->h_out.as<u8>() + slots[i], (size_t)out_sizes[i]});
            return staged_d2h_multi(*E, segs);
        });
}

int mts_dev_decompress_chunks(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets,
                              const long *c_lengths, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags,
                              void *d_out, const long *out_offsets, int *chunk_status)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(E->mu);                       // (dev_decompress makes the device current, after its checks)
    return dev_decompress(*E, (hipStream_t)stream, d_cdata, c_offsets, c_lengths, n_rows, n_chunks, n_channels, itemsize, flags,
                          (u8 *)d_out, out_offsets, chunk_status);
}

int mts_decompress_chunks(int device, const unsigned char *cdata, const long *c_offsets, const long *c_lengths,
                          const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, void *out,
                          const long *out_offsets, int *chunk_status)
{
    EngineLock E;
    int rc = E.open(device);
    if (rc) return rc;
    if (n_chunks <= 0) return n_chunks == 0 ? MTS_OK : MTS_E_ARG;
    if ((rc = E.enter())) return rc;
    const u64 row_bytes = (u64)n_channels * itemsize;
    std::vector<long> ooff(n_chunks);
    u64 otot = 0;
    for (int i = 0; i < n_chunks; i++) {
        if (c_lengths[i] < 0 || n_rows[i] < 0) return MTS_E_ARG;
        ooff[i] = (long)otot; otot += align_up((u64)n_rows[i] * row_bytes, 256);
    }
    RangeStaging S(c_offsets, c_lengths, n_chunks);              // where the compressed bytes lie in E->h_in, and how they get there
    if ((rc = E->h_in.ensure(S.ctot + 256))) return rc;
    if ((rc = E->h_out.ensure(otot + 256))) return rc;
    S.pb = S.piecewise() ? pipe_pieces(n_rows, false, n_chunks, row_bytes) : std::vector<int>{0, n_chunks};
    const std::vector<int> &pb = S.pb;
    const int dev = E->dev;
    return run_pieces((int)pb.size() - 1,
        [&](int k) -> int {
            MTS_HIP(hipSetDevice(dev));
            for (const StageCopy &c : S.copies(k))
                if (const int rc1 = staged_h2d(*E, E->h_in.as<u8>() + c.dst, cdata + c.src, (size_t)c.len)) return rc1;
            return MTS_OK;
        },
        [&](int k) -> int {
            return dev_decompress(*E, nullptr, E->h_in.as<u8>(), S.coff.data() + pb[k], c_lengths + pb[k], n_rows + pb[k], pb[k + 1] - pb[k], n_channels,
                                  itemsize, flags, E->h_out.as<u8>(), ooff.data() + pb[k], chunk_status + pb[k], 0, k > 0);
        },
        [&](int k) -> int {
            MTS_HIP(hipSetDevice(dev));
            std::vector<CopyItem> segs;
            for (int i = pb[k]; i < pb[k + 1]; i++)
                if (chunk_status[i] == MTS_CHUNK_OK && n_rows[i])
                    segs.push_back({(u8 *)out + out_offsets[i], E->h_out.as<u8>() + ooff[i], (size_t)((u64)n_rows[i] * row_bytes)});
            return staged_d2h_multi(*E, segs);
        });
}

// ---- debug taps ---------------------------------------------------------------------------------
int mts_debug_inflate(int device, const unsigned char *zbytes, long zlen, unsigned char *out, long out_cap, long *out_len, int *status)
{
    EngineLock E;
    int rc = E.open(device);
    if (rc) return rc;
    if (zlen < 0 || out_cap < 0) return MTS_E_ARG;
    if ((rc = E.enter())) return rc;
    if ((rc = E->h_in.ensure((u64)zlen + 256))) return rc;
    if (zlen) MTS_HIP(hipMemcpy(E->h_in.p, zbytes, (size_t)zlen, hipMemcpyHostToDevice));
    // the expected size is the caller's out_cap: status BADSIZE when the stream inflates to anything else
    const long coff = 0, clen = zlen, rows = out_cap, ooff = 0;
    rc = decompress_batch(*E, nullptr, E->h_in.as<u8>(), &coff, &clen, &rows, 1, 1, 1, 0, nullptr, &ooff, status, 0, out);
    if (rc) return rc;
    if (out_len) *out_len = *status == MTS_CHUNK_OK ? out_cap : 0;
    return MTS_OK;
}

static int debug_compress_stream(int device, const void *stream_bytes, long n, int level, unsigned char *out, long out_cap,
                                 long *out_len, DebugTap *tap)
{
    EngineLock E;
    int rc = E.open(device);
    if (rc) return rc;
    if (level == -1) level = 6;
    if (level < 1 || level > 9) return MTS_E_ARG;
    if (level < 4 && tap && tap->t_full) return MTS_E_UNSUPPORTED;      // (deflate_fast has no candidate tables)
    if (n < 0 || n >= (1l << 31)) return MTS_E_ARG;
    if ((rc = E.enter())) return rc;
    const u64 bound = align_up((u64)compress_bound(n), 256);
    if ((rc = E->h_in.ensure((u64)n + 2 * STREAM_PAD))) return rc;
    if ((rc = E->h_out.ensure(bound + 256))) return rc;
    MTS_HIP(hipMemset(E->h_in.p, 0, (u64)n + 2 * STREAM_PAD));
    if (n) MTS_HIP(hipMemcpy(E->h_in.p, stream_bytes, (size_t)n, hipMemcpyHostToDevice));
    const long bounds[2] = {0, n};
    const long slot = 0;
    long size = 0;
    rc = compress_batch(*E, nullptr, E->h_in.as<u8>(), true, 1, 1, bounds, 1, 0, level, E->h_out.as<u8>(), &slot, &size, false, tap);
    if (rc) return rc;
    if (out_len) *out_len = size;
    if (out) {
        if (size > out_cap) return MTS_E_ARG;
        MTS_HIP(hipMemcpy(out, E->h_out.p, (size_t)size, hipMemcpyDeviceToHost));
    }
    return MTS_OK;
}

int mts_debug_match_tables(int device, const void *stream_bytes, long n, int level, unsigned *t_full, unsigned *t_quarter)
{
    DebugTap tap; tap.t_full = t_full; tap.t_quarter = t_quarter;
    return debug_compress_stream(device, stream_bytes, n, level, nullptr, 0, nullptr, &tap);
}
int mts_debug_tokens(int device, const void *stream_bytes, long n, int level, unsigned short *tokens, long *n_tokens)
{
    DebugTap tap; tap.tokens = tokens; tap.n_tokens = n_tokens;
    return debug_compress_stream(device, stream_bytes, n, level, nullptr, 0, nullptr, &tap);
}
int mts_debug_deflate(int device, const void *stream_bytes, long n, int level, unsigned char *out, long out_cap, long *out_len)
{
    return debug_compress_stream(device, stream_bytes, n, level, out, out_cap, out_len, nullptr);
}

}  // extern "C"
