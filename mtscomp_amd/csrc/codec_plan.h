// How the codec is fed: the part that decides and touches no device.  The descriptors the kernels read, where a batch's streams,
// tokens, tiles, segments and block slots lie and which arrays share a compress workspace (CompressPlan, InflatePlan), every region of
// the inflate kernels' scratch (InflateScratch), how a call is cut into sub-batches (cut_batches), how a workspace is carved (WsLayout),
// and where the compressed bytes of a call lie in the staging buffer (stage_runs / run_copies, RangeStaging).  The header includes the C/C++ standard library only, so tests/plan_check.cpp sweeps all of it on the CPU;
// codec.hip and cache.hip allocate, copy and launch around it.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

// (what the plans and the files around them share with each other only: not among the symbols the library exports)
#define MTS_LOCAL __attribute__((visibility("hidden")))

namespace mts {

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

// (constexpr: callable from kernels as well)
constexpr u64 align_up(u64 x, u64 a) { return (x + a - 1) / a * a; }

// zlib's compressBound
MTS_LOCAL inline long compress_bound(long n) { return n + (n >> 12) + (n >> 14) + (n >> 25) + 13; }

constexpr int BLOCK_TOKENS = 16383;        // lit_bufsize - 1 (zlib 1.2.11, memLevel 8)

// ---- stream layout ------------------------------------------------------------------------------
// Every chunk's transformed byte stream lives in one device buffer at a 256-B aligned offset and is
// followed by >= STREAM_PAD zero bytes, so kernels may over-read past a stream's end.
constexpr int STREAM_PAD = 512;
constexpr int STREAM_ALIGN = 256;

// ---- match stage tiling ---------------------------------------------------------------------------
// A tile's history (HALO) is sorted and staged again by the next tile, so bigger tiles mean less work.  While every
// workgroup read its own window through L2, big tiles lost to locality (round 1: 64..96 Ki 41-42 ms, 160 Ki 53, 224 Ki 60);
// with the workgroups of an XCD sharing a tile the window is L2 resident whatever its size and the biggest tile the 18-bit
// window-relative positions allow wins (match 31 -> 28.5 ms, sort 12.9 -> 11.4 from 96 Ki to 224 Ki).
// The 32-bit sort keys hold the window-relative position (REL_BITS allow windows up to 2^18) and the 7 hash bits
// the second radix pass still needs; the first pass takes its 8 bits straight from the bytes.
#ifndef MTS_REL_BITS
#define MTS_REL_BITS 18
#endif
constexpr int REL_BITS = MTS_REL_BITS;     // 18 or 19 (a match entry word holds rel : 9 bits : the low bits of byte 7)
constexpr int HALO = 32768;                // history a tile additionally needs (>= MAX_DIST)
constexpr int WIN = 1 << REL_BITS;         // hashed window of a tile
#ifndef MTS_TILE
#define MTS_TILE (WIN - HALO)
#endif
constexpr int TILE = MTS_TILE;             // positions a match-stage workgroup owns (229376 / 491520; anything up to WIN - HALO)
static_assert(TILE > 0 && TILE + HALO <= WIN && TILE % 64 == 0, "a tile and its history fit the window");

constexpr int SEG = 1024;                  // parse segment (positions per speculative walker); measured 512: 9.0, 1024: 8.5, 2048: 8.9, 4096: 9.3 ms (fixpoint + emit)

// The match stage's sink, where its lanes that own no position store (match.hip): behind the flag words of the adler workspace, from
// word MATCH_SINK_WORD0 after the first flag word (256 bytes in) on, a line of MATCH_SINK_LINE_WORDS words per workgroup, the workgroups
// taking the MATCH_SINK_LINES lines in turn
constexpr int MATCH_SINK_BYTES = 65536;
constexpr int MATCH_SINK_WORD0 = 63;
constexpr int MATCH_SINK_LINE_WORDS = 64;
constexpr int MATCH_SINK_LINES = MATCH_SINK_BYTES / (4 * MATCH_SINK_LINE_WORDS);
static_assert((MATCH_SINK_LINES & (MATCH_SINK_LINES - 1)) == 0, "a workgroup finds its line with a mask");

// one match-stage tile
struct TileDesc {
    u64 stream_off;      // byte offset of the chunk's stream in the stream buffer
    u64 sorted_off;      // entry offset of this tile's sorted window in the sort buffers
    u32 n;               // stream length (bytes) of the chunk
    u32 a;               // first owned position
    u32 w;               // window start (= max(0, a - HALO))
    u32 wlen;            // hashed positions in the window: positions [w, w + wlen), all <= n - 3
    u32 own_end;         // owned positions are [a, own_end)
    u32 chunk;
};

// per-chunk descriptor of a compress batch
struct ChunkDesc {
    u64 stream_off;      // into the stream buffer
    u64 tok_off;         // into the token buffer (capacity n + 1 tokens)
    u64 out_off;         // byte offset of the chunk's slot in the output buffer (16-B aligned)
    u64 raw_off;         // byte offset of the chunk's first row in the raw input
    u32 n;               // stream bytes
    u32 n_rows;
    u32 seg0;            // first parse segment (global index)
    u32 nseg;
    u32 blk0;            // first block slot (global index); capacity n / 16383 + 2
    u32 blk_cap;
    u32 tile0;           // first match-stage tile of the chunk (global index)
    u32 pad;
};

// per-chunk descriptor of an inflate batch
struct InfChunk {
    u64 c_off;           // compressed bytes offset in d_cdata
    u64 c_len;
    u64 stream_off;      // where the inflated stream goes (stream buffer)
    u64 tok_off;         // token buffer offset (capacity n + 2)
    u32 n_expect;        // expected inflated size (the whole chunk)
    u32 n_need;          // 0, or: only the first n_need bytes of the stream are wanted (the leading channels of a channel-major
                         // chunk, for Reader[rows, columns]): the block chain stops once it has them, c_len may be a prefix of
                         // the chunk's bytes, no adler32 check; MTS_CHUNK_NEEDMORE when the bytes given do not get that far
};

// (the kernels read these bytes)
static_assert(sizeof(TileDesc) == 40 && offsetof(TileDesc, sorted_off) == 8 && offsetof(TileDesc, n) == 16 && offsetof(TileDesc, chunk) == 36, "TileDesc layout");
static_assert(sizeof(ChunkDesc) == 64 && offsetof(ChunkDesc, raw_off) == 24 && offsetof(ChunkDesc, n) == 32 && offsetof(ChunkDesc, tile0) == 56, "ChunkDesc layout");
static_assert(sizeof(InfChunk) == 40 && offsetof(InfChunk, stream_off) == 16 && offsetof(InfChunk, n_expect) == 32 && offsetof(InfChunk, n_need) == 36, "InfChunk layout");

// ---- a workspace: regions of 256-aligned sizes one behind the other, the outputs last.  An output lies in the workspace only when
// the caller's buffer is host memory (out_on_host: it is copied there at the end); a device buffer is written directly.
struct WsLayout {
    bool out_on_host;
    size_t end = 0;
    size_t take(u64 bytes) { const size_t o = end; end += align_up(bytes, 256); return o; }
    size_t take_out(u64 bytes) { return out_on_host ? take(bytes) : end; }
    template <class T> T *out(u8 *ws, size_t off, T *caller) const { return out_on_host ? (T *)(ws + off) : caller; }
};

// ---- sub-batches: chunks [b[k], b[k + 1]) make batch k.  A batch takes chunks while their bytes fit the budget and their number
// max_chunks; its first chunk it takes whatever its size (a chunk bigger than the budget is a batch of its own, a chunk of no bytes
// never stalls the cut)
template <class BytesOf>
std::vector<int> cut_batches(BytesOf &&bytes_of, int n, size_t budget, int max_chunks)
{
    std::vector<int> b = {0};
    for (int i = 0; i < n;) {
        int j = i;
        size_t acc = 0;
        while (j < n) {
            const size_t bytes = bytes_of(j);
            if (j > i && (acc + bytes > budget || j - i >= max_chunks)) break;
            acc += bytes; j++;
        }
        b.push_back(i = j);
    }
    return b;
}

// ---- a compress batch ---------------------------------------------------------------------------------------------------------------
// what the plan takes from the device code: sizes of records it does not look into, and the workspaces the kernels size themselves
struct CompressDims {
    size_t (*hash_sort_ws_bytes)(int n_tiles);
    size_t (*parse_marks_words)(size_t n_segs);
    size_t parse_cp_words, block_rec_bytes, chunk_out_bytes, blk_code_words, blk_hdr_words, match_sink_bytes;      // (the last: MATCH_SINK_BYTES)
};

// Chunk i's stream lies at cd[i].stream_off (STREAM_ALIGN-aligned, >= STREAM_PAD bytes behind it before the next begins or the
// buffer ends), its tokens at tok_off (room for n + 1), its raw rows at raw_off, its segments [seg0, seg0 + ceil(n / SEG)), its block
// slots [blk0, blk0 + n / BLOCK_TOKENS + 2), its tiles from tile0.  A chunk's tiles own [a, own_end) = TILE positions each, in order,
// and hash the window [w, w + wlen): HALO positions of history, then the owned positions that still have three bytes (<= n - 3).
// Each tile's sorted window is a 64-aligned region of the sort buffers.  segbuf, blk, adler and misc each hold several arrays one
// behind the other: seg, bk, ad and mi say where (they are not re-aligned: the match stage's time has followed buffer placement).
struct MTS_LOCAL CompressPlan {
    char error[96] = "";                                      // not empty: a bad argument, nothing else is valid
    std::vector<ChunkDesc> cd;
    std::vector<TileDesc> tiles;
    u32 nseg = 0, nblk = 0, max_rows = 0, max_n = 0, max_nseg = 0;
    u64 stream_bytes = 0, tok_words = 0;
    size_t sort_n = 0, table_words = 0;
    // workspaces, in bytes
    size_t sort_a = 0, sort_b = 0, sort_ws = 0, tables = 0, tokens = 0, segbuf = 0, blk = 0, blkcodes = 0, blkhdr = 0, desc = 0, adler = 0, misc = 0;
    size_t o_chunks = 0, o_tiles = 0, o_cout = 0;             // the regions of desc
    struct { size_t entry, exit_a, exit_b, cnt, tokbase, seg_chunk, seg_start, cp, end; } seg = {};      // segbuf, in words: nseg + 64 entries each, cp parse_cp_words per entry
    struct { size_t blocks, chunk, in_start, end; } bk = {};      // blk, in bytes: nblk + 1 records, then as many words for the slot's chunk and its first input byte
    struct { size_t sums, changed, flags, sink, end; } ad = {};   // adler, in bytes: two sums per chunk, the parse's flag word, the match stage's, its sink
    struct { size_t so, nn, end; } mi = {};                       // misc, in bytes (raw_is_stream: the streams' offsets and sizes for the check value)

    CompressPlan(const long *bounds, int n_chunks, u64 row_bytes, bool raw_is_stream, const long *slot_off, int level, const CompressDims &D) : cd(n_chunks)
    {
        u64 soff = 0, sorted_off = 0;
        for (int i = 0; i < n_chunks; i++) {
            const u64 rows = (u64)(bounds[i + 1] - bounds[i]);
            const u64 n = raw_is_stream ? rows : rows * row_bytes;
            if (n >= (1ull << 31)) { snprintf(error, sizeof error, "chunk %d is %llu bytes; chunks must be < 2 GiB", i, (unsigned long long)n); return; }
            ChunkDesc &c = cd[i];
            c.stream_off = soff; c.tok_off = tok_words; c.out_off = (u64)slot_off[i];
            c.raw_off = (u64)(bounds[i] - bounds[0]) * (raw_is_stream ? 1 : row_bytes);
            c.n = (u32)n; c.n_rows = (u32)rows;
            c.seg0 = nseg; c.nseg = (u32)((n + SEG - 1) / SEG);
            c.blk0 = nblk; c.blk_cap = (u32)(n / BLOCK_TOKENS + 2);
            if (c.out_off & 15) { snprintf(error, sizeof error, "output slot %d is not 16-byte aligned", i); return; }
            nseg += c.nseg; nblk += c.blk_cap;
            if (rows > max_rows) max_rows = (u32)rows;
            if (c.n > max_n) max_n = c.n;
            if (c.nseg > max_nseg) max_nseg = c.nseg;
            c.tile0 = (u32)tiles.size(); c.pad = 0;
            for (u64 a = 0; a < n; a += TILE) {
                TileDesc t;
                t.stream_off = soff; t.sorted_off = sorted_off; t.n = (u32)n; t.a = (u32)a;
                t.w = (u32)(a >= (u64)HALO ? a - HALO : 0);
                t.own_end = (u32)(a + TILE < n ? a + TILE : n);
                // (a position is hashed with the two bytes behind it: the last is n - 3; a chunk shorter than three bytes has none)
                const u64 hashed_end = n >= 3 ? (t.own_end < n - 2 ? t.own_end : n - 2) : 0;
                t.wlen = hashed_end > t.w ? (u32)(hashed_end - t.w) : 0;
                t.chunk = (u32)i;
                sorted_off += align_up(t.wlen, 64);
                tiles.push_back(t);
            }
            soff += align_up(n + STREAM_PAD, STREAM_ALIGN);
            tok_words += n + 1;
        }
        stream_bytes = soff + STREAM_PAD;
        sort_n = align_up(sorted_off + 64, 64);               // 32-bit keys
        // (the first pass's keys are dead once the sort is done: the parse keeps its marks there)
        const size_t marks_words = D.parse_marks_words((size_t)nseg + 64);
        sort_a = (sort_n > marks_words ? sort_n : marks_words) * 4;
        sort_b = sort_n * 4;
        sort_ws = D.hash_sort_ws_bytes((int)tiles.size());
        // one word per position (levels 1..3: the inverse map) + for levels 4..9 the side table of the quarter-budget results, which is
        // written and read at a fraction of a percent of the positions only
        table_words = align_up(stream_bytes + 64, 64);
        tables = table_words * 4 * (level < 4 ? 1 : 2);
        tokens = (tok_words + 64) * 4;
        const size_t SN = (size_t)nseg + 64, BN = (size_t)nblk + 1;
        seg = {0, SN, 2 * SN, 3 * SN, 4 * SN, 5 * SN, 6 * SN, 7 * SN, (7 + D.parse_cp_words) * SN};
        segbuf = seg.end * 4 + 256;
        bk = {0, BN * D.block_rec_bytes, BN * (D.block_rec_bytes + 4), BN * (D.block_rec_bytes + 8)};
        blk = bk.end + 256;
        blkcodes = ((size_t)nblk + 1) * D.blk_code_words * 4;
        blkhdr = ((size_t)nblk + 1) * D.blk_hdr_words * 4;
        WsLayout L{false};
        o_chunks = L.take(sizeof(ChunkDesc) * n_chunks); o_tiles = L.take(sizeof(TileDesc) * (tiles.size() + 1)); o_cout = L.take(D.chunk_out_bytes * n_chunks);
        desc = L.end;
        ad.sums = 0; ad.changed = sizeof(u64) * 2 * n_chunks; ad.flags = ad.changed + 4; ad.sink = ad.flags + 4 * MATCH_SINK_WORD0;
        ad.end = ad.sink + D.match_sink_bytes;
        adler = ad.changed + 256 + D.match_sink_bytes;
        mi = {0, 8 * (size_t)n_chunks, 12 * (size_t)n_chunks};
        misc = mi.end + 64;
    }

    // the index arrays, which depend on the chunk sizes only: per segment its chunk, then its start position; per block slot its chunk
    void index_arrays(std::vector<u32> &h_seg, std::vector<u32> &h_blk_chunk) const
    {
        h_seg = std::vector<u32>(2 * (size_t)nseg); h_blk_chunk = std::vector<u32>((size_t)nblk + 1);
        for (size_t i = 0; i < cd.size(); i++) {
            for (u32 k = 0; k < cd[i].nseg; k++) { h_seg[cd[i].seg0 + k] = (u32)i; h_seg[nseg + cd[i].seg0 + k] = k * SEG; }
            for (u32 k = 0; k < cd[i].blk_cap; k++) h_blk_chunk[cd[i].blk0 + k] = (u32)i;
        }
    }

    // levels 1..3: the candidate lists are made a phase (W positions of every chunk, K words each) at a time into two buffers that
    // together keep to the budget; W is a multiple of 256, and there are at least 8 phases where the longest chunk allows: only the
    // first lists are waited for
    static u64 phase_width(u64 budget, int n_chunks, u64 K, u32 max_n)
    {
        u64 W = budget / 2 / ((u64)n_chunks * K * 4) / 256 * 256;
        if (W < 256) W = 256;
        if (W > align_up(max_n, 256)) W = align_up(max_n, 256);
        if (W > 1024 && W * 8 > max_n) W = align_up((max_n + 7) / 8, 256);
        return W;
    }
};

// ---- an inflate batch ---------------------------------------------------------------------------------------------------------------
// Streams as in a compress batch; a chunk's tokens lie at a 16-byte aligned tok_off (vector loads) with room for n + 2.  What the host
// fills lies in a row at the head of the descriptor buffer -- ic, so, nn, oo, rows: host_bytes, one copy -- with the results and the
// verdicts behind it.
struct MTS_LOCAL InflatePlan {
    char error[96] = "";
    std::vector<InfChunk> ic;
    std::vector<u64> so, oo;
    std::vector<u32> nn, rows;
    u64 soff = 0, toff = 0;
    u32 max_n = 0, max_rows = 0;
    size_t o_ic = 0, o_so = 0, o_nn = 0, o_oo = 0, o_rows = 0, o_res = 0, o_status = 0, o_end = 0, host_bytes = 0;

    // nc_full > 0: the chunks have nc_full channels and only the first nc are wanted
    InflatePlan(const long *c_off, const long *c_len, const long *n_rows, const long *out_off, int n_chunks, int nc, int sz, int nc_full, size_t inf_result_bytes)
        : ic(n_chunks), so(n_chunks), oo(n_chunks), nn(n_chunks), rows(n_chunks)
    {
        const u64 row_bytes = (u64)(nc_full ? nc_full : nc) * sz;
        for (int i = 0; i < n_chunks; i++) {
            const u64 n = (u64)n_rows[i] * row_bytes;
            if (n >= (1ull << 31)) { snprintf(error, sizeof error, "chunk %d is %llu bytes; chunks must be < 2 GiB", i, (unsigned long long)n); return; }
            ic[i].c_off = (u64)c_off[i]; ic[i].c_len = (u64)c_len[i];
            ic[i].stream_off = soff; ic[i].tok_off = toff; ic[i].n_expect = (u32)n;
            ic[i].n_need = nc_full ? (u32)((u64)n_rows[i] * nc * sz) : 0u;
            if (nc_full && ic[i].n_need == 0) ic[i].n_need = 1;      // (a chunk without rows: still a partial decode)
            so[i] = soff; oo[i] = (u64)out_off[i]; nn[i] = (u32)n; rows[i] = (u32)n_rows[i];
            if (n > max_n) max_n = (u32)n;
            if (n_rows[i] > (long)max_rows) max_rows = (u32)n_rows[i];
            soff += align_up(n + STREAM_PAD, STREAM_ALIGN);
            toff += align_up(n + 2, 4);
        }
        WsLayout L{false};
        o_ic = L.take(sizeof(InfChunk) * n_chunks); o_so = L.take(8 * (u64)n_chunks); o_nn = L.take(4 * (u64)n_chunks); o_oo = L.take(8 * (u64)n_chunks);
        o_rows = L.take(4 * (u64)n_chunks); o_res = L.take(inf_result_bytes * n_chunks); o_status = L.take(4 * (u64)n_chunks);
        o_end = L.end; host_bytes = o_res;
    }
    size_t stream_bytes() const { return soff + STREAM_PAD; }
    size_t token_bytes() const { return (toff + 64) * 4; }

    void fill(u8 *h) const                                    // host_bytes zeroed bytes
    {
        const size_t n = ic.size();
        memcpy(h + o_ic, ic.data(), sizeof(InfChunk) * n); memcpy(h + o_so, so.data(), 8 * n); memcpy(h + o_nn, nn.data(), 4 * n);
        memcpy(h + o_oo, oo.data(), 8 * n); memcpy(h + o_rows, rows.data(), 4 * n);
    }
};

// ---- the scratch of an inflate batch ----------------------------------------------------------------------------------------------------
// per-chunk bookkeeping of the fast path (a device array the host fills, one entry per chunk)
struct InfFast {
    u64 cand_off;                // first slot of this chunk in the candidate arrays
    u32 cand_cap;
    u32 true_off;                // first slot in the true-block array
    u32 true_cap;
    u32 pad;
};
static_assert(sizeof(InfFast) == 24 && offsetof(InfFast, cand_cap) == 8 && offsetof(InfFast, true_off) == 12 && offsetof(InfFast, true_cap) == 16, "InfFast layout");

// what the scratch plan takes from inflate.hip: sizes of records it does not look into, and the constants that size a region
struct InflateDims {
    size_t cand_res_bytes, true_blk_bytes, lz_plan_bytes;     // sizeof(CandRes), sizeof(TrueBlk), sizeof(LzPlan)
    u32 subcap, rowcap, rounds_max, gs_tile, lz_maxseg, lz_win, lz_flush, lz_flushers;
};

// Every region of the inflate kernels' scratch, 256-aligned, one behind the other in the order of the members.  Per chunk: cand_cap
// candidate slots from cand_off and twice as many true-block slots from true_off (fast), groups_of(n) group bases from gb[i] in gbase,
// tiles_of(n) tile bases from tb[i] in tile_base.  What the host fills -- so, nn, fast, gb_off, tb_off -- lies in a row at host_off:
// host_bytes, one copy (fill).  The resolver clears clear[0] and clear[1] before it runs: gflag and seg_adler, which lie in a row.
struct MTS_LOCAL InflateScratch {
    struct Region { const char *name; size_t off, bytes; };
    const InflatePlan &P;
    std::vector<Region> regions;                              // every take, in order: the sweep's view
    size_t so, nn, fast, gb_off, tb_off, cand_cnt, true_cnt, seq_flag, slot_chunk, tslot_chunk, cand_pos, cand_tmp, cres, tblk, subs, gbase, tile_base, surv,
        surv_cnt, plan, win;
    size_t rows_cells;           // pass A's token rows (u32) until pass B and k_inf_move_rows have run, then the resolver's cells (u16): the rows are dead by then
    size_t round_row, row_ctr, gflag, seg_adler, end;
    size_t host_off, host_bytes;
    struct { size_t off, bytes; } clear[2];
    u32 total_cand = 0, total_true = 0, surv_cap, rounds_cap, max_groups = 1;
    u64 max_clen = 0;
    int nseg;                    // segments the resolver cuts every chunk into (1: none)
    std::vector<InfFast> h_fast;
    std::vector<u64> gb, tb;

    static u32 cand_cap_of(u64 c_len) { return (u32)(c_len / 4096 + 64); }
    static u64 rows_rounds_of(u64 c_len) { return c_len * 8 / (64 * 640) + 32; }          // pool share of a chunk, in rounds
    static u64 groups_of(u32 n) { return ((u64)n + 2 + 63) / 64 + 2; }                    // groups of 64 tokens; tokens <= bytes + 1
    static u64 tiles_of(u32 n, u32 gs_tile) { return groups_of(n) / gs_tile + 2; }

    // lz_segs: 0, or MTS_LZ_SEGS; row_rounds: < 0, or MTS_INF_ROW_ROUNDS (tests: a pool that runs out)
    InflateScratch(const InflatePlan &P_, const InflateDims &D, int lz_segs, long row_rounds) : P(P_), h_fast(P_.ic.size()), gb(P_.ic.size()), tb(P_.ic.size())
    {
        const size_t n = P.ic.size();
        u64 cand = 0, ng = 0, nt = 0, cbits = 0, cells = 0, rounds = 0;
        for (size_t i = 0; i < n; i++) {
            const u64 c_len = P.ic[i].c_len;
            const u32 cap = cand_cap_of(c_len);
            h_fast[i] = {cand, cap, (u32)(2 * cand), 2 * cap, 0};
            gb[i] = ng; tb[i] = nt;
            cand += cap; ng += groups_of(P.nn[i]); nt += tiles_of(P.nn[i], D.gs_tile);
            cbits += 8 * c_len; rounds += rows_rounds_of(c_len);
            cells += align_up((u64)P.nn[i] + STREAM_PAD, STREAM_ALIGN);
            if (c_len > max_clen) max_clen = c_len;
            if (groups_of(P.nn[i]) - 2 > max_groups) max_groups = (u32)(groups_of(P.nn[i]) - 2);
        }
        total_cand = (u32)cand; total_true = (u32)(2 * cand);
        // with fewer chunks than CUs the resolver cuts a chunk into segments (inflate.hip: LzPlan); cells and windows live here
        nseg = lz_segs ? lz_segs : n < 128 ? (int)(256 / (n ? n : 1)) : 1;
        if (nseg > (int)D.lz_maxseg) nseg = (int)D.lz_maxseg;
        if (row_rounds >= 0) rounds = (u64)row_rounds;
        if (rounds > 0x3ffffffull) rounds = 0x3ffffffull;     // (row ids are 32 bits)
        rounds_cap = (u32)rounds;
        surv_cap = (u32)(cbits / 256 + 65536);                // ~0.1 % of the bit offsets pass the cheap filters
        const bool cut = nseg > 1;
        const size_t row_bytes = (size_t)rounds * 64 * D.rowcap * 4 + 256, cell_bytes = cut ? 2 * cells + 4096 : 0;
        const size_t seg_adler_bytes = cut ? n * D.lz_maxseg * D.lz_flushers * 16 : 0;

        WsLayout L{false};
        regions.reserve(32);
        auto take = [&](const char *name, size_t bytes) { regions.push_back({name, L.end, bytes}); return L.take(bytes); };
        so = take("so", 8 * n); nn = take("nn", 4 * n); fast = take("fast", sizeof(InfFast) * n); gb_off = take("gb_off", 8 * n); tb_off = take("tb_off", 8 * n);
        host_off = so; host_bytes = L.end - so;
        cand_cnt = take("cand_cnt", 4 * n); true_cnt = take("true_cnt", 4 * n); seq_flag = take("seq_flag", 4 * n);
        slot_chunk = take("slot_chunk", 4 * (size_t)total_cand); tslot_chunk = take("tslot_chunk", 4 * (size_t)total_true);
        cand_pos = take("cand_pos", 8 * (size_t)total_cand); cand_tmp = take("cand_tmp", 8 * (size_t)total_cand);
        cres = take("cres", D.cand_res_bytes * total_cand); tblk = take("tblk", D.true_blk_bytes * total_true);
        subs = take("subs", 8 * (size_t)D.subcap * total_cand);
        gbase = take("gbase", 4 * ng);
        tile_base = take("tile_base", 4 * (ng / D.gs_tile + 2 * n + 16));
        surv = take("surv", 8 * (size_t)surv_cap); surv_cnt = take("surv_cnt", 256);
        plan = take("plan", D.lz_plan_bytes * n);
        win = take("win", cut ? n * D.lz_maxseg * D.lz_win : 0);
        rows_cells = take("rows_cells", row_bytes > cell_bytes ? row_bytes : cell_bytes);
        round_row = take("round_row", 4 * (size_t)D.rounds_max * total_cand); row_ctr = take("row_ctr", 256);
        gflag = take("gflag", cut ? cells / D.lz_flush + n + 64 : 0);
        seg_adler = take("seg_adler", seg_adler_bytes);
        clear[0] = {gflag, seg_adler - gflag}; clear[1] = {seg_adler, seg_adler_bytes};
        end = L.end;
    }

    void fill(u8 *h) const                                    // host_bytes zeroed bytes
    {
        const size_t n = P.ic.size();
        auto put = [&](size_t off, const void *src, size_t bytes) { memcpy(h + (off - host_off), src, bytes); };
        put(so, P.so.data(), 8 * n); put(nn, P.nn.data(), 4 * n); put(fast, h_fast.data(), sizeof(InfFast) * n);
        put(gb_off, gb.data(), 8 * n); put(tb_off, tb.data(), 8 * n);
    }
};

// ---- where compressed bytes lie in the staging buffer ---------------------------------------------------------------------------
struct StageCopy { long src, dst; u64 len; };                 // caller's buffer offset -> staging buffer offset

// The run-joined rule (the decoded-chunk cache, the reductions): the listed chunks ids[0 .. m) lie in the staging buffer in list order
// at soff[id]; chunks back to back in the caller's buffer keep their distances, a gap starts at the next multiple of 16.
// -> the bytes to stage: 16 lie behind the last chunk
MTS_LOCAL inline u64 stage_runs(const long *c_off, const long *c_len, const int *ids, int m, long *soff)
{
    u64 ctot = 0;
    for (int k = 0; k < m; k++) {
        const int i = ids[k], p = k ? ids[k - 1] : -1;
        const bool joins = k && c_off[i] == c_off[p] + c_len[p];
        if (!joins) ctot = align_up(ctot + (k ? 16 : 0), 16);
        soff[i] = (long)ctot; ctot += (u64)c_len[i];
    }
    return ctot + 16;
}

// ... and the copies that move the listed chunks there: one for every run of chunks back to back in both buffers.  done (or null), by
// chunk: chunks moved already are left out, those listed are marked
MTS_LOCAL inline std::vector<StageCopy> run_copies(const long *c_off, const long *c_len, const long *soff, const int *ids, int m, char *done = nullptr)
{
    std::vector<StageCopy> cp;
    for (int k = 0; k < m; k++) {
        const int i = ids[k];
        if (done) { if (done[i]) continue; done[i] = 1; }
        if (!c_len[i]) continue;
        if (!cp.empty() && c_off[i] == cp.back().src + (long)cp.back().len && soff[i] == cp.back().dst + (long)cp.back().len) cp.back().len += (u64)c_len[i];
        else cp.push_back({c_off[i], soff[i], (u64)c_len[i]});
    }
    return cp;
}

// The rules of the host decoder (mts_decompress_chunks), which is handed all chunks of a call at once: when they lie nearly back to
// back in the caller's buffer, in any order -- a range read from a .cbin: at most a quarter of padding and 4096 bytes -- the whole
// range [lo, hi) is staged as it is and a piece's bytes are one copy; otherwise every chunk lies at its own 16-aligned offset with
// 8 bytes behind it and is one copy.  The pieces are cut by decoded bytes; a range that is not in ascending order is one piece.
struct MTS_LOCAL RangeStaging {
    const long *c_off, *c_len;
    int n;
    bool one_range, ascending = true;
    long lo, hi;
    std::vector<long> coff;
    u64 ctot = 0;
    std::vector<int> pb = {0};                                // chunks [pb[k], pb[k + 1]) make piece k (set by the caller: cut_pieces)

    RangeStaging(const long *c_off_, const long *c_len_, int n_) : c_off(c_off_), c_len(c_len_), n(n_), coff(n_)
    {
        lo = c_off[0]; hi = c_off[0] + c_len[0];
        u64 sum = 0;
        for (int i = 0; i < n; i++) {
            coff[i] = (long)ctot; ctot += align_up((u64)c_len[i] + 8, 16);
            if (c_off[i] < lo) lo = c_off[i];
            if (c_off[i] + c_len[i] > hi) hi = c_off[i] + c_len[i];
            sum += (u64)c_len[i];
            if (i) ascending = ascending && c_off[i] >= c_off[i - 1] + c_len[i - 1];
        }
        one_range = lo >= 0 && (u64)(hi - lo) <= sum + sum / 4 + 4096;
        if (one_range) { ctot = (u64)(hi - lo) + 16; for (int i = 0; i < n; i++) coff[i] = c_off[i] - lo; }
    }
    bool piecewise() const { return !one_range || ascending; }

    std::vector<StageCopy> copies(int k) const
    {
        const int np = (int)pb.size() - 1;
        std::vector<StageCopy> cp;
        if (one_range) {
            const long a = k == 0 ? lo : c_off[pb[k]], b = k + 1 == np ? hi : c_off[pb[k + 1]];
            if (b > a) cp.push_back({a, a - lo, (u64)(b - a)});
        } else {
            for (int i = pb[k]; i < pb[k + 1]; i++) if (c_len[i]) cp.push_back({c_off[i], coff[i], (u64)c_len[i]});
        }
        return cp;
    }
};

}  // namespace mts
