// C ABI of libmtscomp_hip.so (include/mtscomp_hip.h): per-device engine, workspace management, the
// stage pipelines and the host-buffer entry points.  No CPU fallback anywhere: without a gfx950 device
// every compute entry point returns MTS_E_NODEV.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <future>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <string>
#include <vector>

#include "common.h"

namespace mts {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// (device, kernel) pairs whose dynamic-LDS limit has been raised
int ensure_dynamic_lds(const void *kernel, int bytes)
{
    static std::mutex mu;
    static std::vector<std::pair<int, const void *>> done;
    int dev = -1;
    MTS_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    for (auto &d : done) if (d.first == dev && d.second == kernel) return MTS_OK;
    MTS_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.push_back({dev, kernel});
    return MTS_OK;
}

static const LevelCfg LEVELS[10] = {{0, 0, 0, 0},     {4, 4, 8, 4},       {4, 5, 16, 8},       {4, 6, 32, 32},
                                    {4, 4, 16, 16},   {8, 16, 32, 32},    {8, 16, 128, 128},   {8, 32, 128, 256},
                                    {32, 128, 258, 1024}, {32, 258, 258, 4096}};

void drop_device_caches();      // frees the decoded-chunk caches of the current device (called when a workspace allocation fails)

// grow-only device buffer
// MTS_ARENA_GB=N (experiment, round 6; default off): the workspaces of a device come out of ONE allocation of N GiB made when
// the first of them is asked for, 2 MiB-aligned pieces handed out one behind the other (a buffer that grows takes a new piece;
// the arena is given back by mts_release).  Asks whether k_match5's three times -- the physical placement of its workspace,
// tools/m5_addr_times.py -- go away when the placement is one big block instead of a dozen allocations made between others.
struct Arena { u8 *base = nullptr; size_t cap = 0, used = 0; bool tried = false; };
static Arena g_arena[64];
static size_t arena_gb() { static const size_t v = [] { const char *e = getenv("MTS_ARENA_GB"); return e ? (size_t)atoll(e) : (size_t)0; }(); return v; }
static void *arena_take(size_t bytes)
{
    if (!arena_gb()) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    Arena &A = g_arena[dev];
    if (!A.tried) {
        A.tried = true;
        if (hipMalloc((void **)&A.base, arena_gb() << 30) == hipSuccess) A.cap = arena_gb() << 30; else { (void)hipGetLastError(); A.base = nullptr; }
    }
    const size_t need = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
    if (!A.base || A.used + need > A.cap) return nullptr;
    void *p = A.base + A.used;
    A.used += need;
    return p;
}
static void arena_reset()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return;
    Arena &A = g_arena[dev];
    if (A.base) (void)hipFree(A.base);
    A = Arena();
}

struct DBuf {
    void *p = nullptr;
    size_t cap = 0;
    u64 gen = 0;              // bumped whenever the buffer is (re)allocated, freed or an allocation fails: what it held is gone
    bool in_arena = false;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return MTS_OK;
        gen++;
        if (p && !in_arena) (void)hipFree(p);
        p = nullptr; cap = 0; in_arena = false;
        const size_t want = bytes + bytes / 8 + 4096;
        if (void *a = arena_take(want)) { p = a; cap = want; in_arena = true; return MTS_OK; }
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            e = hipMalloc(&p, bytes);
            if (e != hipSuccess) { (void)hipGetLastError(); drop_device_caches(); e = hipMalloc(&p, bytes); }      // decoded chunks are only a cache
            if (e != hipSuccess) { p = nullptr; set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); return MTS_E_NOMEM; }
            cap = bytes;
        } else cap = want;
        return MTS_OK;
    }
    void release() { if (p && !in_arena) (void)hipFree(p); p = nullptr; cap = 0; in_arena = false; gen++; }
    template <typename T> T *as() { return (T *)p; }
};

constexpr int MAX_STAGES = 24;

struct Engine {
    int dev = -1;
    std::mutex mu;
    hipStream_t own = nullptr;
    // compress workspace
    DBuf stream, sort_a, sort_b, sort_ws, tables, tokens, marks, segbuf, blk, blkcodes, blkhdr, desc, adler, misc;
    DBuf fast_lists, fast_state;         // levels 1..3: candidate lists of two phases, per-chunk state of the in-order walk
    hipStream_t fast_st = nullptr;       // ... and the stream the lists are made on, with its events (lists ready x2, lists read x2, inputs ready)
    hipEvent_t fast_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // host-API staging
    DBuf h_in, h_out;
    // host copies of a batch's descriptors on their way to the device: they live here until the next batch replaces them, i.e.
    // past the hipStreamSynchronize that ends the batch they belong to (hipMemcpyAsync from pageable memory is not promised to
    // have read its source when it returns)
    std::vector<u8> host_stage[2];
    // pinned pieces the host entry points move user memory through (pageable memory crosses the bus at a fraction of the
    // link's rate, and a fresh destination array takes its page faults on the copying thread): two pieces, so that the
    // DMA of one overlaps the host threads copying the other
    // (round 6: one set per direction -- the host entry points copy the next piece in and the piece before out on two host
    //  threads while the device works on the current one)
    struct Stager {
        void *pin[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {nullptr, nullptr};
        hipStream_t st = nullptr;
        std::mutex mu;                                   // (a stager's pieces belong to one copy at a time)
        void release()
        {
            for (int k = 0; k < 2; k++) { if (pin[k]) (void)hipHostFree(pin[k]); pin[k] = nullptr; if (ev[k]) (void)hipEventDestroy(ev[k]); ev[k] = nullptr; }
            if (st) (void)hipStreamDestroy(st);
            st = nullptr;
        }
    } stg[2];                                            // [0]: host -> device, [1]: device -> host
    // inflate workspace
    DBuf inf_scratch, inf_desc, segsums;
    // window statistics: tile descriptors, the partial slab, the outputs of the host entry point
    DBuf stats;
    // decimation: taps, columns, segment tables, the output of the host entry point
    DBuf dec;
    // peak detection: taps, columns, thresholds, segment tables, the filtered slab, its event bitmap, block counts and offsets,
    // the outputs of the host entry point
    DBuf det;
    // Welch PSD: taper, twiddles, columns, segment tables, block partials, group sums
    DBuf welch;
    // Gram matrices: columns, slab and group tables, slab partials, the accumulators of the host entry point
    DBuf gram;
    // channel-mixing products: weights, offsets, columns, segment tables, the output of the host entry point
    DBuf proj;
    // geometry of the last compress batch whose per-segment / per-block / per-tile descriptors are on the device (a recording is
    // compressed batch after batch of the same shape: the 10 MB of index arrays need not be rebuilt and copied every call)
    // (valid while the three buffers are the allocations the arrays were copied into: DBuf::gen, not the address -- a buffer
    // freed by mts_release() and allocated again usually comes back at the same address with nothing in it)
    std::vector<u32> geo_n;
    u64 geo_seg = ~0ull, geo_blk = ~0ull, geo_desc = ~0ull;
    // stage timing
    hipEvent_t ev[MAX_STAGES + 1];
    bool ev_ok = false;
    const char *stage_name[MAX_STAGES];
    int n_stage = 0;
    float stage_ms[MAX_STAGES];
    int n_stage_done = 0;
    const char *done_name[MAX_STAGES];

    int init_events()
    {
        if (ev_ok) return MTS_OK;
        for (int i = 0; i <= MAX_STAGES; i++) MTS_HIP(hipEventCreate(&ev[i]));
        ev_ok = true;
        return MTS_OK;
    }
    int init_fast_streams()
    {
        if (fast_st) return MTS_OK;
        MTS_HIP(hipStreamCreateWithFlags(&fast_st, hipStreamNonBlocking));
        for (auto &e : fast_ev) MTS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return MTS_OK;
    }
    void t_begin(hipStream_t st) { n_stage = 0; (void)hipEventRecord(ev[0], st); }
    void t_mark(hipStream_t st, const char *name)
    {
        if (n_stage < MAX_STAGES) { stage_name[n_stage] = name; n_stage++; (void)hipEventRecord(ev[n_stage], st); }
    }
    void t_collect(bool accumulate)
    {
        if (!accumulate) { n_stage_done = 0; }
        for (int i = 0; i < n_stage; i++) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            int k = -1;
            for (int j = 0; j < n_stage_done; j++) if (!strcmp(done_name[j], stage_name[i])) k = j;
            if (k < 0 && n_stage_done < MAX_STAGES) { k = n_stage_done++; done_name[k] = stage_name[i]; stage_ms[k] = 0; }
            if (k >= 0) stage_ms[k] += ms;
        }
    }
    void release_all()
    {
        DBuf *all[] = {&stream, &sort_a, &sort_b, &sort_ws, &tables, &tokens, &marks, &segbuf, &blk, &blkcodes, &blkhdr, &desc,
                       &adler, &misc, &h_in, &h_out, &inf_scratch, &inf_desc, &segsums, &fast_lists, &fast_state, &stats, &dec, &det, &welch, &gram, &proj};
        for (DBuf *b : all) b->release();
        arena_reset();                                   // (every piece of it has just been let go)
        geo_n.clear();
        for (auto &g : stg) g.release();
        if (fast_st) (void)hipStreamDestroy(fast_st);
        fast_st = nullptr;
        for (auto &e : fast_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
};

static std::mutex g_mu;
static std::vector<Engine *> g_engines;
static int g_ndev = -2;

static int device_count()
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ndev != -2) return g_ndev;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    int ok = 0;
    for (int d = 0; d < n; d++) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) break;
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) break;     // code objects are gfx950 only
        ok++;
    }
    g_ndev = ok;
    g_engines.assign(ok, nullptr);
    return g_ndev;
}

static int get_engine(int device, Engine **out)
{
    const int n = device_count();
    if (n <= 0) { set_error("no gfx950 device visible (libmtscomp_hip has no CPU path)"); return MTS_E_NODEV; }
    if (device < 0 || device >= n) { set_error("device %d out of range (%d visible)", device, n); return MTS_E_ARG; }
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_engines[device]) { g_engines[device] = new Engine(); g_engines[device]->dev = device; }
    *out = g_engines[device];
    return MTS_OK;
}

constexpr int PARSE_PARALLEL_ROUNDS = 96;     // parallel correction rounds of the speculative parse (~40 us each) before the in-order pass:
                                              // chains of a few dozen segments (a dead channel) are cheaper in parallel, whole-chunk chains are not

static long compress_bound(long n) { return n + (n >> 12) + (n >> 14) + (n >> 25) + 13; }

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
    std::vector<ChunkDesc> cd(n_chunks);
    std::vector<TileDesc> tiles;
    u64 soff = 0, toff = 0, sorted_off = 0;
    u32 nseg = 0, nblk = 0, max_rows = 0;
    const u64 row_bytes = (u64)nc * sz;
    for (int i = 0; i < n_chunks; i++) {
        const u64 rows = (u64)(bounds[i + 1] - bounds[i]);
        const u64 n = raw_is_stream ? rows : rows * row_bytes;
        if (n >= (1ull << 31)) { set_error("chunk %d is %llu bytes; chunks must be < 2 GiB", i, (unsigned long long)n); return MTS_E_ARG; }
        ChunkDesc &c = cd[i];
        c.stream_off = soff; c.tok_off = toff; c.out_off = (u64)slot_off[i];
        c.raw_off = (u64)(bounds[i] - bounds[0]) * (raw_is_stream ? 1 : row_bytes);
        c.n = (u32)n; c.n_rows = (u32)rows;
        c.seg0 = nseg; c.nseg = (u32)((n + SEG - 1) / SEG);
        c.blk0 = nblk; c.blk_cap = (u32)(n / BLOCK_TOKENS + 2);
        if (c.out_off & 15) { set_error("output slot %d is not 16-byte aligned", i); return MTS_E_ARG; }
        nseg += c.nseg; nblk += c.blk_cap;
        if (rows > max_rows) max_rows = (u32)rows;
        c.tile0 = (u32)tiles.size(); c.pad = 0;
        for (u64 a = 0; a < n; a += TILE) {
            TileDesc t;
            t.stream_off = soff; t.sorted_off = sorted_off; t.n = (u32)n; t.a = (u32)a;
            t.w = (u32)(a >= (u64)HALO ? a - HALO : 0);
            t.own_end = (u32)(a + TILE < n ? a + TILE : n);
            const u64 hashed_end = n >= 3 ? (t.own_end < n - 2 ? t.own_end : n - 2) : 0;
            t.wlen = hashed_end > t.w ? (u32)(hashed_end - t.w) : 0;
            t.chunk = (u32)i;
            sorted_off += align_up(t.wlen, 64);
            tiles.push_back(t);
        }
        soff += align_up(n + STREAM_PAD, STREAM_ALIGN);
        toff += n + 1;
    }
    const u64 stream_bytes = soff + STREAM_PAD;
    // ---- workspace ----
    int rc;
    if (!raw_is_stream) { if ((rc = E.stream.ensure(stream_bytes))) return rc; }
    const size_t sort_n = align_up(sorted_off + 64, 64);          // 32-bit keys
    // (the first pass's keys are dead once the sort is done: the parse keeps its marks there)
    const size_t marks_words = parse_marks_words((size_t)nseg + 64);
    if ((rc = E.sort_a.ensure((sort_n > marks_words ? sort_n : marks_words) * 4))) return rc;
    if ((rc = E.sort_b.ensure(sort_n * 4))) return rc;
    if ((rc = E.sort_ws.ensure(hash_sort_ws_bytes((int)tiles.size())))) return rc;
    // one word per position (levels 1..3: the inverse map) + for levels 4..9 the side table of the quarter-budget results, which is
    // written and read at a fraction of a percent of the positions only
    const size_t table_words = align_up(stream_bytes + 64, 64);
    if ((rc = E.tables.ensure(table_words * 4 * (level < 4 ? 1 : 2)))) return rc;
    if ((rc = E.tokens.ensure((toff + 64) * 4))) return rc;
    if ((rc = E.segbuf.ensure((size_t)(nseg + 64) * 4 * (7 + parse_cp_words()) + 256))) return rc;
    if ((rc = E.blk.ensure((size_t)(nblk + 1) * (sizeof(BlockRec) + 8) + 256))) return rc;
    if ((rc = E.blkcodes.ensure((size_t)(nblk + 1) * BLK_CODE_WORDS * 4))) return rc;
    if ((rc = E.blkhdr.ensure((size_t)(nblk + 1) * BLK_HDR_WORDS * 4))) return rc;
    const size_t desc_bytes = align_up(sizeof(ChunkDesc) * n_chunks, 256) + align_up(sizeof(TileDesc) * (tiles.size() + 1), 256) +
                              align_up(sizeof(ChunkOut) * n_chunks, 256);
    if ((rc = E.desc.ensure(desc_bytes))) return rc;
    if ((rc = E.adler.ensure(sizeof(u64) * 2 * n_chunks + 256 + MATCH_SINK_BYTES))) return rc;      // + the flag words and the match stage's sink behind them
    if ((rc = E.init_events())) return rc;

    u8 *dp = E.desc.as<u8>();
    ChunkDesc *d_chunks = (ChunkDesc *)dp; dp += align_up(sizeof(ChunkDesc) * n_chunks, 256);
    TileDesc *d_tiles = (TileDesc *)dp; dp += align_up(sizeof(TileDesc) * (tiles.size() + 1), 256);
    ChunkOut *d_cout = (ChunkOut *)dp;
    // per-segment arrays
    u32 *sg = E.segbuf.as<u32>();
    ParseBufs pb;
    const size_t SN = nseg + 64;
    pb.entry = sg; pb.exit_a = sg + SN; pb.exit_b = sg + 2 * SN; pb.cnt = sg + 3 * SN; pb.tokbase = sg + 4 * SN;
    pb.seg_chunk = sg + 5 * SN; pb.seg_start = sg + 6 * SN;
    pb.cp = sg + 7 * SN;
    pb.changed = (int *)(E.adler.as<u8>() + sizeof(u64) * 2 * n_chunks);
    pb.marks = E.sort_a.as<u32>();
    // block arrays
    BlockRec *d_blocks = E.blk.as<BlockRec>();
    u32 *d_blk_chunk = (u32 *)(d_blocks + nblk + 1);
    u32 *d_blk_in_start = d_blk_chunk + nblk + 1;

    MTS_HIP(hipMemcpyAsync(d_chunks, cd.data(), sizeof(ChunkDesc) * n_chunks, hipMemcpyHostToDevice, st));
    {
        // the index arrays depend on the chunk sizes only: kept on the device while the next batch has the same sizes and
        // the buffers have not moved
        std::vector<u32> sizes_now(n_chunks);
        for (int i = 0; i < n_chunks; i++) sizes_now[i] = cd[i].n;
        const bool same = sizes_now == E.geo_n && E.geo_seg == E.segbuf.gen && E.geo_blk == E.blk.gen && E.geo_desc == E.desc.gen;
        if (!same) {
            E.geo_n.clear();                                      // (not valid again until everything below is on its way)
            std::vector<u32> h_seg(2 * (size_t)nseg), h_blk_chunk(nblk + 1);
            for (int i = 0; i < n_chunks; i++) {
                for (u32 k = 0; k < cd[i].nseg; k++) { h_seg[cd[i].seg0 + k] = (u32)i; h_seg[nseg + cd[i].seg0 + k] = k * SEG; }
                for (u32 k = 0; k < cd[i].blk_cap; k++) h_blk_chunk[cd[i].blk0 + k] = (u32)i;
            }
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

    E.t_begin(st);
    const u8 *d_stream;
    u64 *d_adler = E.adler.as<u64>();
    std::vector<u64> so(n_chunks); std::vector<u32> nn(n_chunks);
    if (raw_is_stream) {
        // debug path: the caller's bytes already are the transformed stream (one chunk)
        d_stream = d_raw;
        for (int i = 0; i < n_chunks; i++) { so[i] = cd[i].stream_off; nn[i] = cd[i].n; }
        if ((rc = E.misc.ensure(12 * (size_t)n_chunks + 64))) return rc;
        u64 *d_so = E.misc.as<u64>(); u32 *d_nn = (u32 *)(d_so + n_chunks);
        MTS_HIP(hipMemcpyAsync(d_so, so.data(), 8 * (size_t)n_chunks, hipMemcpyHostToDevice, st));
        MTS_HIP(hipMemcpyAsync(d_nn, nn.data(), 4 * (size_t)n_chunks, hipMemcpyHostToDevice, st));
        u32 max_n = 0; for (int i = 0; i < n_chunks; i++) if (cd[i].n > max_n) max_n = cd[i].n;
        if ((rc = launch_adler_stream(st, d_stream, d_so, d_nn, n_chunks, max_n, d_adler, nullptr, 0))) return rc;
    } else {
        if ((rc = launch_delta_transpose(st, d_raw, E.stream.p, d_chunks, n_chunks, max_rows, nc, sz, flags, d_adler))) return rc;
        d_stream = E.stream.as<u8>();
    }
    E.t_mark(st, "delta_transpose");
    u32 *tmp_k = E.sort_a.as<u32>(), *srt_k = E.sort_b.as<u32>();
    u32 *d_tables = E.tables.as<u32>(), *d_quarter = d_tables + table_words;
    u32 *d_flags = (u32 *)(pb.changed + 1);                   // [0] bit 0: the match stage found a hash run out of position order
    u32 *d_tokens = E.tokens.as<u32>();
    int force_ballot = getenv("MTS_SORT_INJECT_DISORDER") ? 2 : 0;      // (test hook: the first sort of the call is deliberately mis-ranked)
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
            u32 max_n = 0;
            for (int i = 0; i < n_chunks; i++) if (cd[i].n > max_n) max_n = cd[i].n;
            const u64 K = (u64)fast_list_rows(level);
            const char *be = getenv("MTS_FAST_LIST_BYTES");      // (tests: a tiny budget = many phases)
            const u64 budget = be ? strtoull(be, nullptr, 10) : (u64)8 << 30;
            // two list buffers: the lists of phase k + 1 are made on a second stream while phase k is walked (the walk keeps
            // one wave per chunk busy, the rest of the device is free)
            u64 W = budget / 2 / ((u64)n_chunks * K * 4) / 256 * 256;
            if (W < 256) W = 256;
            if (W > align_up(max_n, 256)) W = align_up(max_n, 256);
            if (W > 1024 && W * 8 > max_n) W = align_up((max_n + 7) / 8, 256);      // at least 8 phases: only the first lists are waited for
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
        if (getenv("MTS_DEBUG_ADDR"))                                 // (tools/m5_addr_times.py: does the match stage's time follow where its buffers lie?)
            fprintf(stderr, "[addr] stream %p sorted %p tables %p quarter %p tiles %zu\n", (void *)d_stream, (void *)srt_k, (void *)d_tables, (void *)d_quarter, tiles.size());
        if ((rc = launch_match(st, d_stream, d_tiles, (int)tiles.size(), srt_k, d_tables, d_quarter, cfg, d_flags, tap && tap->t_full ? 1 : 0))) return rc;
        E.t_mark(st, "match");
        u32 max_nseg = 0;
        for (int i = 0; i < n_chunks; i++) if (cd[i].nseg > max_nseg) max_nseg = cd[i].nseg;
        if ((rc = launch_parse_spec(st, d_tables, d_quarter, d_chunks, pb, (int)nseg, cfg, n_chunks, max_nseg))) return rc;
        for (;;) {
            if ((rc = launch_parse_fix(st, d_tables, d_quarter, d_chunks, pb, (int)nseg, cfg, round))) return rc;
            round++;
            int hflags[2] = {0, 0};                              // {changed, match-stage flags}
            MTS_HIP(hipMemcpyAsync(hflags, pb.changed, 8, hipMemcpyDeviceToHost, st));
            MTS_HIP(hipStreamSynchronize(st));
            static const bool debug_flags = getenv("MTS_DEBUG_FLAGS") != nullptr;      // (read once)
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
        u32 max_nseg = 0;
        for (int i = 0; i < n_chunks; i++) if (cd[i].nseg > max_nseg) max_nseg = cd[i].nseg;
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

// ------------------------------------------------------------------------------------------------
// user memory <-> device through pinned pieces
// ------------------------------------------------------------------------------------------------
constexpr size_t PIN_PIECE = (size_t)32 << 20;

static int host_threads()
{
    static const int n = [] { const char *e = getenv("MTS_HOST_THREADS"); int v = e ? atoi(e) : 8; return v < 1 ? 1 : v > 64 ? 64 : v; }();
    return n;
}

// memcpy by several threads (a fresh destination is faulted in by all of them at once).  The threads are a pool that lives as
// long as the library (round 6): started per call they cost ~100 us per copy -- nothing against a 32 MiB piece, a third of the
// time of the 4 MiB pieces a cold Reader window is moved in.  One copy at a time uses the pool; a second caller (the other
// direction of a pipelined host call) copies on its own thread instead of waiting.
namespace {
struct CopyPool {
    std::mutex mu, use;                                 // mu: the job; use: one parallel copy at a time
    std::condition_variable cv_go, cv_done;
    std::vector<std::thread> th;
    u8 *dst = nullptr; const u8 *src = nullptr; size_t n = 0, per = 0;
    u64 gen = 0; int pending = 0; bool stop = false;
    void worker(int t, u64 seen /* the job counter when the thread was made: jobs published before are not its */)
    {
        for (;;) {
            std::unique_lock<std::mutex> lk(mu);
            cv_go.wait(lk, [&] { return stop || gen != seen; });
            if (stop) return;
            seen = gen;
            const size_t a = (size_t)t * per;
            u8 *d = dst; const u8 *s = src; const size_t nn = n, pp = per;
            lk.unlock();
            if (a < nn) memcpy(d + a, s + a, nn - a < pp ? nn - a : pp);
            lk.lock();
            if (--pending == 0) cv_done.notify_one();
        }
    }
    void run(void *d, const void *s, size_t bytes, int nt)
    {
        if ((int)th.size() + 1 < nt) {
            std::lock_guard<std::mutex> lk(mu);
            for (int t = (int)th.size() + 1; t < nt; t++) th.emplace_back(&CopyPool::worker, this, t, gen);
        }
        // (the share is rounded UP before it is aligned: with n / nt an exact multiple of 4096 and n % nt != 0 the threads' shares
        //  ended n % nt bytes short of n -- the last bytes of such a copy were never made; found by tools/fuzz_gpu.py, seed 301)
        const size_t p = ((bytes + nt - 1) / nt + 4095) & ~(size_t)4095;
        {
            std::lock_guard<std::mutex> lk(mu);
            dst = (u8 *)d; src = (const u8 *)s; n = bytes; per = p; pending = (int)th.size(); gen++;
        }
        cv_go.notify_all();
        memcpy(d, s, bytes < p ? bytes : p);                            // share 0 on the calling thread
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
    }
    ~CopyPool()
    {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv_go.notify_all();
        for (auto &t : th) t.join();
    }
};
CopyPool g_copy_pool;
}  // namespace
static void par_memcpy(void *dst, const void *src, size_t n)
{
    const int nt = n < ((size_t)1 << 20) ? 1 : host_threads();
    if (nt == 1) { memcpy(dst, src, n); return; }
    std::unique_lock<std::mutex> one(g_copy_pool.use, std::try_to_lock);
    if (!one.owns_lock()) { memcpy(dst, src, n); return; }            // (the pool is busy with the other direction's copy)
    g_copy_pool.run(dst, src, n, nt);
}

static int pin_init(Engine::Stager &G)
{
    if (G.pin[0]) return MTS_OK;
    for (int k = 0; k < 2; k++) {
        if (hipHostMalloc(&G.pin[k], PIN_PIECE, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); G.pin[k] = nullptr; }
        if (G.pin[k] && hipEventCreateWithFlags(&G.ev[k], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(G.pin[k]); G.pin[k] = nullptr; }
    }
    if (G.pin[0] && G.pin[1] && hipStreamCreateWithFlags(&G.st, hipStreamNonBlocking) == hipSuccess) return MTS_OK;
    (void)hipGetLastError();
    for (int k = 0; k < 2; k++) { if (G.pin[k]) (void)hipHostFree(G.pin[k]); G.pin[k] = nullptr; }
    return MTS_E_NOMEM;           // (the callers fall back to plain copies)
}

// device -> user memory, any number of pieces (dst, src, bytes).  The device data must be complete (the caller synchronised the
// stream that produced it).  The DMA of the next piece runs while the host threads copy the one before out of its pinned buffer.
struct CopyItem { void *dst; const void *src; size_t n; };
static bool host_ptr_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

static int staged_d2h_multi(Engine &E, const std::vector<CopyItem> &segs)
{
    Engine::Stager &G = E.stg[1];
    std::lock_guard<std::mutex> lk(G.mu);
    size_t total = 0;
    for (auto &s : segs) total += s.n;
    // a destination that is pinned already (mts_host_alloc) takes the DMA itself: no pinned piece in between, no host copy
    if (total >= ((size_t)1 << 20) && !segs.empty()) {
        bool all_pinned = true;
        for (auto &s : segs) if (s.n && !host_ptr_pinned(s.dst)) { all_pinned = false; break; }
        if (all_pinned) {
            hipStream_t cs = pin_init(G) == MTS_OK ? G.st : nullptr;
            for (auto &s : segs) if (s.n) MTS_HIP(hipMemcpyAsync(s.dst, s.src, s.n, hipMemcpyDeviceToHost, cs));
            MTS_HIP(hipStreamSynchronize(cs));
            return MTS_OK;
        }
    }
    if (total < ((size_t)1 << 20) || pin_init(G) != MTS_OK) {
        for (auto &s : segs) if (s.n) MTS_HIP(hipMemcpy(s.dst, s.src, s.n, hipMemcpyDeviceToHost));
        return MTS_OK;
    }
    std::vector<CopyItem> items;                      // cut to pinned-piece size
    for (auto &s : segs)
        for (size_t o = 0; o < s.n; o += PIN_PIECE) items.push_back({(u8 *)s.dst + o, (const u8 *)s.src + o, s.n - o < PIN_PIECE ? s.n - o : PIN_PIECE});
    auto issue = [&](size_t k) -> int {
        MTS_HIP(hipMemcpyAsync(G.pin[k & 1], items[k].src, items[k].n, hipMemcpyDeviceToHost, G.st));
        MTS_HIP(hipEventRecord(G.ev[k & 1], G.st));
        return MTS_OK;
    };
    int rc;
    if (!items.empty() && (rc = issue(0))) return rc;
    for (size_t k = 0; k < items.size(); k++) {
        if (k + 1 < items.size() && (rc = issue(k + 1))) return rc;
        MTS_HIP(hipEventSynchronize(G.ev[k & 1]));
        par_memcpy(items[k].dst, G.pin[k & 1], items[k].n);
    }
    return MTS_OK;
}
static int staged_d2h(Engine &E, void *dst, const void *d_src, size_t n) { return staged_d2h_multi(E, {{dst, d_src, n}}); }

// user memory -> device; complete on return
static int staged_h2d(Engine &E, void *d_dst, const void *src, size_t n)
{
    Engine::Stager &G = E.stg[0];
    std::lock_guard<std::mutex> lk(G.mu);
    if (n >= ((size_t)1 << 20) && host_ptr_pinned(src)) {            // (a pinned source: the DMA reads it directly; on the stager's own
        hipStream_t cs = pin_init(G) == MTS_OK ? G.st : nullptr;   //  stream, so that it runs beside the kernels of the piece before)
        MTS_HIP(hipMemcpyAsync(d_dst, src, n, hipMemcpyHostToDevice, cs));
        MTS_HIP(hipStreamSynchronize(cs));
        return MTS_OK;
    }
    // (small copies take the plain call -- which, on the null stream, waits for the kernels there: the pieces of a pipelined call are
    //  megabytes and go through the stager's own stream)
    if (n < ((size_t)1 << 20) || pin_init(G) != MTS_OK) { MTS_HIP(hipMemcpy(d_dst, src, n, hipMemcpyHostToDevice)); return MTS_OK; }
    // pieces of the page-locked buffers' size -- or, for a transfer of a few MB (the compressed bytes of a cold window), a quarter
    // of it, so that the DMA of one piece runs under the host copy of the next
    size_t piece = PIN_PIECE;
    if (n < 4 * PIN_PIECE) { piece = ((n + 3) / 4 + 4095) & ~(size_t)4095; if (piece < ((size_t)2 << 20)) piece = (size_t)2 << 20; if (piece > PIN_PIECE) piece = PIN_PIECE; }
    const size_t np = (n + piece - 1) / piece;
    auto len = [&](size_t k) { return k + 1 < np ? piece : n - k * piece; };
    for (size_t k = 0; k < np; k++) {
        if (k >= 2) MTS_HIP(hipEventSynchronize(G.ev[k & 1]));       // the DMA out of this piece two rounds ago
        par_memcpy(G.pin[k & 1], (const u8 *)src + k * piece, len(k));
        MTS_HIP(hipMemcpyAsync((u8 *)d_dst + k * piece, G.pin[k & 1], len(k), hipMemcpyHostToDevice, G.st));
        MTS_HIP(hipEventRecord(G.ev[k & 1], G.st));
    }
    MTS_HIP(hipStreamSynchronize(G.st));
    return MTS_OK;
}

// The host entry points work piece by piece (round 6): while the device compresses / inflates piece k, one host thread copies
// piece k + 1 in and another copies the result of piece k - 1 out -- the three used to follow each other (PCIe in, kernels, PCIe
// out: 21 / 31 GB/s for the 60-chunk recording where the kernels alone do 46 / 134).  A piece is MTS_PIPE_BYTES of raw data
// (default 256 MiB; 0 = one piece, the old behaviour): big enough that the kernels lose nothing, small enough that a recording
// of a few hundred MB already overlaps.
// a piece's copy on a helper thread; when no thread can be started (std::system_error) the copy is made at once, on this one
template <class F>
static std::future<int> copy_beside(F &&f, int k)
{
    try {
        return std::async(std::launch::async, f, k);
    } catch (...) {
        std::promise<int> p;
        int rc = MTS_E_INTERNAL;
        try { rc = f(k); } catch (...) {}
        p.set_value(rc);
        return p.get_future();
    }
}
static size_t pipe_piece_bytes()
{
    const char *e = getenv("MTS_PIPE_BYTES");
    return e ? (size_t)atoll(e) : ((size_t)256 << 20);
}
static std::vector<int> pipe_pieces(const long *n_rows_or_bounds, bool is_bounds, int n_chunks, u64 row_bytes)
{
    std::vector<int> pb = {0};
    const size_t piece = pipe_piece_bytes();
    if (piece) {
        u64 acc = 0;
        for (int i = 0; i < n_chunks; i++) {
            const u64 n = (u64)(is_bounds ? n_rows_or_bounds[i + 1] - n_rows_or_bounds[i] : n_rows_or_bounds[i]) * row_bytes;
            if (acc && acc + n > piece) { pb.push_back(i); acc = 0; }
            acc += n;
        }
    }
    pb.push_back(n_chunks);
    return pb;
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
    if (sz != 1 && sz != 2 && sz != 4 && sz != 8) { set_error("itemsize %d unsupported", sz); return MTS_E_ARG; }
    if ((flags & MTS_FLAG_FLOAT) && sz != 4 && sz != 8) { set_error("float items of %d bytes unsupported", sz); return MTS_E_ARG; }
    if (nc <= 0 || n_chunks < 0) return MTS_E_ARG;
    MTS_HIP(hipSetDevice(E.dev));
    const size_t budget = batch_budget_bytes(level < 4);
    const u64 row_bytes = (u64)nc * sz;
    int i = 0;
    bool first = !add_times;
    while (i < n_chunks) {
        int j = i;
        size_t acc = 0;
        while (j < n_chunks) {
            const size_t n = (size_t)(bounds[j + 1] - bounds[j]) * row_bytes;
            if (j > i && (acc + n > budget || j - i >= MAX_BATCH_CHUNKS)) break;
            acc += n; j++;
        }
        const u8 *raw = (const u8 *)d_raw + (u64)(bounds[i] - bounds[0]) * row_bytes;
        int rc = compress_batch(E, st, raw, false, nc, sz, bounds + i, j - i, flags, level, d_out, slot_off + i, out_sizes + i,
                                !first, nullptr);
        if (rc) return rc;
        first = false;
        i = j;
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
    std::vector<InfChunk> ic(n_chunks);
    std::vector<u64> so(n_chunks), oo(n_chunks);
    std::vector<u32> nn(n_chunks), rows(n_chunks);
    u64 soff = 0, toff = 0;
    u32 max_n = 0, max_rows = 0;
    const u64 row_bytes = (u64)(nc_full ? nc_full : nc) * sz;
    for (int i = 0; i < n_chunks; i++) {
        const u64 n = (u64)n_rows[i] * row_bytes;
        if (n >= (1ull << 31)) { set_error("chunk %d is %llu bytes; chunks must be < 2 GiB", i, (unsigned long long)n); return MTS_E_ARG; }
        ic[i].c_off = (u64)c_off[i]; ic[i].c_len = (u64)c_len[i];
        ic[i].stream_off = soff; ic[i].tok_off = toff; ic[i].n_expect = (u32)n;
        ic[i].n_need = nc_full ? (u32)((u64)n_rows[i] * nc * sz) : 0u;
        if (nc_full && ic[i].n_need == 0) ic[i].n_need = 1;      // (a chunk without rows: still a partial decode)
        so[i] = soff; oo[i] = (u64)out_off[i]; nn[i] = (u32)n; rows[i] = (u32)n_rows[i];
        if (n > max_n) max_n = (u32)n;
        if (n_rows[i] > (long)max_rows) max_rows = (u32)n_rows[i];
        soff += align_up(n + STREAM_PAD, STREAM_ALIGN);
        toff += align_up(n + 2, 4);          // 16-byte aligned token arrays (vector loads)
    }
    int rc;
    if ((rc = E.stream.ensure(soff + STREAM_PAD))) return rc;
    if ((rc = E.tokens.ensure((toff + 64) * 4))) return rc;
    // (what the host fills lies in a row: one copy)
    const size_t o_ic = 0, o_so = align_up(sizeof(InfChunk) * n_chunks, 256), o_nn = o_so + align_up(8 * (size_t)n_chunks, 256),
                 o_oo = o_nn + align_up(4 * (size_t)n_chunks, 256), o_rows = o_oo + align_up(8 * (size_t)n_chunks, 256),
                 o_res = o_rows + align_up(4 * (size_t)n_chunks, 256), o_status = o_res + align_up(sizeof(InfResult) * n_chunks, 256),
                 o_end = o_status + align_up(4 * (size_t)n_chunks, 256);
    if ((rc = E.inf_desc.ensure(o_end + 256))) return rc;
    if ((rc = E.adler.ensure(sizeof(u64) * 2 * n_chunks + 256))) return rc;
    if ((rc = E.segsums.ensure(cumsum_scratch_bytes(n_chunks, max_rows, nc)))) return rc;
    if ((rc = E.init_events())) return rc;
    u8 *dp = E.inf_desc.as<u8>();
    InfChunk *d_ic = (InfChunk *)(dp + o_ic);
    InfResult *d_res = (InfResult *)(dp + o_res);
    u64 *d_so = (u64 *)(dp + o_so);
    u64 *d_oo = (u64 *)(dp + o_oo);
    u32 *d_rows = (u32 *)(dp + o_rows);
    int *d_status = (int *)(dp + o_status);
    {
        std::vector<u64> clens(n_chunks);
        for (int i = 0; i < n_chunks; i++) clens[i] = ic[i].c_len;
        if ((rc = E.inf_scratch.ensure(inflate_scratch_bytes(n_chunks, clens.data(), nn.data())))) return rc;
    }
    {
        std::vector<u8> &hst = E.host_stage[0];
        hst.assign(o_res, 0);
        memcpy(hst.data() + o_ic, ic.data(), sizeof(InfChunk) * n_chunks);
        memcpy(hst.data() + o_so, so.data(), 8 * (size_t)n_chunks);
        memcpy(hst.data() + o_nn, nn.data(), 4 * (size_t)n_chunks);
        memcpy(hst.data() + o_oo, oo.data(), 8 * (size_t)n_chunks);
        memcpy(hst.data() + o_rows, rows.data(), 4 * (size_t)n_chunks);
        MTS_HIP(hipMemcpyAsync(dp, hst.data(), o_res, hipMemcpyHostToDevice, st));
    }
    E.t_begin(st);
    if ((rc = launch_inflate(st, d_cdata, d_ic, ic.data(), n_chunks, E.stream.as<u8>(), E.tokens.as<u32>(), d_res, E.adler.as<u64>(),
                             max_n, d_status, E.inf_scratch.p, &E))) return rc;
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

void inflate_mark(void *engine, hipStream_t st, const char *name) { ((Engine *)engine)->t_mark(st, name); }
u8 *inflate_host_stage(void *engine, size_t bytes) { auto &v = ((Engine *)engine)->host_stage[1]; v.assign(bytes, 0); return v.data(); }

static int dev_decompress(Engine &E, hipStream_t st, const u8 *d_cdata, const long *c_off, const long *c_len, const long *n_rows,
                          int n_chunks, int nc, int sz, int flags, u8 *d_out, const long *out_off, int *status, int nc_full = 0,
                          bool add_times = false)
{
    if (sz != 1 && sz != 2 && sz != 4 && sz != 8) { set_error("itemsize %d unsupported", sz); return MTS_E_ARG; }
    if ((flags & MTS_FLAG_FLOAT) && sz != 4 && sz != 8) { set_error("float items of %d bytes unsupported", sz); return MTS_E_ARG; }
    if (nc <= 0 || n_chunks < 0) return MTS_E_ARG;
    for (int i = 0; i < n_chunks; i++)              // (K2 stores whole items; any multiple of the item size is allowed)
        if (((uintptr_t)d_out + (u64)out_off[i]) % (unsigned)sz) {
            set_error("chunk %d: output address (d_out + offset %ld) is not a multiple of the item size %d", i, out_off[i], sz);
            return MTS_E_ARG;
        }
    MTS_HIP(hipSetDevice(E.dev));
    const size_t budget = batch_budget_bytes() * 4;          // inflate needs ~5 bytes of workspace per byte
    const u64 row_bytes = (u64)(nc_full > nc ? nc_full : nc) * sz;
    int i = 0;
    bool first = !add_times;
    while (i < n_chunks) {
        int j = i;
        size_t acc = 0;
        while (j < n_chunks) {
            const size_t n = (size_t)n_rows[j] * row_bytes;
            if (j > i && (acc + n > budget || j - i >= MAX_BATCH_CHUNKS)) break;
            acc += n; j++;
        }
        int rc = decompress_batch(E, st, d_cdata, c_off + i, c_len + i, n_rows + i, j - i, nc, sz, flags, d_out, out_off + i,
                                  status + i, first ? 0 : 1, nullptr, nc_full);
        if (rc) return rc;
        first = false;
        i = j;
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

int mts_version(void) { return 100; }

int mts_device_count(void) { return device_count() > 0 ? device_count() : 0; }

const char *mts_strerror(int code)
{
    switch (code) {
    case MTS_OK: return "ok";
    case MTS_E_ARG: return "bad argument";
    case MTS_E_NODEV: return "no usable gfx950 device";
    case MTS_E_HIP: return "HIP runtime error";
    case MTS_E_NOMEM: return "out of memory";
    case MTS_E_UNSUPPORTED: return "not implemented";
    case MTS_E_INTERNAL: return "internal error";
    case MTS_E_MISS: return "chunk not resident in the device cache";
    default: return "unknown error";
    }
}

const char *mts_last_error(void) { return g_err; }

long mts_compress_bound(long raw_len) { return compress_bound(raw_len); }

// ---- decoded-chunk cache on the device (Reader random access) ------------------------------------
namespace {
struct CacheEntry { u8 *d = nullptr; u64 cap = 0, size = 0, stamp = 0; long rows = 0; int cols = 0; };      // (rows, cols) C order; cols < n_channels: the leading channels only
struct DevCache {
    int device = 0;
    u64 capacity = 0, used = 0, clock = 0;
    std::unordered_map<long, CacheEntry> map;
    std::vector<std::pair<u8 *, u64>> spare;         // buffers of evicted entries, reused for new ones
    void drop(long key)
    {
        auto it = map.find(key);
        if (it == map.end()) return;
        used -= it->second.cap;
        if (spare.size() < 4) spare.push_back({it->second.d, it->second.cap}); else (void)hipFree(it->second.d);
        map.erase(it);
    }
    // room for `need` more bytes: evict least recently used entries that this call does not use (stamp < keep_from)
    void make_room(u64 need, u64 keep_from)
    {
        while (used + need > capacity) {
            long victim = 0; u64 best = ~0ull; bool found = false;
            for (auto &kv : map) if (kv.second.stamp < keep_from && kv.second.stamp < best) { best = kv.second.stamp; victim = kv.first; found = true; }
            if (!found) break;                       // everything left belongs to this call: overshoot rather than fail
            drop(victim);
        }
    }
    int alloc(u64 size, u8 **out, u64 *cap)
    {
        for (size_t k = 0; k < spare.size(); k++)
            if (spare[k].second >= size && spare[k].second <= size + size / 2 + 4096) {
                *out = spare[k].first; *cap = spare[k].second; spare.erase(spare.begin() + k); return MTS_OK;
            }
        while (!spare.empty()) { (void)hipFree(spare.back().first); spare.pop_back(); }
        const u64 want = align_up(size ? size : 1, 4096);
        hipError_t e = hipMalloc((void **)out, want);
        if (e != hipSuccess) { set_error("hipMalloc(%llu) for the chunk cache failed: %s", (unsigned long long)want, hipGetErrorString(e)); return MTS_E_NOMEM; }
        *cap = want;
        return MTS_OK;
    }
    void clear()
    {
        for (auto &kv : map) (void)hipFree(kv.second.d);
        map.clear();
        for (auto &b : spare) (void)hipFree(b.first);
        spare.clear();
        used = 0;
    }
};
std::mutex g_cache_mu;
std::unordered_map<long, DevCache *> g_caches;
long g_cache_next = 1;
DevCache *find_cache(long id, int *device = nullptr)
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    auto it = g_caches.find(id);
    if (it == g_caches.end()) return nullptr;
    if (device) *device = it->second->device;                  // (read under the lock: the cache may be freed once it is released)
    return it->second;
}
// mts_cache_destroy unregisters a cache first and frees it under its engine's lock; an entry point that looked the cache
// up before it took that lock asks again once it holds it, and never touches a cache that has gone in between
bool cache_alive(long id, const DevCache *c) { return find_cache(id) == c; }
}  // namespace

}  // extern "C"
namespace mts {
void drop_device_caches()
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return;
    std::lock_guard<std::mutex> lk(g_cache_mu);
    for (auto &kv : g_caches) if (kv.second->device == dev) kv.second->clear();      // (the caller holds this device's engine lock)
}
}  // namespace mts
extern "C" {

void mts_release(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    for (Engine *e : g_engines)
        if (e) {
            std::lock_guard<std::mutex> l2(e->mu);
            (void)hipSetDevice(e->dev);
            e->release_all();
            std::lock_guard<std::mutex> l3(g_cache_mu);
            for (auto &kv : g_caches) if (kv.second->device == e->dev) kv.second->clear();
        }
}

int mts_dev_compress_chunks(int device, void *stream, const void *d_raw, int n_channels, int itemsize,
                            const long *chunk_bounds, int n_chunks, int flags, int level, unsigned char *d_out,
                            const long *out_slot_offsets, long *out_sizes)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(E->mu);
    return dev_compress(*E, (hipStream_t)stream, d_raw, n_channels, itemsize, chunk_bounds, n_chunks, flags, level, d_out,
                        out_slot_offsets, out_sizes);
}

int mts_compress_chunks(int device, const void *raw, int n_channels, int itemsize, const long *chunk_bounds, int n_chunks,
                        int flags, int level, unsigned char *out, const long *out_slot_offsets, long *out_sizes)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    if (n_chunks <= 0) return n_chunks == 0 ? MTS_OK : MTS_E_ARG;
    std::lock_guard<std::mutex> lk(E->mu);
    MTS_HIP(hipSetDevice(E->dev));
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
    const int np = (int)pb.size() - 1;
    const int dev = E->dev;
    auto copy_in = [&](int k) -> int {                               // the raw rows of piece k (on the calling or on a helper thread)
        MTS_HIP(hipSetDevice(dev));
        const u64 off = (u64)(chunk_bounds[pb[k]] - chunk_bounds[0]) * row_bytes, len = (u64)(chunk_bounds[pb[k + 1]] - chunk_bounds[pb[k]]) * row_bytes;
        return len ? staged_h2d(*E, E->h_in.as<u8>() + off, (const u8 *)raw + off, len) : MTS_OK;
    };
    auto copy_out = [&](int k) -> int {                              // the streams of piece k, each to its slot in the caller's buffer
        MTS_HIP(hipSetDevice(dev));
        std::vector<CopyItem> segs;
        for (int i = pb[k]; i < pb[k + 1]; i++)
            if (out_sizes[i] > 0) segs.push_back({out + out_slot_offsets[i], E->h_out.as<u8>() + slots[i], (size_t)out_sizes[i]});
        return staged_d2h_multi(*E, segs);
    };
    if ((rc = copy_in(0))) return rc;
    for (int k = 0; k < np; k++) {
        std::future<int> f_in, f_out;
        if (k + 1 < np) f_in = copy_beside(copy_in, k + 1);
        if (k >= 1) f_out = copy_beside(copy_out, k - 1);
        const u64 off = (u64)(chunk_bounds[pb[k]] - chunk_bounds[0]) * row_bytes;
        rc = dev_compress(*E, nullptr, E->h_in.as<u8>() + off, n_channels, itemsize, chunk_bounds + pb[k], pb[k + 1] - pb[k], flags, level,
                          E->h_out.as<u8>(), slots.data() + pb[k], out_sizes + pb[k], k > 0);
        const int rc_in = f_in.valid() ? f_in.get() : MTS_OK, rc_out = f_out.valid() ? f_out.get() : MTS_OK;      // (always joined: they hold references to this frame)
        if (rc || rc_in || rc_out) return rc ? rc : rc_in ? rc_in : rc_out;
    }
    return copy_out(np - 1);
}

int mts_delta_transpose(int device, const void *raw, long n_samples, int n_channels, int itemsize, int flags,
                        void *stream_out)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    if (itemsize != 1 && itemsize != 2 && itemsize != 4 && itemsize != 8) return MTS_E_ARG;
    if (n_samples < 0 || n_channels <= 0) return MTS_E_ARG;
    std::lock_guard<std::mutex> lk(E->mu);
    MTS_HIP(hipSetDevice(E->dev));
    const u64 n = (u64)n_samples * n_channels * itemsize;
    if (n == 0) return MTS_OK;
    if (n >= (1ull << 31)) return MTS_E_ARG;
    if ((rc = E->h_in.ensure(n + 256))) return rc;
    if ((rc = E->stream.ensure(n + 2 * STREAM_PAD))) return rc;
    if ((rc = E->desc.ensure(4096))) return rc;
    if ((rc = E->adler.ensure(4096))) return rc;
    ChunkDesc c; memset(&c, 0, sizeof c);
    c.n = (u32)n; c.n_rows = (u32)n_samples;
    MTS_HIP(hipMemcpy(E->h_in.p, raw, n, hipMemcpyHostToDevice));
    MTS_HIP(hipMemcpy(E->desc.p, &c, sizeof c, hipMemcpyHostToDevice));
    if ((rc = launch_delta_transpose(nullptr, E->h_in.p, E->stream.p, E->desc.as<ChunkDesc>(), 1, (u32)n_samples, n_channels,
                                     itemsize, flags, E->adler.as<u64>()))) return rc;
    MTS_HIP(hipMemcpy(stream_out, E->stream.p, n, hipMemcpyDeviceToHost));
    return MTS_OK;
}

int mts_cumsum_transpose(int device, const void *stream, long n_samples, int n_channels, int itemsize, int flags, void *out)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    if (itemsize != 1 && itemsize != 2 && itemsize != 4 && itemsize != 8) return MTS_E_ARG;
    if (n_samples < 0 || n_channels <= 0) return MTS_E_ARG;
    std::lock_guard<std::mutex> lk(E->mu);
    MTS_HIP(hipSetDevice(E->dev));
    const u64 n = (u64)n_samples * n_channels * itemsize;
    if (n == 0) return MTS_OK;
    if (n >= (1ull << 31)) return MTS_E_ARG;
    if ((rc = E->stream.ensure(n + 2 * STREAM_PAD))) return rc;
    if ((rc = E->h_out.ensure(n + 256))) return rc;
    if ((rc = E->desc.ensure(4096))) return rc;
    if ((rc = E->segsums.ensure(cumsum_scratch_bytes(1, (u32)n_samples, n_channels)))) return rc;
    struct { u64 so, oo; u32 rows; } h = {0, 0, (u32)n_samples};
    u8 *dp = E->desc.as<u8>();
    MTS_HIP(hipMemcpy(E->stream.p, stream, n, hipMemcpyHostToDevice));
    MTS_HIP(hipMemcpy(dp, &h.so, 8, hipMemcpyHostToDevice));
    MTS_HIP(hipMemcpy(dp + 8, &h.oo, 8, hipMemcpyHostToDevice));
    MTS_HIP(hipMemcpy(dp + 16, &h.rows, 4, hipMemcpyHostToDevice));
    if ((rc = launch_cumsum_transpose(nullptr, E->stream.p, E->h_out.p, (u64 *)dp, (u64 *)(dp + 8), (u32 *)(dp + 16), nullptr, 1,
                                      (u32)n_samples, n_channels, itemsize, flags, E->segsums.p))) return rc;
    MTS_HIP(hipMemcpy(out, E->h_out.p, n, hipMemcpyDeviceToHost));
    return MTS_OK;
}

int mts_dev_synth_int16(int device, void *stream, void *d_out, long t0, long t1, int n_channels, long seed)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(E->mu);
    MTS_HIP(hipSetDevice(E->dev));
    return launch_synth_int16((hipStream_t)stream, (int16_t *)d_out, t0, t1, n_channels, seed);
}

// ------------------------------------------------------------------------------------------------
// device memory for callers of the dev_* entry points: a process that keeps its recordings in HBM allocates, copies and waits
// through THIS library -- one HIP runtime per process, the one these kernels are launched with (no second runtime's handles)
// ------------------------------------------------------------------------------------------------
__global__ void k_count_diff(const u8 *__restrict__ a, const u8 *__restrict__ b, u64 n, unsigned long long *__restrict__ out /* count, first */)
{
    const u64 n16 = n / 16, stride = (u64)gridDim.x * blockDim.x;
    u32 cnt = 0;
    u64 first = ~0ull;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const uint4 x = ((const uint4 *)a)[i], y = ((const uint4 *)b)[i];
        if (x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w) {
            for (int k = 0; k < 16; k++) if (a[i * 16 + k] != b[i * 16 + k]) { cnt++; if (first == ~0ull) first = i * 16 + k; }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (u32)(n & 15)) { const u64 j = n16 * 16 + threadIdx.x; if (a[j] != b[j]) { cnt++; first = first < j ? first : j; } }
    if (cnt) { atomicAdd(&out[0], (unsigned long long)cnt); atomicMin(&out[1], (unsigned long long)first); }
}

int mts_host_alloc(long nbytes, void **h_ptr)
{
    if (nbytes < 0 || !h_ptr) return MTS_E_ARG;
    if (device_count() <= 0) { set_error("no gfx950 device visible (libmtscomp_hip has no CPU path)"); return MTS_E_NODEV; }
    void *p = nullptr;
    if (hipHostMalloc(&p, nbytes > 0 ? (size_t)nbytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); set_error("hipHostMalloc of %ld bytes failed", nbytes); return MTS_E_NOMEM; }
    *h_ptr = p;
    return MTS_OK;
}

int mts_host_free(void *h_ptr)
{
    if (h_ptr) MTS_HIP(hipHostFree(h_ptr));
    return MTS_OK;
}

int mts_dev_alloc(int device, long nbytes, void **d_ptr)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    if (nbytes < 0 || !d_ptr) return MTS_E_ARG;
    MTS_HIP(hipSetDevice(E->dev));
    void *p = nullptr;
    if (hipMalloc(&p, nbytes > 0 ? (size_t)nbytes : 1) != hipSuccess) { (void)hipGetLastError(); set_error("hipMalloc of %ld bytes failed", nbytes); return MTS_E_NOMEM; }
    *d_ptr = p;
    return MTS_OK;
}

int mts_dev_free(int device, void *d_ptr)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    MTS_HIP(hipSetDevice(E->dev));
    if (d_ptr) MTS_HIP(hipFree(d_ptr));
    return MTS_OK;
}

int mts_dev_copy(int device, void *stream, void *dst, const void *src, long nbytes, int kind)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    if (nbytes < 0 || kind < 0 || kind > 2) return MTS_E_ARG;
    MTS_HIP(hipSetDevice(E->dev));
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (nbytes) MTS_HIP(hipMemcpyAsync(dst, src, (size_t)nbytes, k, (hipStream_t)stream));
    MTS_HIP(hipStreamSynchronize((hipStream_t)stream));
    return MTS_OK;
}

int mts_dev_sync(int device)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    MTS_HIP(hipSetDevice(E->dev));
    MTS_HIP(hipDeviceSynchronize());
    return MTS_OK;
}

int mts_dev_compare(int device, void *stream, const void *d_a, const void *d_b, long nbytes, long *n_diff, long *first_diff)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    if (nbytes < 0 || !n_diff) return MTS_E_ARG;
    if (((uintptr_t)d_a | (uintptr_t)d_b) & 15) { set_error("mts_dev_compare: buffers must be 16-byte aligned"); return MTS_E_ARG; }
    std::lock_guard<std::mutex> lk(E->mu);
    MTS_HIP(hipSetDevice(E->dev));
    unsigned long long *d_out = nullptr, h[2] = {0, ~0ull};
    MTS_HIP(hipMalloc(&d_out, 16));
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(d_out, h, 16, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && nbytes) {
        hipLaunchKernelGGL(k_count_diff, dim3(2048), dim3(256), 0, st, (const u8 *)d_a, (const u8 *)d_b, (u64)nbytes, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, d_out, 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_out);
    MTS_HIP(e);
    *n_diff = (long)h[0];
    if (first_diff) *first_diff = h[0] ? (long)h[1] : -1;
    return MTS_OK;
}

int mts_last_stage_times(int device, const char **names, float *ms, int cap)
{
    Engine *E;
    if (get_engine(device, &E)) return 0;
    std::lock_guard<std::mutex> lk(E->mu);
    int n = E->n_stage_done < cap ? E->n_stage_done : cap;
    for (int i = 0; i < n; i++) { names[i] = E->done_name[i]; ms[i] = E->stage_ms[i]; }
    return n;
}


int mts_dev_decompress_chunks(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets,
                              const long *c_lengths, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags,
                              void *d_out, const long *out_offsets, int *chunk_status)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(E->mu);
    return dev_decompress(*E, (hipStream_t)stream, d_cdata, c_offsets, c_lengths, n_rows, n_chunks, n_channels, itemsize, flags,
                          (u8 *)d_out, out_offsets, chunk_status);
}

int mts_decompress_chunks(int device, const unsigned char *cdata, const long *c_offsets, const long *c_lengths,
                          const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, void *out,
                          const long *out_offsets, int *chunk_status)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    if (n_chunks <= 0) return n_chunks == 0 ? MTS_OK : MTS_E_ARG;
    std::lock_guard<std::mutex> lk(E->mu);
    MTS_HIP(hipSetDevice(E->dev));
    const u64 row_bytes = (u64)n_channels * itemsize;
    std::vector<long> coff(n_chunks), ooff(n_chunks);
    u64 ctot = 0, otot = 0;
    for (int i = 0; i < n_chunks; i++) {
        if (c_lengths[i] < 0 || n_rows[i] < 0) return MTS_E_ARG;
        coff[i] = (long)ctot; ctot += align_up((u64)c_lengths[i] + 8, 16);
        ooff[i] = (long)otot; otot += align_up((u64)n_rows[i] * row_bytes, 256);
    }
    // the compressed bytes: when the chunks lie (nearly) back to back in the caller's buffer -- a range read from a .cbin --
    // the whole range crosses the bus in one staged copy and the chunks keep their distances; otherwise chunk by chunk
    long lo = c_offsets[0], hi = c_offsets[0] + c_lengths[0];
    u64 sum = 0;
    for (int i = 0; i < n_chunks; i++) {
        if (c_offsets[i] < lo) lo = c_offsets[i];
        if (c_offsets[i] + c_lengths[i] > hi) hi = c_offsets[i] + c_lengths[i];
        sum += (u64)c_lengths[i];
    }
    const bool one_range = lo >= 0 && (u64)(hi - lo) <= sum + sum / 4 + 4096;
    if (one_range) { ctot = (u64)(hi - lo) + 16; for (int i = 0; i < n_chunks; i++) coff[i] = c_offsets[i] - lo; }
    if ((rc = E->h_in.ensure(ctot + 256))) return rc;
    if ((rc = E->h_out.ensure(otot + 256))) return rc;
    // piece by piece (see pipe_pieces) when the compressed chunks lie in file order in one range: piece k's bytes are then one
    // range of the caller's buffer as well
    bool ascending = true;
    for (int i = 1; i < n_chunks && ascending; i++) ascending = c_offsets[i] >= c_offsets[i - 1] + c_lengths[i - 1];
    std::vector<int> pb = {0, n_chunks};
    if (!one_range || ascending) pb = pipe_pieces(n_rows, false, n_chunks, row_bytes);
    const int np = (int)pb.size() - 1;
    const int dev = E->dev;
    auto copy_in = [&](int k) -> int {
        MTS_HIP(hipSetDevice(dev));
        if (one_range) {
            const long a = k == 0 ? lo : c_offsets[pb[k]], b = k + 1 == np ? hi : c_offsets[pb[k + 1]];
            return b > a ? staged_h2d(*E, E->h_in.as<u8>() + (a - lo), cdata + a, (size_t)(b - a)) : MTS_OK;
        }
        for (int i = pb[k]; i < pb[k + 1]; i++)                       // chunks that lie apart in the caller's memory: one copy each
            if (c_lengths[i]) { const int rc1 = staged_h2d(*E, E->h_in.as<u8>() + coff[i], cdata + c_offsets[i], (size_t)c_lengths[i]); if (rc1) return rc1; }
        return MTS_OK;
    };
    auto copy_out = [&](int k) -> int {
        MTS_HIP(hipSetDevice(dev));
        std::vector<CopyItem> segs;
        for (int i = pb[k]; i < pb[k + 1]; i++)
            if (chunk_status[i] == MTS_CHUNK_OK && n_rows[i])
                segs.push_back({(u8 *)out + out_offsets[i], E->h_out.as<u8>() + ooff[i], (size_t)((u64)n_rows[i] * row_bytes)});
        return staged_d2h_multi(*E, segs);
    };
    if ((rc = copy_in(0))) return rc;
    for (int k = 0; k < np; k++) {
        std::future<int> f_in, f_out;
        if (k + 1 < np) f_in = copy_beside(copy_in, k + 1);
        if (k >= 1) f_out = copy_beside(copy_out, k - 1);
        rc = dev_decompress(*E, nullptr, E->h_in.as<u8>(), coff.data() + pb[k], c_lengths + pb[k], n_rows + pb[k], pb[k + 1] - pb[k], n_channels,
                            itemsize, flags, E->h_out.as<u8>(), ooff.data() + pb[k], chunk_status + pb[k], 0, k > 0);
        const int rc_in = f_in.valid() ? f_in.get() : MTS_OK, rc_out = f_out.valid() ? f_out.get() : MTS_OK;
        if (rc || rc_in || rc_out) return rc ? rc : rc_in ? rc_in : rc_out;
    }
    return copy_out(np - 1);
}

// ---- decoded-chunk cache: entry points (state above mts_release) ----------------------------------

int mts_cache_create(int device, long capacity_bytes, long *cache_id)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    if (!cache_id || capacity_bytes < 0) return MTS_E_ARG;
    DevCache *c = new DevCache();
    c->device = device; c->capacity = (u64)capacity_bytes;
    std::lock_guard<std::mutex> lk(g_cache_mu);
    *cache_id = g_cache_next++;
    g_caches[*cache_id] = c;
    return MTS_OK;
}

int mts_cache_destroy(long cache_id)
{
    DevCache *c;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        auto it = g_caches.find(cache_id);
        if (it == g_caches.end()) return MTS_E_ARG;
        c = it->second;
        g_caches.erase(it);                                    // from here on no entry point starts on this cache; those inside finish first (engine lock)
    }
    Engine *E;
    if (get_engine(c->device, &E) == MTS_OK) {
        std::lock_guard<std::mutex> lk(E->mu);
        (void)hipSetDevice(E->dev);
        c->clear();
    }
    delete c;
    return MTS_OK;
}

int mts_cache_query(long cache_id, const long *chunk_keys, int n, int *present)
{
    int dev = 0;
    DevCache *c = find_cache(cache_id, &dev);
    if (!c || n < 0) return MTS_E_ARG;
    Engine *E;
    int rc = get_engine(dev, &E);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(E->mu);
    if (!cache_alive(cache_id, c)) return MTS_E_ARG;
    for (int i = 0; i < n; i++) {           // 0: not resident, else the number of (leading) channels the entry holds
        auto it = c->map.find(chunk_keys[i]);
        present[i] = it == c->map.end() ? 0 : it->second.cols > 0 ? it->second.cols : 1;
    }
    return MTS_OK;
}

// make every listed chunk resident (decode the missing ones in one batch) and pin them for this call by their stamp
static int cache_ensure(DevCache *c, Engine *E, int n_chunks, const long *chunk_keys, const unsigned char *cdata, const long *c_offsets,
                        const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, int *chunk_status, u64 call_stamp,
                        long *total_rows_out, int n_cols /* leading channels wanted: n_channels = whole chunks */)
{
    int rc;
    std::vector<int> miss;
    long total_rows = 0;
    {   // every key once: a key listed twice would be decoded and accounted twice
        std::vector<long> keys(chunk_keys, chunk_keys + n_chunks);
        std::sort(keys.begin(), keys.end());
        if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) { set_error("a chunk key is listed twice"); return MTS_E_ARG; }
    }
    auto usable = [&](int i) -> bool {
        auto it = c->map.find(chunk_keys[i]);
        return it != c->map.end() && it->second.rows == n_rows[i] && it->second.cols >= n_cols && it->second.cols <= n_channels &&
               it->second.size == (u64)n_rows[i] * it->second.cols * itemsize;
    };
    for (int i = 0; i < n_chunks; i++) {          // every key is looked at before anything is dropped: a miss leaves the cache as it was
        if (n_rows[i] < 0) return MTS_E_ARG;
        if (!usable(i) && c_lengths[i] <= 0) {
            set_error("chunk key %ld is not resident%s and no compressed bytes were given", chunk_keys[i], c->map.count(chunk_keys[i]) ? " with the channels asked for" : "");
            return MTS_E_MISS;
        }
    }
    for (int i = 0; i < n_chunks; i++) {
        total_rows += n_rows[i];
        chunk_status[i] = MTS_CHUNK_OK;
        if (usable(i)) { c->map.find(chunk_keys[i])->second.stamp = call_stamp; continue; }
        c->drop(chunk_keys[i]);                    // same key, other shape or fewer channels: decoded again
        miss.push_back(i);
    }
    *total_rows_out = total_rows;
    auto all_resident = [&]() -> int {            // (a workspace allocation that failed may have emptied the caches of this device)
        for (int i = 0; i < n_chunks; i++)
            if (chunk_status[i] == MTS_CHUNK_OK && !c->map.count(chunk_keys[i])) { set_error("chunk key %ld was dropped from the cache during the call", chunk_keys[i]); return MTS_E_MISS; }
        return MTS_OK;
    };
    if (miss.empty()) return all_resident();
    static const bool times = getenv("MTS_CACHE_TIMES") != nullptr;      // (where a cold read's time goes: stderr, one line per call)
    const auto t_0 = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_0).count(); };
    double t_h2d = 0, t_dec = 0;
    const int m = (int)miss.size();
    const u64 row_bytes = (u64)n_cols * itemsize;              // of what is decoded and kept
    std::vector<long> coff(m), clen(m), rows(m), ooff(m);
    std::vector<int> st(m);
    u64 ctot = 0, otot = 0;
    for (int k = 0; k < m; k++) {
        const int i = miss[k];
        clen[k] = c_lengths[i]; rows[k] = n_rows[i];
        // (chunks that lie back to back in the caller's buffer keep their distances on the device: one copy moves the run)
        const bool joins = k > 0 && c_offsets[i] == c_offsets[miss[k - 1]] + clen[k - 1];
        if (!joins) ctot = align_up(ctot + (k ? 16 : 0), 16);
        coff[k] = (long)ctot; ctot += (u64)clen[k];
        ooff[k] = (long)otot; otot += align_up((u64)rows[k] * row_bytes, 256);
    }
    ctot += 16;
    if ((rc = E->h_in.ensure(ctot + 256))) return rc;
    if ((rc = E->h_out.ensure(otot + 256))) return rc;
    // the compressed bytes: chunks that lie back to back in the caller's buffer (a range read or mapped from a .cbin) cross in ONE
    // staged copy -- page-locked memory by DMA as it is, anything else (a mapping of the file, a bytes object) through the
    // page-locked pieces, copied by the host threads while the DMA of the piece before runs
    for (int k = 0; k < m;) {
        int j = k + 1;
        while (j < m && c_offsets[miss[j]] == c_offsets[miss[j - 1]] + clen[j - 1] && coff[j] == coff[j - 1] + clen[j - 1]) j++;
        u64 len = 0;
        for (int q = k; q < j; q++) len += (u64)clen[q];
        if (len && (rc = staged_h2d(*E, E->h_in.as<u8>() + coff[k], cdata + c_offsets[miss[k]], (size_t)len))) return rc;
        k = j;
    }
    if (times) t_h2d = since();
    rc = dev_decompress(*E, nullptr, E->h_in.as<u8>(), coff.data(), clen.data(), rows.data(), m, n_cols, itemsize, flags,
                        E->h_out.as<u8>(), ooff.data(), st.data(), n_channels);
    if (rc) return rc;
    if (times) t_dec = since();
    for (int k = 0; k < m; k++) {
        const int i = miss[k];
        if (st[k] == MTS_CHUNK_NEEDMORE) {
            set_error("chunk key %ld: the %ld compressed bytes given do not reach the %d leading channels asked for", chunk_keys[i], clen[k], n_cols);
            return MTS_E_MISS;
        }
        chunk_status[i] = st[k];
        if (st[k] != MTS_CHUNK_OK) continue;
        const u64 size = (u64)rows[k] * row_bytes;
        CacheEntry e;
        c->make_room(align_up(size ? size : 1, 4096), call_stamp);
        if ((rc = c->alloc(size, &e.d, &e.cap))) return rc;
        e.size = size; e.rows = rows[k]; e.cols = n_cols; e.stamp = call_stamp;
        if (size) MTS_HIP(hipMemcpyAsync(e.d, E->h_out.as<u8>() + ooff[k], (size_t)size, hipMemcpyDeviceToDevice, nullptr));
        c->used += e.cap;
        c->map[chunk_keys[i]] = e;
    }
    if (times) { (void)hipStreamSynchronize(nullptr); fprintf(stderr, "[cache] %d chunks: copy in %.3f ms, decode %.3f ms, entries %.3f ms\n", m, t_h2d, t_dec - t_h2d, since() - t_dec); }
    return all_resident();
}

int mts_cache_read_rows(long cache_id, int n_chunks, const long *chunk_keys, const unsigned char *cdata, const long *c_offsets,
                        const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_begin,
                        long row_end, void *out, int *chunk_status)
{
    int dev = 0;
    DevCache *c = find_cache(cache_id, &dev);
    if (!c || n_chunks < 0 || n_channels <= 0 || row_begin < 0 || row_end < row_begin) return MTS_E_ARG;
    Engine *E;
    int rc = get_engine(dev, &E);
    if (rc) return rc;
    if (n_chunks == 0) return row_end == 0 ? MTS_OK : MTS_E_ARG;
    std::lock_guard<std::mutex> lk(E->mu);
    if (!cache_alive(cache_id, c)) return MTS_E_ARG;         // (destroyed while this call waited for the engine)
    MTS_HIP(hipSetDevice(E->dev));
    const u64 row_bytes = (u64)n_channels * itemsize;
    const u64 call_stamp = ++c->clock;
    long total_rows = 0;
    if ((rc = cache_ensure(c, E, n_chunks, chunk_keys, cdata, c_offsets, c_lengths, n_rows, n_channels, itemsize, flags, chunk_status, call_stamp, &total_rows, n_channels))) return rc;
    if (row_end > total_rows) return MTS_E_ARG;
    // rows [row_begin, row_end) of the concatenation, straight from the resident chunks
    long r0 = 0;
    for (int i = 0; i < n_chunks; i++) {
        const long r1 = r0 + n_rows[i];
        const long lo = row_begin > r0 ? row_begin : r0, hi = row_end < r1 ? row_end : r1;
        if (lo < hi && chunk_status[i] == MTS_CHUNK_OK) {
            const CacheEntry &e = c->map[chunk_keys[i]];
            MTS_HIP(hipMemcpyAsync((u8 *)out + (u64)(lo - row_begin) * row_bytes, e.d + (u64)(lo - r0) * row_bytes,
                                   (size_t)((u64)(hi - lo) * row_bytes), hipMemcpyDeviceToHost, nullptr));
        }
        r0 = r1;
    }
    MTS_HIP(hipStreamSynchronize(nullptr));
    c->make_room(0, ~0ull);                         // back under the capacity (this call's chunks may go too)
    return MTS_OK;
}

int mts_cache_read_slices_leading(long cache_id, int n_chunks, const long *chunk_keys, const unsigned char *cdata, const long *c_offsets,
                                  const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, int n_leading,
                                  int n_req, const long *req, void *out, const long *out_offsets, long out_bytes, int *chunk_status)
{
    if (n_leading <= 0 || n_leading > n_channels) return MTS_E_ARG;
    if (n_leading < n_channels && (!(flags & MTS_FLAG_ORDER_F) || (flags & MTS_FLAG_FLOAT))) {
        set_error("leading channels alone can only be decoded from channel-major integer chunks");
        return MTS_E_ARG;
    }
    int dev = 0;
    DevCache *c = find_cache(cache_id, &dev);
    if (!c || n_chunks < 0 || n_channels <= 0 || n_req < 0 || out_bytes < 0) return MTS_E_ARG;
    if (itemsize != 1 && itemsize != 2 && itemsize != 4 && itemsize != 8) return MTS_E_ARG;
    Engine *E;
    int rc = get_engine(dev, &E);
    if (rc) return rc;
    if (n_chunks == 0 || n_req == 0) return MTS_OK;
    std::lock_guard<std::mutex> lk(E->mu);
    if (!cache_alive(cache_id, c)) return MTS_E_ARG;
    MTS_HIP(hipSetDevice(E->dev));
    const u64 call_stamp = ++c->clock;
    // the requests first: their sizes are known without the chunks, and every allocation of this call has to come BEFORE the
    // residency check -- a workspace allocation that fails once drops this device's decoded chunks (DBuf::ensure)
    long total_rows = 0;
    for (int i = 0; i < n_chunks; i++) { if (n_rows[i] < 0) return MTS_E_ARG; total_rows += n_rows[i]; }
    std::vector<GatherReq> gr(n_req);
    u64 max_items = 0;
    for (int k = 0; k < n_req; k++) {
        const long *q = req + 6 * k;
        if (q[0] < 0 || q[1] < q[0] || q[1] > total_rows || q[2] < 1 || q[3] < 0 || q[4] < q[3] || q[4] > n_leading || q[5] < 1) return MTS_E_ARG;
        GatherReq &g = gr[k];
        g.rb = q[0]; g.rs = q[2]; g.cb = q[3]; g.cs = q[5];
        g.nr = (q[1] - q[0] + q[2] - 1) / q[2]; g.ncol = (q[4] - q[3] + q[5] - 1) / q[5];
        g.out_off = out_offsets[k];
        if (out_offsets[k] < 0 || (u64)out_offsets[k] + (u64)g.nr * g.ncol * itemsize > (u64)out_bytes) return MTS_E_ARG;
        if (out_offsets[k] % itemsize) { set_error("request %d: output offset %ld is not a multiple of the item size", k, out_offsets[k]); return MTS_E_ARG; }
        if ((u64)g.nr * g.ncol > max_items) max_items = (u64)g.nr * g.ncol;
    }
    const size_t o_req = align_up(sizeof(GatherChunk) * n_chunks, 256), desc = o_req + align_up(sizeof(GatherReq) * n_req, 256);
    if ((rc = E->misc.ensure(desc + 256))) return rc;
    if ((rc = E->h_out.ensure((u64)out_bytes + 256))) return rc;
    long total_rows_seen = 0;
    if ((rc = cache_ensure(c, E, n_chunks, chunk_keys, cdata, c_offsets, c_lengths, n_rows, n_channels, itemsize, flags, chunk_status, call_stamp, &total_rows_seen, n_leading))) return rc;
    // (cache_ensure ends with the residency check and nothing below allocates: the base pointers stay valid)
    std::vector<GatherChunk> gc(n_chunks);
    long r0 = 0;
    for (int i = 0; i < n_chunks; i++) {
        gc[i].row0 = r0; r0 += n_rows[i];
        if (chunk_status[i] == MTS_CHUNK_OK) { const CacheEntry &e = c->map[chunk_keys[i]]; gc[i].base = e.d; gc[i].pitch = e.cols; }
        else { gc[i].base = nullptr; gc[i].pitch = n_channels; }
    }
    MTS_HIP(hipMemcpyAsync(E->misc.p, gc.data(), sizeof(GatherChunk) * n_chunks, hipMemcpyHostToDevice, nullptr));
    MTS_HIP(hipMemcpyAsync(E->misc.as<u8>() + o_req, gr.data(), sizeof(GatherReq) * n_req, hipMemcpyHostToDevice, nullptr));
    if (max_items && (rc = launch_gather_slices(nullptr, (const GatherChunk *)E->misc.p, n_chunks, (const GatherReq *)(E->misc.as<u8>() + o_req), n_req, max_items,
                                                n_channels, itemsize, E->h_out.as<u8>()))) return rc;
    if (out_bytes) MTS_HIP(hipMemcpyAsync(out, E->h_out.p, (size_t)out_bytes, hipMemcpyDeviceToHost, nullptr));      // the requested items, nothing else, in one copy
    MTS_HIP(hipStreamSynchronize(nullptr));
    c->make_room(0, ~0ull);
    return MTS_OK;
}

int mts_cache_read_slices(long cache_id, int n_chunks, const long *chunk_keys, const unsigned char *cdata, const long *c_offsets,
                          const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, int n_req,
                          const long *req, void *out, const long *out_offsets, long out_bytes, int *chunk_status)
{
    return mts_cache_read_slices_leading(cache_id, n_chunks, chunk_keys, cdata, c_offsets, c_lengths, n_rows, n_channels, itemsize, flags, n_channels,
                                         n_req, req, out, out_offsets, out_bytes, chunk_status);
}

int mts_debug_inflate(int device, const unsigned char *zbytes, long zlen, unsigned char *out, long out_cap, long *out_len, int *status)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    if (zlen < 0 || out_cap < 0) return MTS_E_ARG;
    std::lock_guard<std::mutex> lk(E->mu);
    MTS_HIP(hipSetDevice(E->dev));
    if ((rc = E->h_in.ensure((u64)zlen + 256))) return rc;
    if (zlen) MTS_HIP(hipMemcpy(E->h_in.p, zbytes, (size_t)zlen, hipMemcpyHostToDevice));
    // the expected size is the caller's out_cap: status BADSIZE when the stream inflates to anything else
    const long coff = 0, clen = zlen, rows = out_cap, ooff = 0;
    rc = decompress_batch(*E, nullptr, E->h_in.as<u8>(), &coff, &clen, &rows, 1, 1, 1, 0, nullptr, &ooff, status, 0, out);
    if (rc) return rc;
    if (out_len) *out_len = *status == MTS_CHUNK_OK ? out_cap : 0;
    return MTS_OK;
}

}  // extern "C"

// ================================================================================================
// How a reduction is fed (window_stats_run, rank_hist_run, decimate_run, welch_run, gram_run)
// ================================================================================================
// A reduction reads the rows of some chunks and never keeps them.  A chunk that is whole in the call's device cache (resident) is read
// where it lies; every other chunk (missing) comes with its compressed bytes and is decoded into the piece workspace E.h_out.  The
// missing chunks are cut into pieces of MTS_PIPE_BYTES of decoded bytes (pipe_pieces; resident chunks weigh nothing, device input is
// one piece: nothing to copy beside the kernels, and smaller batches inflate slower): while piece p is decoded and reduced, the
// compressed bytes of piece p + 1 cross the bus on a helper thread.  Two families share this code:
//   tiles (window_stats, rank_hist): a chunk's rows are cut into tiles that are reduced on their own, so the resident chunks go first
//        and each piece decodes exactly its own missing chunks (TilePlan);
//   halo (decimate, welch, gram): a unit of output (outputs, blocks, groups -- the op maps them to pieces itself) reads rows of
//        several adjacent chunks, so a piece reads chunks [c0, c1] through a table of segment bases and first rows, and decodes the
//        missing ones among them -- a boundary chunk in both pieces (plan_pieces, segment_tables).
// What every caller keeps to, and feed_pieces and ChunkFeed hold up:
//   - An allocation that fails empties this device's caches before it tries again (DBuf::ensure -> drop_device_caches: hipFree,
//     which waits for the kernels already launched -- earlier reads are done).  So every allocation of the call (the op's own DBuf,
//     then ChunkFeed::ensure) comes BEFORE the first use of a resident entry's address, and ensure looks every resident entry up
//     again: a call whose entries went ends with MTS_E_MISS (the Reader sends every chunk's bytes once more).
//   - A decode allocates again (decompress_batch).  The tile family therefore reduces the resident tiles and waits for the stream
//     before the first decode (only when there are resident tiles); the halo family checks after each piece's decode and before its
//     launch that every resident chunk the piece reads is still in the cache at the address its table holds (still_placed).
//   - The helper thread's copy of piece p + 1 starts before piece p's decode and is always joined before feed_pieces returns, on
//     error paths too: it holds references to the caller's frame.
//   - The first dev_decompress of a call starts the stage times (add_times false), every later one adds to them.
//   - The compressed bytes of the missing chunks lie in E.h_in in chunk order, at mcoff[]: chunks back to back in the caller's buffer
//     keep their distances (a run of them with adjacent chunk indices is one staged copy), a gap starts at the next multiple of 16.
namespace {

int check_items(int sz, int flags)
{
    if (sz != 1 && sz != 2 && sz != 4 && sz != 8) { set_error("itemsize %d unsupported", sz); return MTS_E_ARG; }
    if ((flags & MTS_FLAG_FLOAT) && sz != 4 && sz != 8) { set_error("float items of %d bytes unsupported", sz); return MTS_E_ARG; }
    return MTS_OK;
}

int check_columns(const int *cols, int n_cols, int nc)
{
    for (int j = 0; j < n_cols; j++)
        if (cols[j] < 0 || cols[j] >= nc) { set_error("column %d out of range (%d channels)", cols[j], nc); return MTS_E_ARG; }
    return MTS_OK;
}

// adjacent: every chunk begins where the one before it ends (the halo family); else the chunks are in order, do not overlap and each
// holds a row of [row_begin, row_end) (the tile family)
int check_chunk_table(bool adjacent, bool have_cache, const long *c_len, const long *row0, const long *n_rows, int n_chunks, int nc, int sz,
                      long row_begin = 0, long row_end = 0)
{
    for (int i = 0; i < n_chunks; i++) {
        if (n_rows[i] <= 0 || row0[i] < 0 || c_len[i] < 0) { set_error("chunk %d: rows or bytes invalid", i); return MTS_E_ARG; }
        if (adjacent) {
            if (i && row0[i] != row0[i - 1] + n_rows[i - 1]) { set_error("chunk %d: chunks must be adjacent", i); return MTS_E_ARG; }
        } else {
            if (i && row0[i] < row0[i - 1] + n_rows[i - 1]) { set_error("chunk %d: rows out of order or overlapping", i); return MTS_E_ARG; }
            if (row0[i] >= row_end || row0[i] + n_rows[i] <= row_begin) { set_error("chunk %d holds no row of [%ld, %ld)", i, row_begin, row_end); return MTS_E_ARG; }
        }
        if (!have_cache && c_len[i] == 0) { set_error("chunk %d: no compressed bytes and no cache", i); return MTS_E_ARG; }
        if (c_len[i] && (u64)n_rows[i] * nc * sz >= (1ull << 31)) { set_error("chunk %d: chunks must be < 2 GiB", i); return MTS_E_ARG; }
    }
    return MTS_OK;
}

// the chunk holding `row` (clamped to the chunks)
int chunk_of(const long *row0, int n_chunks, long row)
{
    int lo = 0, hi = n_chunks - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) / 2; if (row0[mid] <= row) lo = mid; else hi = mid - 1; }
    return lo;
}

// one piece: the missing chunks `miss` (ascending) are decoded to E.h_out + ooff[]; a halo piece covers the op's units [u0, u1) and
// reads chunks [c0, c1] (c1 < c0: nothing to read)
struct FeedPiece {
    long u0 = 0, u1 = 0;
    int c0 = 0, c1 = -1;
    std::vector<int> miss;
    std::vector<long> ooff;
    u64 ws = 0;
    void add(int chunk, u64 bytes) { miss.push_back(chunk); ooff.push_back((long)ws); ws += align_up(bytes, 256); }
};

// which chunks of a call are resident, where the bytes of the others lie, and their way into E.h_out
struct ChunkFeed {
    DevCache *cache;
    const long *keys;
    const u8 *cdata;
    bool on_device;
    const long *c_off, *c_len, *n_rows;
    int n_chunks, nc, sz;
    u64 row_bytes;
    std::vector<char> resident, copied;
    std::vector<const u8 *> res_ptr;                          // the address of each resident entry the tables hold (halo family)
    std::vector<long> mcoff;                                  // per missing chunk: its compressed bytes in src()
    u64 ctot = 0;
    bool any_miss = false, first_decode = true;

    ChunkFeed(DevCache *cache_, const long *keys_, const u8 *cdata_, bool on_device_, const long *c_off_, const long *c_len_,
              const long *n_rows_, int n_chunks_, int nc_, int sz_)
        : cache(cache_), keys(keys_), cdata(cdata_), on_device(on_device_), c_off(c_off_), c_len(c_len_), n_rows(n_rows_), n_chunks(n_chunks_),
          nc(nc_), sz(sz_), row_bytes((u64)nc_ * sz_), resident(n_chunks_, 0), copied(n_chunks_, 0), res_ptr(n_chunks_, nullptr),
          mcoff(n_chunks_, 0) {}

    const CacheEntry *entry_of(int i) const                   // chunk i whole in the cache, or nullptr
    {
        if (!cache) return nullptr;
        auto it = cache->map.find(keys[i]);
        if (it == cache->map.end()) return nullptr;
        const CacheEntry &e = it->second;
        return e.rows == n_rows[i] && e.cols == nc && e.size == (u64)n_rows[i] * nc * sz ? &e : nullptr;
    }
    long key_of(int i) const { return keys ? keys[i] : (long)i; }
    const u8 *src(Engine &E) const { return on_device ? cdata : E.h_in.as<u8>(); }

    // resident or missing (a missing chunk without bytes: MTS_E_MISS), and the layout of the missing chunks' bytes in E.h_in
    int classify()
    {
        int prev = -1;
        for (int i = 0; i < n_chunks; i++) {
            if (entry_of(i)) { resident[i] = 1; continue; }
            if (c_len[i] == 0) { set_error("chunk key %ld is not resident and no compressed bytes were given", key_of(i)); return MTS_E_MISS; }
            any_miss = true;
            if (on_device) { mcoff[i] = c_off[i]; continue; }
            const bool joins = prev >= 0 && c_off[i] == c_off[prev] + c_len[prev];
            if (!joins) ctot = align_up(ctot + (prev >= 0 ? 16 : 0), 16);
            mcoff[i] = (long)ctot; ctot += (u64)c_len[i];
            prev = i;
        }
        ctot += 16;
        return MTS_OK;
    }

    // chunks [pb[p], pb[p + 1]) are decoded in piece p
    std::vector<int> piece_bounds() const
    {
        if (on_device) return {0, n_chunks};
        std::vector<long> weight(n_chunks, 0);
        for (int i = 0; i < n_chunks; i++) if (!resident[i]) weight[i] = n_rows[i];
        return pipe_pieces(weight.data(), false, n_chunks, row_bytes);
    }

    // the last allocations of the call (after the op's own), then the resident entries once more
    int ensure(Engine &E, u64 piece_cap)
    {
        int rc;
        if (any_miss && !on_device && (rc = E.h_in.ensure(ctot + 256))) return rc;
        if (piece_cap && (rc = E.h_out.ensure(piece_cap + 256))) return rc;
        for (int i = 0; i < n_chunks; i++)
            if (resident[i] && !entry_of(i)) { set_error("chunk key %ld was dropped from the cache during the call", key_of(i)); return MTS_E_MISS; }
        return MTS_OK;
    }

    // the compressed bytes of `chunks` (ascending, missing) into E.h_in, each chunk once in a call; runs on the helper thread
    int copy_in(Engine &E, const std::vector<int> &chunks)
    {
        if (on_device) return MTS_OK;
        MTS_HIP(hipSetDevice(E.dev));
        for (size_t a = 0; a < chunks.size();) {
            if (copied[chunks[a]]) { a++; continue; }
            size_t e = a + 1;                                     // a run of chunks back to back here and in the caller's buffer
            while (e < chunks.size() && !copied[chunks[e]] && chunks[e] == chunks[e - 1] + 1 &&
                   c_off[chunks[e]] == c_off[chunks[e - 1]] + c_len[chunks[e - 1]] && mcoff[chunks[e]] == mcoff[chunks[e - 1]] + c_len[chunks[e - 1]]) e++;
            u64 len = 0;
            for (size_t z = a; z < e; z++) { len += (u64)c_len[chunks[z]]; copied[chunks[z]] = 1; }
            if (len) { const int rc = staged_h2d(E, E.h_in.as<u8>() + mcoff[chunks[a]], cdata + c_off[chunks[a]], (size_t)len); if (rc) return rc; }
            a = e;
        }
        return MTS_OK;
    }

    // a piece's missing chunks into E.h_out; status[] of each of them
    int decode(Engine &E, hipStream_t st, const FeedPiece &P, int dflags, int *status)
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
            if (!e || e->d != res_ptr[i]) { set_error("chunk key %ld was dropped from the cache during the call", key_of(i)); return MTS_E_MISS; }
        }
        return MTS_OK;
    }
};

// piece after piece: the next piece's bytes are copied beside this piece's decode and launch(p)
template <class Launch>
int feed_pieces(ChunkFeed &F, Engine &E, hipStream_t st, const std::vector<FeedPiece> &pieces, int dflags, int *status, Launch &&launch)
{
    auto copy_in = [&](int p) -> int { return F.copy_in(E, pieces[p].miss); };
    const int np = (int)pieces.size();
    int rc;
    if (np > 0 && (rc = copy_in(0))) return rc;
    for (int p = 0; p < np; p++) {
        std::future<int> f_in;
        if (p + 1 < np) f_in = copy_beside(copy_in, p + 1);
        rc = F.decode(E, st, pieces[p], dflags, status);
        if (!rc) rc = launch(p);
        const int rc_in = f_in.valid() ? f_in.get() : MTS_OK;      // (always joined: it holds references to this frame)
        if (rc || rc_in) return rc ? rc : rc_in;
    }
    return MTS_OK;
}

// ---- halo family: the chunks [c0, c1] of every piece are set by the op
// fills miss / ooff / ws of every piece; -> where each piece's segment table begins ((c1 - c0 + 1) bases, then (c1 - c0 + 2) first rows)
std::vector<long> plan_pieces(const ChunkFeed &F, std::vector<FeedPiece> &pieces, u64 *piece_cap)
{
    std::vector<long> seg_at(pieces.size() + 1, 0);
    *piece_cap = 0;
    for (size_t p = 0; p < pieces.size(); p++) {
        FeedPiece &P = pieces[p];
        for (int i = P.c0; i <= P.c1; i++) if (!F.resident[i]) P.add(i, (u64)F.n_rows[i] * F.row_bytes);
        *piece_cap = std::max(*piece_cap, P.ws);
        seg_at[p + 1] = seg_at[p] + 2l * (P.c1 - P.c0 + 1) + 1;
    }
    return seg_at;
}

// the segment tables, one after the other (after ChunkFeed::ensure: they hold the resident entries' addresses, kept in F.res_ptr)
std::vector<long> segment_tables(ChunkFeed &F, Engine &E, const std::vector<FeedPiece> &pieces, const std::vector<long> &seg_at, const long *row0)
{
    std::vector<long> seg(seg_at.back() + 1, 0);
    for (int i = 0; i < F.n_chunks; i++) if (F.resident[i]) F.res_ptr[i] = F.entry_of(i)->d;
    for (size_t p = 0; p < pieces.size(); p++) {
        const FeedPiece &P = pieces[p];
        long *b = seg.data() + seg_at[p], *r = b + (P.c1 - P.c0 + 1);
        size_t m = 0;
        for (int i = P.c0; i <= P.c1; i++) {
            const u8 *base = F.resident[i] ? F.res_ptr[i] : E.h_out.as<u8>() + P.ooff[m++];
            b[i - P.c0] = (long)(uintptr_t)base;
            r[i - P.c0] = row0[i];
        }
        r[P.c1 - P.c0 + 1] = P.c1 >= P.c0 ? row0[P.c1] + F.n_rows[P.c1] : 0;
    }
    return seg;
}

// ---- tile family: the rows of every (chunk ∩ window) segment cut into tiles of tile_rows rows, in row order
struct TilePlan {
    std::vector<StatTile> tiles;
    std::vector<long> tile_win, chunk_tile0;
    std::vector<FeedPiece> pieces;
    u64 piece_cap = 0;
    std::vector<int> ids;                                     // the tiles in launch order: the resident chunks', then piece after piece
    std::vector<long> launch0;                                // ids [launch0[0], launch0[1]): resident, [launch0[1 + p], launch0[2 + p]): piece p

    TilePlan(const ChunkFeed &F, const long *row0, long row_begin, long row_end, long window_rows, long tile_rows) : chunk_tile0(F.n_chunks + 1)
    {
        for (int i = 0; i < F.n_chunks; i++) {
            chunk_tile0[i] = (long)tiles.size();
            const long a = row0[i] > row_begin ? row0[i] : row_begin, b = row0[i] + F.n_rows[i] < row_end ? row0[i] + F.n_rows[i] : row_end;
            for (long r = a; r < b;) {
                const long w = (r - row_begin) / window_rows, wend = row_begin + (w + 1) * window_rows, e = b < wend ? b : wend;
                for (long q = r; q < e; q += tile_rows) {
                    StatTile t;
                    t.base = nullptr; t.row_lo = q - row0[i]; t.n_rows = (e - q) < tile_rows ? (e - q) : tile_rows; t.chunk = i; t.pad = 0;
                    tiles.push_back(t);
                    tile_win.push_back(w);
                }
                r = e;
            }
        }
        chunk_tile0[F.n_chunks] = (long)tiles.size();
        const std::vector<int> pb = F.piece_bounds();
        for (size_t p = 0; p + 1 < pb.size(); p++) {
            FeedPiece P;
            for (int i = pb[p]; i < pb[p + 1]; i++) if (!F.resident[i]) P.add(i, (u64)F.n_rows[i] * F.row_bytes);
            if (P.miss.empty()) continue;
            piece_cap = std::max(piece_cap, P.ws);
            pieces.push_back(std::move(P));
        }
    }

    // after ChunkFeed::ensure: the tiles' bases and the order of the launches; resident chunks are ok and their status is set
    void place(const ChunkFeed &F, Engine &E, std::vector<int> &ok, int *status)
    {
        auto take = [&](int i, const u8 *base) { for (long t = chunk_tile0[i]; t < chunk_tile0[i + 1]; t++) { tiles[t].base = base; ids.push_back((int)t); } };
        launch0.push_back(0);
        for (int i = 0; i < F.n_chunks; i++) {
            if (!F.resident[i]) continue;
            take(i, F.entry_of(i)->d);
            ok[i] = 1;
            status[i] = MTS_CHUNK_OK;
        }
        for (const FeedPiece &P : pieces) {
            launch0.push_back((long)ids.size());
            for (size_t z = 0; z < P.miss.size(); z++) take(P.miss[z], E.h_out.as<u8>() + P.ooff[z]);
        }
        launch0.push_back((long)ids.size());
    }

    // after piece p's decode: which of its chunks are good, for the kernel (tiles of the others are identities)
    int mark_decoded(int p, const int *status, std::vector<int> &ok, int *d_ok, hipStream_t st) const
    {
        for (int i : pieces[p].miss) ok[i] = status[i] == MTS_CHUNK_OK;
        hipError_t e = hipMemcpyAsync(d_ok, ok.data(), 4 * ok.size(), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) { set_error("hipMemcpyAsync: %s", hipGetErrorString(e)); return MTS_E_HIP; }
        return MTS_OK;
    }

    void add_counts(const std::vector<int> &ok, long *count) const
    {
        for (size_t t = 0; t < tiles.size(); t++) if (ok[tiles[t].chunk]) count[tile_win[t]] += tiles[t].n_rows;
    }
};

}  // namespace

// ---- per-window statistics (mts_window_stats, mts_dev_window_stats) ---------------------------------
// Tiles of STAT_TILE_ROWS rows (stats.hip), one partial per (tile, column); one combine launch at the end takes the tiles of
// window w, [win_tiles[w], win_tiles[w + 1]), in row order.
static int window_stats_run(Engine &E, hipStream_t st, DevCache *cache, const long *keys, const u8 *cdata, bool cdata_on_device,
                            const long *c_off, const long *c_len, const long *row0, const long *n_rows, int n_chunks, int nc, int sz,
                            int flags, long row_begin, long row_end, long window_rows, int n_cols, const int *cols, void *o_min,
                            void *o_max, void *o_sum, void *o_sq, bool out_on_host, long *count, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    int rc;
    if ((rc = check_items(sz, flags))) return rc;
    if (nc <= 0 || n_chunks < 0 || n_cols < 1 || !cols) { set_error("window stats: n_channels, n_chunks or columns invalid"); return MTS_E_ARG; }
    if (window_rows < 1) { set_error("window_rows %ld < 1", window_rows); return MTS_E_ARG; }
    if (row_begin < 0 || row_end < row_begin) { set_error("row range [%ld, %ld) invalid", row_begin, row_end); return MTS_E_ARG; }
    if ((rc = check_columns(cols, n_cols, nc))) return rc;
    const bool exact = !(flags & MTS_FLAG_FLOAT) && sz <= 2;
    const long span = row_end - row_begin;
    if (exact && (window_rows < span ? window_rows : span) > (1l << 31)) { set_error("windows of more than 2^31 rows on the exact path"); return MTS_E_ARG; }
    if ((rc = check_chunk_table(false, cache != nullptr, c_len, row0, n_rows, n_chunks, nc, sz, row_begin, row_end))) return rc;
    const long n_win = (span + window_rows - 1) / window_rows;
    if (n_win && (!o_min || !o_max || !o_sum || !o_sq || !count)) return MTS_E_ARG;
    for (long w = 0; w < n_win; w++) count[w] = 0;
    if (n_win == 0) return MTS_OK;                           // (no chunk can hold a row of an empty range: n_chunks is 0)

    ChunkFeed F(cache, keys, cdata, cdata_on_device, c_off, c_len, n_rows, n_chunks, nc, sz);
    if ((rc = F.classify())) return rc;
    TilePlan P(F, row0, row_begin, row_end, window_rows, STAT_TILE_ROWS);
    const long n_tiles = (long)P.tiles.size();
    std::vector<long> win_tiles(n_win + 1, 0);
    for (long t = 0; t < n_tiles; t++) win_tiles[P.tile_win[t] + 1]++;
    for (long w = 0; w < n_win; w++) win_tiles[w + 1] += win_tiles[w];

    // ---- workspace
    const u64 plane = (u64)n_tiles * n_cols * 8;
    const size_t o_tiles = 0, o_ids = align_up(sizeof(StatTile) * (n_tiles + 1), 256), o_ok = o_ids + align_up(4 * (u64)(n_tiles + 1), 256),
                 o_cols = o_ok + align_up(4 * (u64)(n_chunks + 1), 256), o_wt = o_cols + align_up(4 * (u64)n_cols, 256),
                 o_slab = o_wt + align_up(8 * (u64)(n_win + 1), 256), o_out = o_slab + align_up(4 * plane, 256);
    const u64 n_items = (u64)n_win * n_cols;
    const size_t o_omin = o_out, o_omax = o_omin + align_up(n_items * sz, 256), o_osum = o_omax + align_up(n_items * sz, 256),
                 o_osq = o_osum + align_up(n_items * 8, 256), o_end = out_on_host ? o_osq + align_up(n_items * 8, 256) : o_out;
    if ((rc = E.stats.ensure(o_end + 256))) return rc;
    if ((rc = F.ensure(E, P.piece_cap))) return rc;
    u8 *ws = E.stats.as<u8>();
    StatTile *d_tiles = (StatTile *)(ws + o_tiles);
    int *d_ids = (int *)(ws + o_ids), *d_ok = (int *)(ws + o_ok), *d_cols = (int *)(ws + o_cols);
    long *d_wt = (long *)(ws + o_wt);
    u8 *d_slab = ws + o_slab;
    std::vector<int> ok(n_chunks + 1, 0);
    P.place(F, E, ok, status);
    // (pageable sources: hipMemcpyAsync has staged them when it returns; the vectors live to the end of the call anyway)
    if (n_tiles) MTS_HIP(hipMemcpyAsync(d_tiles, P.tiles.data(), sizeof(StatTile) * n_tiles, hipMemcpyHostToDevice, st));
    if (n_tiles) MTS_HIP(hipMemcpyAsync(d_ids, P.ids.data(), 4 * (size_t)n_tiles, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_ok, ok.data(), 4 * (size_t)(n_chunks + 1), hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_wt, win_tiles.data(), 8 * (size_t)(n_win + 1), hipMemcpyHostToDevice, st));
    const int dflags = flags & ~MTS_FLAG_UNSIGNED;           // (the decoder compares the transform flags as a whole)
    const std::vector<long> &l0 = P.launch0;
    auto launch = [&](long first, long n) {
        return launch_stats_tiles(st, sz, flags, d_tiles, d_ids + first, (int)n, d_ok, d_cols, n_cols, nc, d_slab, n_tiles);
    };
    // resident chunks: reduced and waited for before any decode
    if (l0[1] > 0) {
        if ((rc = launch(0, l0[1]))) return rc;
        MTS_HIP(hipStreamSynchronize(st));
    }
    // ---- the other chunks, piece by piece
    rc = feed_pieces(F, E, st, P.pieces, dflags, status, [&](int p) {
        const int r = P.mark_decoded(p, status, ok, d_ok, st);
        return r ? r : launch(l0[1 + p], l0[2 + p] - l0[1 + p]);
    });
    if (rc) return rc;
    // ---- windows: the tiles in order
    void *c_min = out_on_host ? (void *)(ws + o_omin) : o_min, *c_max = out_on_host ? (void *)(ws + o_omax) : o_max;
    void *c_sum = out_on_host ? (void *)(ws + o_osum) : o_sum, *c_sq = out_on_host ? (void *)(ws + o_osq) : o_sq;
    if ((rc = launch_stats_combine(st, sz, flags, d_slab, n_tiles, d_wt, n_win, n_cols, c_min, c_max, c_sum, c_sq))) return rc;
    if (out_on_host) {                                        // the results, and nothing else, cross the bus
        MTS_HIP(hipMemcpyAsync(o_min, c_min, n_items * sz, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_max, c_max, n_items * sz, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_sum, c_sum, n_items * 8, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_sq, c_sq, n_items * 8, hipMemcpyDeviceToHost, st));
    }
    MTS_HIP(hipStreamSynchronize(st));
    P.add_counts(ok, count);
    return MTS_OK;
}

// ---- one round of a radix select (mts_rank_hist, mts_dev_rank_hist) ---------------------------------
// Tiles of SEL_TILE_ROWS rows and no combine launch: every tile adds its counts to the histograms of its window with integer
// atomics (select.hip), so the outputs are the same whatever the order of the launches.
static int rank_hist_run(Engine &E, hipStream_t st, DevCache *cache, const long *keys, const u8 *cdata, bool cdata_on_device,
                         const long *c_off, const long *c_len, const long *row0, const long *n_rows, int n_chunks, int nc, int sz, int flags,
                         long row_begin, long row_end, long window_rows, int n_cols, const int *cols, int mode, const double *center,
                         const unsigned long long *sel_prefix, const int *sel_shift, unsigned int *o_hist, unsigned long long *o_kmin,
                         unsigned long long *o_kmax, bool out_on_host, long *count, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    int rc;
    if ((rc = check_items(sz, flags))) return rc;
    if (nc <= 0 || n_chunks < 0 || n_cols < 1 || !cols) { set_error("rank hist: n_channels, n_chunks or columns invalid"); return MTS_E_ARG; }
    if (window_rows < 1) { set_error("window_rows %ld < 1", window_rows); return MTS_E_ARG; }
    if (row_begin < 0 || row_end < row_begin) { set_error("row range [%ld, %ld) invalid", row_begin, row_end); return MTS_E_ARG; }
    if (mode < 0 || mode > 2) { set_error("rank hist: mode %d (0, 1 or 2)", mode); return MTS_E_ARG; }
    if ((rc = check_columns(cols, n_cols, nc))) return rc;
    const long span = row_end - row_begin;
    if ((window_rows < span ? window_rows : span) >= (1l << 32)) { set_error("windows of 2^32 rows or more"); return MTS_E_ARG; }
    if ((rc = check_chunk_table(false, cache != nullptr, c_len, row0, n_rows, n_chunks, nc, sz, row_begin, row_end))) return rc;
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
    for (long w = 0; w < n_win; w++) count[w] = 0;
    if (n_win == 0) return MTS_OK;                           // (no chunk can hold a row of an empty range: n_chunks is 0)

    ChunkFeed F(cache, keys, cdata, cdata_on_device, c_off, c_len, n_rows, n_chunks, nc, sz);
    if ((rc = F.classify())) return rc;
    TilePlan P(F, row0, row_begin, row_end, window_rows, SEL_TILE_ROWS);
    const long n_tiles = (long)P.tiles.size();

    // ---- workspace
    const u64 n_cells = (u64)n_win * n_cols, hist_bytes = n_sel * (4ull << MTS_RANK_BITS), k_bytes = n_sel * 8;
    const size_t o_tiles = 0, o_tw = align_up(sizeof(StatTile) * (n_tiles + 1), 256), o_ids = o_tw + align_up(8 * (u64)(n_tiles + 1), 256),
                 o_ok = o_ids + align_up(4 * (u64)(n_tiles + 1), 256), o_cols = o_ok + align_up(4 * (u64)(n_chunks + 1), 256),
                 o_cen = o_cols + align_up(4 * (u64)n_cols, 256), o_pre = o_cen + align_up(mode ? 8 * n_cells : 0, 256),
                 o_shf = o_pre + align_up(k_bytes, 256), o_out = o_shf + align_up(n_sel * 4, 256);
    const size_t w_hist = o_out, w_kmin = w_hist + align_up(hist_bytes, 256), w_kmax = w_kmin + align_up(k_bytes, 256),
                 o_end = out_on_host ? w_kmax + align_up(k_bytes, 256) : o_out;
    if ((rc = E.stats.ensure(o_end + 256))) return rc;
    if ((rc = F.ensure(E, P.piece_cap))) return rc;
    u8 *ws = E.stats.as<u8>();
    StatTile *d_tiles = (StatTile *)(ws + o_tiles);
    long *d_tw = (long *)(ws + o_tw);
    int *d_ids = (int *)(ws + o_ids), *d_ok = (int *)(ws + o_ok), *d_cols = (int *)(ws + o_cols), *d_shf = (int *)(ws + o_shf);
    double *d_cen = (double *)(ws + o_cen);
    u64 *d_pre = (u64 *)(ws + o_pre);
    u32 *d_hist = out_on_host ? (u32 *)(ws + w_hist) : (u32 *)o_hist;
    u64 *d_kmin = out_on_host ? (u64 *)(ws + w_kmin) : (u64 *)o_kmin, *d_kmax = out_on_host ? (u64 *)(ws + w_kmax) : (u64 *)o_kmax;
    std::vector<int> ok(n_chunks + 1, 0);
    P.place(F, E, ok, status);
    if (n_tiles) MTS_HIP(hipMemcpyAsync(d_tiles, P.tiles.data(), sizeof(StatTile) * n_tiles, hipMemcpyHostToDevice, st));
    if (n_tiles) MTS_HIP(hipMemcpyAsync(d_tw, P.tile_win.data(), 8 * (size_t)n_tiles, hipMemcpyHostToDevice, st));
    if (n_tiles) MTS_HIP(hipMemcpyAsync(d_ids, P.ids.data(), 4 * (size_t)n_tiles, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_ok, ok.data(), 4 * (size_t)(n_chunks + 1), hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    if (mode) MTS_HIP(hipMemcpyAsync(d_cen, center, 8 * (size_t)n_cells, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_pre, sel_prefix, (size_t)k_bytes, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(d_shf, sel_shift, 4 * (size_t)n_sel, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemsetAsync(d_hist, 0, (size_t)hist_bytes, st));
    MTS_HIP(hipMemsetAsync(d_kmin, 0xff, (size_t)k_bytes, st));
    MTS_HIP(hipMemsetAsync(d_kmax, 0, (size_t)k_bytes, st));
    const int dflags = flags & ~MTS_FLAG_UNSIGNED;           // (the decoder compares the transform flags as a whole)
    const std::vector<long> &l0 = P.launch0;
    auto launch = [&](long first, long n) {
        return launch_rank_hist(st, sz, flags, mode, d_tiles, d_tw, d_ids + first, (int)n, d_ok, d_cols, n_cols, nc, d_cen, d_pre, d_shf, d_hist,
                                d_kmin, d_kmax);
    };
    // resident chunks: counted and waited for before any decode
    if (l0[1] > 0) {
        if ((rc = launch(0, l0[1]))) return rc;
        MTS_HIP(hipStreamSynchronize(st));
    }
    // ---- the other chunks, piece by piece
    rc = feed_pieces(F, E, st, P.pieces, dflags, status, [&](int p) {
        const int r = P.mark_decoded(p, status, ok, d_ok, st);
        return r ? r : launch(l0[1 + p], l0[2 + p] - l0[1 + p]);
    });
    if (rc) return rc;
    if (out_on_host) {                                        // the histograms, and nothing else, cross the bus
        MTS_HIP(hipMemcpyAsync(o_hist, d_hist, (size_t)hist_bytes, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_kmin, d_kmin, (size_t)k_bytes, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(o_kmax, d_kmax, (size_t)k_bytes, hipMemcpyDeviceToHost, st));
    }
    MTS_HIP(hipStreamSynchronize(st));
    P.add_counts(ok, count);
    return MTS_OK;
}

// ---- decimation (mts_decimate, mts_dev_decimate) ---------------------------------------------------------------------------
// Piece p owns the outputs whose newest row (first_row + k * q) lies in its chunks; their support reaches L - 1 rows further down,
// so a group reads its own chunks and those of the halo below.  Every output is computed once, from the same rows, in the same
// order: the result does not depend on the pieces.
static int decimate_run(Engine &E, hipStream_t st, DevCache *cache, const long *keys, const u8 *cdata, bool cdata_on_device, const long *c_off,
                        const long *c_len, const long *row0, const long *n_rows, int n_chunks, int nc, int sz, int flags, long vb, long ve,
                        long first_row, long n_out, int q, int n_taps, const double *taps, int osz, int n_cols, const int *cols, void *out,
                        bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    int rc;
    if ((rc = check_items(sz, flags))) return rc;
    if (nc <= 0 || n_chunks < 0 || n_cols < 1 || n_cols > 64 * 65535 || !cols) { set_error("decimate: n_channels, n_chunks or columns invalid"); return MTS_E_ARG; }
    if (q < 1) { set_error("decimate: q %d < 1", q); return MTS_E_ARG; }
    if (n_taps < 1 || n_taps > MTS_DECIMATE_MAX_TAPS || !taps) { set_error("decimate: %d taps (1 .. %d)", n_taps, MTS_DECIMATE_MAX_TAPS); return MTS_E_ARG; }
    for (int j = 0; j < n_taps; j++)
        if (!std::isfinite(taps[j])) { set_error("decimate: tap %d is not finite", j); return MTS_E_ARG; }
    if (osz != 4 && osz != 8) { set_error("decimate: output itemsize %d (4 or 8)", osz); return MTS_E_ARG; }
    if (vb < 0 || ve < vb || n_out < 0 || n_out > (1l << 40) || first_row < -(1l << 60) || first_row > (1l << 60)) {
        set_error("decimate: rows or outputs invalid"); return MTS_E_ARG;
    }
    if (n_out && !out) { set_error("decimate: no output buffer"); return MTS_E_ARG; }
    if ((rc = check_columns(cols, n_cols, nc))) return rc;
    if ((rc = check_chunk_table(true, cache != nullptr, c_len, row0, n_rows, n_chunks, nc, sz))) return rc;
    // the rows the outputs read: support ∩ valid range; the chunks must cover them
    const long need_lo = n_out ? std::max(vb, first_row - (n_taps - 1)) : 0, need_hi = n_out ? std::min(ve, first_row + (n_out - 1) * q + 1) : 0;
    if (need_lo < need_hi) {
        if (n_chunks == 0 || row0[0] > need_lo || row0[n_chunks - 1] + n_rows[n_chunks - 1] < need_hi) {
            set_error("decimate: the chunks do not cover rows [%ld, %ld)", need_lo, need_hi); return MTS_E_ARG;
        }
    }
    for (int i = 0; i < n_chunks; i++) status[i] = MTS_CHUNK_OK;
    if (n_out == 0) return MTS_OK;

    ChunkFeed F(cache, keys, cdata, cdata_on_device, c_off, c_len, n_rows, n_chunks, nc, sz);
    if ((rc = F.classify())) return rc;
    // ---- groups of outputs: [u0, u1) reads chunks [c0, c1]
    const std::vector<int> pb = F.piece_bounds();
    const int np = (int)pb.size() - 1;
    std::vector<long> gk;
    gk.push_back(0);
    for (int p = 1; p < np; p++) {
        const long r = row0[pb[p]] - first_row;                  // the first output whose newest row is in piece p
        long k = r <= 0 ? 0 : (r + q - 1) / q;
        if (k > n_out) k = n_out;
        gk.push_back(std::max(k, gk.back()));
    }
    gk.push_back(n_out);
    std::vector<FeedPiece> groups;
    for (int g = 0; g < np; g++) {
        if (gk[g + 1] <= gk[g]) continue;
        FeedPiece G;
        G.u0 = gk[g]; G.u1 = gk[g + 1];
        const long lo = std::max(vb, first_row + G.u0 * q - (n_taps - 1)), hi = std::min(ve, first_row + (G.u1 - 1) * q + 1);
        if (lo < hi && n_chunks) { G.c0 = chunk_of(row0, n_chunks, lo); G.c1 = chunk_of(row0, n_chunks, hi - 1); }
        // (else nothing valid to read, c1 < c0: every row is 0)
        groups.push_back(std::move(G));
    }
    u64 piece_cap;
    const std::vector<long> seg_at = plan_pieces(F, groups, &piece_cap);
    const u64 n_items = (u64)n_out * n_cols;
    const size_t o_taps = 0, o_cols = align_up(8 * (u64)n_taps, 256), o_seg = o_cols + align_up(4 * (u64)n_cols, 256),
                 o_out = o_seg + align_up(8 * (u64)(seg_at.back() + 1), 256), o_end = out_on_host ? o_out + align_up(n_items * osz, 256) : o_out;
    // ---- workspace
    if ((rc = E.dec.ensure(o_end + 256))) return rc;
    if ((rc = F.ensure(E, piece_cap))) return rc;
    u8 *ws = E.dec.as<u8>();
    std::vector<u8> h_taps(8 * (size_t)n_taps);
    for (int j = 0; j < n_taps; j++) {
        if (osz == 4) { const float f = (float)taps[j]; memcpy(h_taps.data() + 4 * j, &f, 4); }
        else memcpy(h_taps.data() + 8 * j, &taps[j], 8);
    }
    const std::vector<long> seg = segment_tables(F, E, groups, seg_at, row0);
    MTS_HIP(hipMemcpyAsync(ws + o_taps, h_taps.data(), (size_t)osz * n_taps, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_seg, seg.data(), 8 * seg.size(), hipMemcpyHostToDevice, st));
    void *d_out = out_on_host ? (void *)(ws + o_out) : out;
    const int dflags = flags & ~MTS_FLAG_UNSIGNED;           // (the decoder compares the transform flags as a whole)
    rc = feed_pieces(F, E, st, groups, dflags, status, [&](int g) {
        const FeedPiece &G = groups[g];
        const int r = F.still_placed(G);
        if (r) return r;
        const long *sb = (const long *)(ws + o_seg) + seg_at[g];
        const int ns = G.c1 - G.c0 + 1;
        return launch_decimate(st, sz, flags, osz, (const u8 *const *)sb, sb + (ns > 0 ? ns : 0), ns > 0 ? ns : 0, nc, (const int *)(ws + o_cols), n_cols,
                               ws + o_taps, n_taps, q, first_row, G.u0, G.u1, ns > 0 ? vb : 0, ns > 0 ? ve : 0,
                               (u8 *)d_out + (u64)G.u0 * n_cols * osz);
    });
    if (rc) return rc;
    if (out_on_host) MTS_HIP(hipMemcpyAsync(out, d_out, n_items * osz, hipMemcpyDeviceToHost, st));
    MTS_HIP(hipStreamSynchronize(st));
    return MTS_OK;
}

// ---- channel-mixing products (mts_project, mts_dev_project) --------------------------------------------------------------------
// The unit is a row and the halo is empty: piece p owns the rows of [row_begin, row_end) in its chunks and reads those chunks alone,
// so no chunk is decoded twice.  A row's outputs depend on that row only: the result does not depend on the pieces.
static int project_run(Engine &E, hipStream_t st, DevCache *cache, const long *keys, const u8 *cdata, bool cdata_on_device, const long *c_off,
                       const long *c_len, const long *row0, const long *n_rows, int n_chunks, int nc, int sz, int flags, long row_begin,
                       long row_end, int n_cols, const int *cols, const double *offset, int n_out, const double *weights, int osz, void *out,
                       bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    int rc;
    if ((rc = check_items(sz, flags))) return rc;
    if (nc <= 0 || n_chunks < 0) { set_error("project: n_channels or n_chunks invalid"); return MTS_E_ARG; }
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
    if ((rc = check_chunk_table(true, cache != nullptr, c_len, row0, n_rows, n_chunks, nc, sz))) return rc;
    if (row_begin < row_end && (n_chunks == 0 || row0[0] > row_begin || row0[n_chunks - 1] + n_rows[n_chunks - 1] < row_end)) {
        set_error("project: the chunks do not cover rows [%ld, %ld)", row_begin, row_end); return MTS_E_ARG;
    }
    for (int i = 0; i < n_chunks; i++) status[i] = MTS_CHUNK_OK;
    if (row_begin == row_end) return MTS_OK;

    ChunkFeed F(cache, keys, cdata, cdata_on_device, c_off, c_len, n_rows, n_chunks, nc, sz);
    if ((rc = F.classify())) return rc;
    // ---- pieces: rows [u0, u1) of the range in chunks [c0, c1]
    const std::vector<int> pb = F.piece_bounds();
    std::vector<FeedPiece> pieces;
    for (size_t p = 0; p + 1 < pb.size(); p++) {
        if (pb[p + 1] <= pb[p]) continue;
        FeedPiece P;
        P.u0 = std::max(row_begin, row0[pb[p]]);
        P.u1 = std::min(row_end, row0[pb[p + 1] - 1] + n_rows[pb[p + 1] - 1]);
        if (P.u1 <= P.u0) continue;                               // (chunks outside the range are not read)
        P.c0 = chunk_of(row0, n_chunks, P.u0); P.c1 = chunk_of(row0, n_chunks, P.u1 - 1);
        pieces.push_back(std::move(P));
    }
    u64 piece_cap;
    const std::vector<long> seg_at = plan_pieces(F, pieces, &piece_cap);
    // ---- workspace: weights (padded with zeros to multiples of PROJECT_PAD rows and columns), offsets, columns, segment tables, output
    const int kp = (int)align_up((u64)n_cols, PROJECT_PAD), wp = (int)align_up((u64)n_out, PROJECT_PAD);
    const u64 n_items = (u64)(row_end - row_begin) * n_out;
    const size_t o_w = 0, o_off = align_up((u64)osz * kp * wp, 256), o_cols = o_off + align_up((u64)osz * n_cols, 256),
                 o_seg = o_cols + align_up(4 * (u64)n_cols, 256), o_out = o_seg + align_up(8 * (u64)(seg_at.back() + 1), 256),
                 o_end = out_on_host ? o_out + align_up(n_items * osz, 256) : o_out;
    if ((rc = E.proj.ensure(o_end + 256))) return rc;
    if ((rc = F.ensure(E, piece_cap))) return rc;
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
    const std::vector<long> seg = segment_tables(F, E, pieces, seg_at, row0);
    MTS_HIP(hipMemcpyAsync(ws + o_w, h_w.data(), (size_t)osz * kp * wp, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_off, h_off, (size_t)osz * n_cols, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_seg, seg.data(), 8 * seg.size(), hipMemcpyHostToDevice, st));
    void *d_out = out_on_host ? (void *)(ws + o_out) : out;
    const int dflags = flags & ~MTS_FLAG_UNSIGNED;           // (the decoder compares the transform flags as a whole)
    rc = feed_pieces(F, E, st, pieces, dflags, status, [&](int p) {
        const FeedPiece &P = pieces[p];
        const int r = F.still_placed(P);
        if (r) return r;
        const long *sb = (const long *)(ws + o_seg) + seg_at[p];
        const int ns = P.c1 - P.c0 + 1;
        return launch_project(st, sz, flags, osz, (const u8 *const *)sb, sb + ns, ns, nc, (const int *)(ws + o_cols), ws + o_off, n_cols, ws + o_w, wp,
                              n_out, P.u0, P.u1, (u8 *)d_out + (u64)(P.u0 - row_begin) * n_out * osz);
    });
    if (rc) { (void)hipStreamSynchronize(st); return rc; }   // (h_w has been read before it goes)
    if (out_on_host) MTS_HIP(hipMemcpyAsync(out, d_out, n_items * osz, hipMemcpyDeviceToHost, st));
    MTS_HIP(hipStreamSynchronize(st));
    return MTS_OK;
}

// ---- peak detection (mts_detect, mts_dev_detect) -------------------------------------------------------------------------------
// The unit is a row.  Piece p owns the rows of [row_begin, row_end) in its chunks; their events need the detection value R rows either
// side, and that the filter's support: piece p reads the chunks from the one holding u0 - R + half - (L - 1) to the one holding
// u1 - 1 + R + half, within the valid range.  A piece's rows go through the float32 workspace in slabs that keep it <= the slab bound
// (filter -> median -> mask -> count / scan / emit on the stream); the write position is carried on the device from slab to slab and
// piece to piece.  Every value is computed from the same rows in the same order whatever the pieces and slabs.
static const u64 DETECT_SLAB_BYTES = 256ull << 20;
static const long DETECT_SLAB_MAX_ROWS = 1l << 22;                  // (bounds the bitmap of narrow selections: <= 32 MiB up to 64 columns)

static u64 detect_slab_bytes()
{
    const char *e = getenv("MTS_DETECT_SLAB_BYTES");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (u64)v : DETECT_SLAB_BYTES;
}

static int detect_run(Engine &E, hipStream_t st, DevCache *cache, const long *keys, const u8 *cdata, bool cdata_on_device, const long *c_off,
                      const long *c_len, const long *row0, const long *n_rows, int n_chunks, int nc, int sz, int flags, long vb, long ve,
                      long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols, const float *threshold, int sign,
                      int reference, int R, int S, long max_events, long *out_row, int *out_pos, float *out_amp, bool out_on_host,
                      long *n_events, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    int rc;
    if ((rc = check_items(sz, flags))) return rc;
    if (nc <= 0 || n_chunks < 0 || n_cols < 1 || n_cols > 64 * 65535 || !cols) { set_error("detect: n_channels, n_chunks or columns invalid"); return MTS_E_ARG; }
    if (n_taps < 1 || n_taps > MTS_DECIMATE_MAX_TAPS || !taps) { set_error("detect: %d taps (1 .. %d)", n_taps, MTS_DECIMATE_MAX_TAPS); return MTS_E_ARG; }
    for (int j = 0; j < n_taps; j++)
        if (!std::isfinite(taps[j])) { set_error("detect: tap %d is not finite", j); return MTS_E_ARG; }
    if (!threshold) { set_error("detect: no thresholds"); return MTS_E_ARG; }
    for (int j = 0; j < n_cols; j++)
        if (!std::isfinite(threshold[j]) || !(threshold[j] > 0)) { set_error("detect: threshold %d is not a finite positive number", j); return MTS_E_ARG; }
    if (sign < 0 || sign > 2) { set_error("detect: sign %d (0 neg, 1 pos, 2 both)", sign); return MTS_E_ARG; }
    if (reference < 0 || reference > 1) { set_error("detect: reference %d (0 none, 1 median)", reference); return MTS_E_ARG; }
    if (reference && n_cols > MTS_DETECT_MAX_REF_COLS) { set_error("detect: a median reference over %d columns (<= %d)", n_cols, MTS_DETECT_MAX_REF_COLS); return MTS_E_ARG; }
    if (R < 0 || R > MTS_DETECT_MAX_EXCLUDE || S < 0 || S > MTS_DETECT_MAX_SPREAD) {
        set_error("detect: exclude_rows %d (0 .. %d) or exclude_cols %d (0 .. %d)", R, MTS_DETECT_MAX_EXCLUDE, S, MTS_DETECT_MAX_SPREAD); return MTS_E_ARG;
    }
    if (vb < 0 || ve < vb || ve > (1l << 60) || row_begin < vb || row_end < row_begin || row_end > ve) { set_error("detect: rows invalid"); return MTS_E_ARG; }
    if (max_events < 0 || max_events > (1l << 40) || !n_events) { set_error("detect: max_events invalid or no n_events"); return MTS_E_ARG; }
    if (max_events && (!out_row || !out_pos || !out_amp)) { set_error("detect: no output buffers"); return MTS_E_ARG; }
    if ((rc = check_columns(cols, n_cols, nc))) return rc;
    if ((rc = check_chunk_table(true, cache != nullptr, c_len, row0, n_rows, n_chunks, nc, sz))) return rc;
    const long half = (n_taps - 1) / 2;
    const bool any = row_end > row_begin;
    // the rows the events read: (rows + R either side)'s support ∩ valid range; the chunks must cover them
    const long need_lo = any ? std::max(vb, row_begin - R + half - (n_taps - 1)) : 0, need_hi = any ? std::min(ve, row_end + R + half) : 0;
    if (need_lo < need_hi) {
        if (n_chunks == 0 || row0[0] > need_lo || row0[n_chunks - 1] + n_rows[n_chunks - 1] < need_hi) {
            set_error("detect: the chunks do not cover rows [%ld, %ld)", need_lo, need_hi); return MTS_E_ARG;
        }
    }
    for (int i = 0; i < n_chunks; i++) status[i] = MTS_CHUNK_OK;
    *n_events = 0;
    if (!any) return MTS_OK;

    ChunkFeed F(cache, keys, cdata, cdata_on_device, c_off, c_len, n_rows, n_chunks, nc, sz);
    if ((rc = F.classify())) return rc;
    // ---- pieces of rows: [u0, u1) reads chunks [c0, c1]
    const std::vector<int> pb = F.piece_bounds();
    const int np = (int)pb.size() - 1;
    std::vector<long> gr;
    gr.push_back(row_begin);
    for (int p = 1; p < np; p++) gr.push_back(std::max(gr.back(), std::min(row_end, row0[pb[p]])));
    gr.push_back(row_end);
    std::vector<FeedPiece> pieces;
    for (int p = 0; p < np; p++) {
        if (gr[p + 1] <= gr[p]) continue;
        FeedPiece Pc;
        Pc.u0 = gr[p]; Pc.u1 = gr[p + 1];
        const long lo = std::max(vb, Pc.u0 - R + half - (n_taps - 1)), hi = std::min(ve, Pc.u1 + R + half);
        if (lo < hi && n_chunks) { Pc.c0 = chunk_of(row0, n_chunks, lo); Pc.c1 = chunk_of(row0, n_chunks, hi - 1); }
        pieces.push_back(std::move(Pc));
    }
    u64 piece_cap;
    const std::vector<long> seg_at = plan_pieces(F, pieces, &piece_cap);
    // rows a slab owns: the workspace holds them and R rows either side
    const long cap_rows = (long)std::min<u64>(detect_slab_bytes() / (4 * (u64)n_cols), (u64)DETECT_SLAB_MAX_ROWS);
    const long own = std::min(row_end - row_begin, std::max(1l, cap_rows - 2l * R));
    const long max_words = detect_bitmap_words(own, n_cols), max_blocks = detect_blocks(max_words);
    const size_t o_taps = 0, o_cols = align_up(4 * (u64)n_taps, 256), o_thr = o_cols + align_up(4 * (u64)n_cols, 256),
                 o_seg = o_thr + align_up(4 * (u64)n_cols, 256), o_total = o_seg + align_up(8 * (u64)(seg_at.back() + 1), 256),
                 o_y = o_total + 256, o_bits = o_y + align_up(4 * (u64)(own + 2l * R) * n_cols, 256), o_cnt = o_bits + align_up(8 * (u64)max_words, 256),
                 o_offs = o_cnt + align_up(4 * (u64)max_blocks, 256), o_row = o_offs + align_up(8 * (u64)max_blocks, 256),
                 o_pos = out_on_host ? o_row + align_up(8 * (u64)max_events, 256) : o_row,
                 o_amp = out_on_host ? o_pos + align_up(4 * (u64)max_events, 256) : o_row,
                 o_end = out_on_host ? o_amp + align_up(4 * (u64)max_events, 256) : o_row;
    // ---- workspace
    if ((rc = E.det.ensure(o_end + 256))) return rc;
    if ((rc = F.ensure(E, piece_cap))) return rc;
    u8 *ws = E.det.as<u8>();
    std::vector<float> h_taps(n_taps);
    for (int j = 0; j < n_taps; j++) h_taps[j] = (float)taps[j];
    const std::vector<long> seg = segment_tables(F, E, pieces, seg_at, row0);
    MTS_HIP(hipMemcpyAsync(ws + o_taps, h_taps.data(), 4 * (size_t)n_taps, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_thr, threshold, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_seg, seg.data(), 8 * seg.size(), hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemsetAsync(ws + o_total, 0, 8, st));
    long *d_row = out_on_host ? (long *)(ws + o_row) : out_row;
    int *d_pos = out_on_host ? (int *)(ws + o_pos) : out_pos;
    float *d_amp = out_on_host ? (float *)(ws + o_amp) : out_amp;
    float *d_y = (float *)(ws + o_y);
    u64 *d_bits = (u64 *)(ws + o_bits), *d_total = (u64 *)(ws + o_total);
    const int dflags = flags & ~MTS_FLAG_UNSIGNED;           // (the decoder compares the transform flags as a whole)
    rc = feed_pieces(F, E, st, pieces, dflags, status, [&](int p) {
        const FeedPiece &Pc = pieces[p];
        int r = F.still_placed(Pc);
        const long *sb = (const long *)(ws + o_seg) + seg_at[p];
        const int ns = Pc.c1 - Pc.c0 + 1 > 0 ? Pc.c1 - Pc.c0 + 1 : 0;
        for (long s0 = Pc.u0; !r && s0 < Pc.u1; s0 += own) {
            const long s1 = std::min(Pc.u1, s0 + own), a = std::max(vb, s0 - R), b = std::min(ve, s1 + R);
            // y[t] for t in [a, b): output k = t of a decimation by 1 whose newest row is half + k
            r = launch_decimate(st, sz, flags, 4, (const u8 *const *)sb, sb + ns, ns, nc, (const int *)(ws + o_cols), n_cols, ws + o_taps, n_taps, 1,
                                half, a, b, ns ? vb : 0, ns ? ve : 0, d_y);
            if (!r && reference) r = launch_row_median(st, d_y, b - a, n_cols);
            if (!r) r = launch_detect_mask(st, d_y, a, b - a, n_cols, (const float *)(ws + o_thr), sign, R, S, s0, s1, d_bits);
            if (!r) r = launch_detect_emit(st, d_bits, detect_bitmap_words(s1 - s0, n_cols), (u32 *)(ws + o_cnt), (u64 *)(ws + o_offs), d_total, d_y,
                                           a, n_cols, s0, max_events, d_row, d_pos, d_amp);
        }
        return r;
    });
    if (rc) return rc;
    u64 total = 0;
    MTS_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    MTS_HIP(hipStreamSynchronize(st));
    *n_events = (long)total;
    const size_t n_w = (size_t)std::min<u64>(total, (u64)max_events);
    if (out_on_host && n_w) {
        MTS_HIP(hipMemcpyAsync(out_row, d_row, 8 * n_w, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_pos, d_pos, 4 * n_w, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipMemcpyAsync(out_amp, d_amp, 4 * n_w, hipMemcpyDeviceToHost, st));
        MTS_HIP(hipStreamSynchronize(st));
    }
    return MTS_OK;
}

// ---- Welch PSD (mts_welch, mts_dev_welch) ------------------------------------------------------------------------------------
// The call's segments are cut into blocks of B (WELCH_BLOCK_SEGMENTS) and groups of G.  Piece p owns the blocks whose first row lies
// in its chunks.  A piece's blocks are launched in runs that keep the partial slab <= WELCH_SLAB_BYTES, each followed by the combine
// that adds them to their groups' sums in block order: every group sum is the same sequence of additions whatever the pieces and runs.
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

static int welch_run(Engine &E, hipStream_t st, DevCache *cache, const long *keys, const u8 *cdata, bool cdata_on_device, const long *c_off,
                     const long *c_len, const long *row0, const long *n_rows, int n_chunks, int nc, int sz, int flags, long row_seg0, long seg_begin,
                     long seg_end, int nperseg, long step, const double *taper, int detrend, int csize, int n_cols, const int *cols, double *out,
                     bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    int rc;
    if ((rc = check_items(sz, flags))) return rc;
    if (nc <= 0 || n_chunks < 0 || n_cols < 1 || n_cols > (1 << 24) || !cols) { set_error("welch: n_channels, n_chunks or columns invalid"); return MTS_E_ARG; }
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
    if ((rc = check_chunk_table(true, cache != nullptr, c_len, row0, n_rows, n_chunks, nc, sz))) return rc;
    // the rows the segments read; the chunks must cover them
    const long need_lo = row_seg0 + seg_begin * step, need_hi = row_seg0 + (seg_end - 1) * step + nperseg;
    if (n_chunks == 0 || row0[0] > need_lo || row0[n_chunks - 1] + n_rows[n_chunks - 1] < need_hi) {
        set_error("welch: the chunks do not cover rows [%ld, %ld)", need_lo, need_hi); return MTS_E_ARG;
    }
    for (int i = 0; i < n_chunks; i++) status[i] = MTS_CHUNK_OK;
    int log2n = 0;
    while ((1 << log2n) < nperseg) log2n++;
    const long n_seg = seg_end - seg_begin, n_blocks = (n_seg + B - 1) / B, GB = G / B, n_groups = (n_seg + G - 1) / G;
    const long b_first = seg_begin / B;                              // the call's block 0 (absolute)
    const long n_elems = (long)(nperseg / 2 + 1) * n_cols;

    ChunkFeed F(cache, keys, cdata, cdata_on_device, c_off, c_len, n_rows, n_chunks, nc, sz);
    if ((rc = F.classify())) return rc;
    // ---- pieces of blocks: [u0, u1) (call-local block indices) read chunks [c0, c1]
    const std::vector<int> pb = F.piece_bounds();
    const int np = (int)pb.size() - 1;
    const long block_rows = step * B, row_b0 = row_seg0 + seg_begin * step; // first row of call block 0
    std::vector<long> gb;
    gb.push_back(0);
    for (int p = 1; p < np; p++) {
        const long r = row0[pb[p]] - row_b0;                        // the first block whose first row is in piece p
        long k = r <= 0 ? 0 : (r + block_rows - 1) / block_rows;
        if (k > n_blocks) k = n_blocks;
        gb.push_back(std::max(k, gb.back()));
    }
    gb.push_back(n_blocks);
    std::vector<FeedPiece> pieces;
    for (int p = 0; p < np; p++) {
        if (gb[p + 1] <= gb[p]) continue;
        FeedPiece Pc;
        Pc.u0 = gb[p]; Pc.u1 = gb[p + 1];
        const long s_lo = seg_begin + Pc.u0 * B, s_hi = std::min(seg_end, seg_begin + Pc.u1 * B);
        Pc.c0 = chunk_of(row0, n_chunks, row_seg0 + s_lo * step);
        Pc.c1 = chunk_of(row0, n_chunks, row_seg0 + (s_hi - 1) * step + nperseg - 1);
        pieces.push_back(std::move(Pc));
    }
    u64 piece_cap;
    const std::vector<long> seg_at = plan_pieces(F, pieces, &piece_cap);
    // blocks per launch: the slab of partials stays <= WELCH_SLAB_BYTES (at least one block)
    const u64 blk_bytes = 8 * (u64)n_elems;
    long run_blocks = (long)std::max<u64>(1, WELCH_SLAB_BYTES / blk_bytes);
    run_blocks = std::min(run_blocks, std::min(n_blocks, 65535l));
    const size_t o_taper = 0, o_tw = align_up((u64)csize * nperseg, 256), o_cols = o_tw + align_up(2 * (u64)csize * nperseg, 256),
                 o_seg = o_cols + align_up(4 * (u64)n_cols, 256), o_part = o_seg + align_up(8 * (u64)(seg_at.back() + 1), 256),
                 o_acc = o_part + align_up(blk_bytes * run_blocks, 256),
                 o_end = out_on_host ? o_acc + align_up(8 * (u64)n_groups * n_elems, 256) : o_acc;
    // ---- workspace
    if ((rc = E.welch.ensure(o_end + 256))) return rc;
    if ((rc = F.ensure(E, piece_cap))) return rc;
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
    const std::vector<long> seg = segment_tables(F, E, pieces, seg_at, row0);
    MTS_HIP(hipMemcpyAsync(ws + o_taper, h_tt.data(), (size_t)csize * nperseg, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_tw, h_tt.data() + (size_t)csize * nperseg, 2 * (size_t)csize * nperseg, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_seg, seg.data(), 8 * seg.size(), hipMemcpyHostToDevice, st));
    double *d_acc = out_on_host ? (double *)(ws + o_acc) : out;
    MTS_HIP(hipMemsetAsync(d_acc, 0, 8 * (size_t)n_groups * n_elems, st));
    double *d_part = (double *)(ws + o_part);
    const int dflags = flags & ~MTS_FLAG_UNSIGNED;
    rc = feed_pieces(F, E, st, pieces, dflags, status, [&](int p) {
        const FeedPiece &Pc = pieces[p];
        int r = F.still_placed(Pc);
        const long *sb = (const long *)(ws + o_seg) + seg_at[p];
        const int ns = Pc.c1 - Pc.c0 + 1;
        for (long lb = Pc.u0; !r && lb < Pc.u1; lb += run_blocks) {
            const long lb1 = std::min(Pc.u1, lb + run_blocks);
            r = launch_welch(st, sz, flags, csize, log2n, (const u8 *const *)sb, sb + ns, ns, nc, (const int *)(ws + o_cols), n_cols, ws + o_taper,
                             ws + o_tw, row_seg0, step, seg_end, b_first + lb, lb1 - lb, detrend ? 1 : 0, d_part);
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
// The call's groups are cut into slabs of GRAM_SLAB_ROWS rows.  Piece p owns the groups whose first row lies in its chunks.  A piece's
// slabs are launched in runs that keep the partial slab <= GRAM_SLAB_BYTES, each followed by the combine that adds them to their
// groups' accumulators in slab order: every group sum is the same sequence of additions whatever the pieces and runs.
static const u64 GRAM_SLAB_BYTES = 256ull << 20;

static int gram_run(Engine &E, hipStream_t st, DevCache *cache, const long *keys, const u8 *cdata, bool cdata_on_device, const long *c_off,
                    const long *c_len, const long *row0, const long *n_rows, int n_chunks, int nc, int sz, int flags, long range_begin,
                    long range_end, long window_rows, long group_begin, long group_end, int n_cols, const int *cols, void *out_gram, void *out_sum,
                    bool out_on_host, int *status)
{
    // ---- arguments: everything is checked before anything is allocated or launched
    int rc;
    if ((rc = check_items(sz, flags))) return rc;
    if (nc <= 0 || n_chunks < 0 || n_cols < 1 || n_cols > MTS_GRAM_MAX_COLS || !cols) {
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
    if ((rc = check_chunk_table(true, cache != nullptr, c_len, row0, n_rows, n_chunks, nc, sz))) return rc;
    // the groups' rows: group g -> [grow[g], grow_end(g))
    const long n_groups = group_end - group_begin;
    if (n_groups > (1l << 31)) { set_error("gram: too many groups in one call"); return MTS_E_ARG; }
    auto group_rows = [&](long g, long *lo, long *hi) {
        const long w = g / K, k = g % K, w0 = range_begin + w * window_rows;
        const long w1 = std::min(w0 + window_rows, range_end);
        *lo = w0 + k * GR;
        *hi = std::min(*lo + GR, w1);
    };
    long need_lo, need_hi, tmp;
    group_rows(group_begin, &need_lo, &tmp);
    group_rows(group_end - 1, &tmp, &need_hi);
    if (n_chunks == 0 || row0[0] > need_lo || row0[n_chunks - 1] + n_rows[n_chunks - 1] < need_hi) {
        set_error("gram: the chunks do not cover rows [%ld, %ld)", need_lo, need_hi); return MTS_E_ARG;
    }
    for (int i = 0; i < n_chunks; i++) status[i] = MTS_CHUNK_OK;
    // slabs of the call: slab_rows (2 per slab), gfirst[g] the first slab of call group g
    std::vector<long> gfirst(n_groups + 1, 0), glo(n_groups);
    long n_slabs = 0;
    for (long g = 0; g < n_groups; g++) {
        long lo, hi;
        group_rows(group_begin + g, &lo, &hi);
        glo[g] = lo;
        gfirst[g] = n_slabs;
        n_slabs += (hi - lo + SR - 1) / SR;
    }
    gfirst[n_groups] = n_slabs;
    std::vector<long> slab_rows(2 * (size_t)n_slabs);
    for (long g = 0; g < n_groups; g++) {
        long lo, hi;
        group_rows(group_begin + g, &lo, &hi);
        for (long s = gfirst[g], r = lo; s < gfirst[g + 1]; s++, r += SR) { slab_rows[2 * s] = r; slab_rows[2 * s + 1] = std::min(r + SR, hi); }
    }

    ChunkFeed F(cache, keys, cdata, cdata_on_device, c_off, c_len, n_rows, n_chunks, nc, sz);
    if ((rc = F.classify())) return rc;
    // ---- pieces of groups: [u0, u1) (call-local group indices) read chunks [c0, c1]
    const std::vector<int> pb = F.piece_bounds();
    const int np = (int)pb.size() - 1;
    std::vector<long> gp;
    gp.push_back(0);
    for (int p = 1; p < np; p++) {
        const long r = row0[pb[p]];                                     // the first group whose first row is in piece p
        const long k = std::lower_bound(glo.begin(), glo.end(), r) - glo.begin();
        gp.push_back(std::max(k, gp.back()));
    }
    gp.push_back(n_groups);
    std::vector<FeedPiece> pieces;
    for (int p = 0; p < np; p++) {
        if (gp[p + 1] <= gp[p]) continue;
        FeedPiece Pc;
        Pc.u0 = gp[p]; Pc.u1 = gp[p + 1];
        Pc.c0 = chunk_of(row0, n_chunks, slab_rows[2 * gfirst[Pc.u0]]);
        Pc.c1 = chunk_of(row0, n_chunks, slab_rows[2 * gfirst[Pc.u1] - 1] - 1);
        pieces.push_back(std::move(Pc));
    }
    u64 piece_cap;
    const std::vector<long> seg_at = plan_pieces(F, pieces, &piece_cap);
    // slabs per launch: the partials stay <= GRAM_SLAB_BYTES (at least one slab)
    const u64 slab_bytes = (u64)gram_slab_bytes(n_cols);
    long run_slabs = (long)std::max<u64>(1, GRAM_SLAB_BYTES / slab_bytes);
    run_slabs = std::min(run_slabs, std::min(n_slabs, 65535l));
    const u64 nn = (u64)n_cols * n_cols;
    const size_t o_cols = 0, o_slab = align_up(4 * (u64)n_cols, 256), o_gf = o_slab + align_up(16 * (u64)n_slabs, 256),
                 o_seg = o_gf + align_up(8 * (u64)(n_groups + 1), 256), o_part = o_seg + align_up(8 * (u64)(seg_at.back() + 1), 256),
                 o_psum = o_part + align_up((u64)run_slabs * gram_pairs(n_cols) * 64 * 64 * 8, 256),
                 o_acc = o_psum + align_up((u64)run_slabs * 8 * n_cols, 256),
                 o_accs = o_acc + (out_on_host ? align_up(8 * (u64)n_groups * nn, 256) : 0),
                 o_end = o_accs + (out_on_host ? align_up(8 * (u64)n_groups * n_cols, 256) : 0);
    // ---- workspace
    if ((rc = E.gram.ensure(o_end + 256))) return rc;
    if ((rc = F.ensure(E, piece_cap))) return rc;
    u8 *ws = E.gram.as<u8>();
    const std::vector<long> seg = segment_tables(F, E, pieces, seg_at, row0);
    MTS_HIP(hipMemcpyAsync(ws + o_cols, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_slab, slab_rows.data(), 16 * (size_t)n_slabs, hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_gf, gfirst.data(), 8 * (size_t)(n_groups + 1), hipMemcpyHostToDevice, st));
    MTS_HIP(hipMemcpyAsync(ws + o_seg, seg.data(), 8 * seg.size(), hipMemcpyHostToDevice, st));
    double *d_gram = out_on_host ? (double *)(ws + o_acc) : (double *)out_gram;
    u64 *d_sum = out_on_host ? (u64 *)(ws + o_accs) : (u64 *)out_sum;
    MTS_HIP(hipMemsetAsync(d_gram, 0, 8 * (size_t)n_groups * nn, st));
    MTS_HIP(hipMemsetAsync(d_sum, 0, 8 * (size_t)n_groups * n_cols, st));
    double *d_part = (double *)(ws + o_part);
    u64 *d_psum = (u64 *)(ws + o_psum);
    const long *d_slab = (const long *)(ws + o_slab), *d_gf = (const long *)(ws + o_gf);
    const bool exact = !(flags & MTS_FLAG_FLOAT) && sz <= 2;
    const int float_sum = (flags & MTS_FLAG_FLOAT) ? 1 : 0;
    const int dflags = flags & ~MTS_FLAG_UNSIGNED;
    rc = feed_pieces(F, E, st, pieces, dflags, status, [&](int p) {
        const FeedPiece &Pc = pieces[p];
        int r = F.still_placed(Pc);
        const long *sb = (const long *)(ws + o_seg) + seg_at[p];
        const int ns = Pc.c1 - Pc.c0 + 1;
        const long p_s0 = gfirst[Pc.u0], p_s1 = gfirst[Pc.u1];
        for (long s = p_s0; !r && s < p_s1; s += run_slabs) {
            const long s1 = std::min(p_s1, s + run_slabs);
            r = launch_gram(st, sz, flags, (const u8 *const *)sb, sb + ns, ns, nc, (const int *)(ws + o_cols), n_cols, d_slab, s, s1 - s, d_part, d_psum);
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

// ---- the entries of the reductions: the cache (host entries), the engine and its lock, the device, then run(engine, cache).
// bad_table: the wrapper's own null-pointer check, which answers after a cache that does not exist and before everything else
template <class Run>
static int host_entry(int device, long cache_id, bool bad_table, Run &&run)
{
    DevCache *c = nullptr;
    if (cache_id) {
        int cdev = 0;
        c = find_cache(cache_id, &cdev);
        if (!c || cdev != device) { set_error("cache %ld does not exist on device %d", cache_id, device); return MTS_E_ARG; }
    }
    if (bad_table) return MTS_E_ARG;
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(E->mu);
    if (c && !cache_alive(cache_id, c)) return MTS_E_ARG;      // (destroyed while this call waited for the engine)
    MTS_HIP(hipSetDevice(E->dev));
    return run(*E, c);
}

template <class Run>
static int dev_entry(int device, bool bad_table, Run &&run)
{
    if (bad_table) return MTS_E_ARG;
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(E->mu);
    MTS_HIP(hipSetDevice(E->dev));
    return run(*E);
}

extern "C" {

int mts_window_stats(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                     const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_begin,
                     long row_end, long window_rows, int n_cols, const int *cols, void *out_min, void *out_max, void *out_sum, void *out_sumsq,
                     long *out_count, int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status || (cache_id && !chunk_keys));
    return host_entry(device, cache_id, bad, [&](Engine &E, DevCache *c) {
        return window_stats_run(E, nullptr, c, chunk_keys, cdata, false, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels, itemsize,
                                flags, row_begin, row_end, window_rows, n_cols, cols, out_min, out_max, out_sum, out_sumsq, true, out_count,
                                chunk_status);
    });
}

int mts_dev_window_stats(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                         const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_begin,
                         long row_end, long window_rows, int n_cols, const int *cols, void *d_min, void *d_max, void *d_sum, void *d_sumsq,
                         long *count, int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!d_cdata || !chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status);
    return dev_entry(device, bad, [&](Engine &E) {
        return window_stats_run(E, (hipStream_t)stream, nullptr, nullptr, d_cdata, true, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks,
                                n_channels, itemsize, flags, row_begin, row_end, window_rows, n_cols, cols, d_min, d_max, d_sum, d_sumsq, false,
                                count, chunk_status);
    });
}

int mts_rank_hist(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                  const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_begin,
                  long row_end, long window_rows, int n_cols, const int *cols, int mode, const double *center,
                  const unsigned long long *sel_prefix, const int *sel_shift, unsigned int *out_hist, unsigned long long *out_kmin,
                  unsigned long long *out_kmax, long *out_count, int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status || (cache_id && !chunk_keys));
    return host_entry(device, cache_id, bad, [&](Engine &E, DevCache *c) {
        return rank_hist_run(E, nullptr, c, chunk_keys, cdata, false, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels, itemsize,
                             flags, row_begin, row_end, window_rows, n_cols, cols, mode, center, sel_prefix, sel_shift, out_hist, out_kmin,
                             out_kmax, true, out_count, chunk_status);
    });
}

int mts_dev_rank_hist(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                      const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_begin,
                      long row_end, long window_rows, int n_cols, const int *cols, int mode, const double *center,
                      const unsigned long long *sel_prefix, const int *sel_shift, unsigned int *d_hist, unsigned long long *d_kmin,
                      unsigned long long *d_kmax, long *count, int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!d_cdata || !chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status);
    return dev_entry(device, bad, [&](Engine &E) {
        return rank_hist_run(E, (hipStream_t)stream, nullptr, nullptr, d_cdata, true, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks,
                             n_channels, itemsize, flags, row_begin, row_end, window_rows, n_cols, cols, mode, center, sel_prefix, sel_shift,
                             d_hist, d_kmin, d_kmax, false, count, chunk_status);
    });
}

int mts_decimate(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                 const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                 long valid_end, long first_row, long n_out, int q, int n_taps, const double *taps, int out_itemsize, int n_cols, const int *cols,
                 void *out, int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status || (cache_id && !chunk_keys));
    return host_entry(device, cache_id, bad, [&](Engine &E, DevCache *c) {
        return decimate_run(E, nullptr, c, chunk_keys, cdata, false, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels, itemsize,
                            flags, valid_begin, valid_end, first_row, n_out, q, n_taps, taps, out_itemsize, n_cols, cols, out, true, chunk_status);
    });
}

int mts_dev_decimate(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths, const long *chunk_row0,
                     const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin, long valid_end, long first_row,
                     long n_out, int q, int n_taps, const double *taps, int out_itemsize, int n_cols, const int *cols, void *d_out,
                     int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!d_cdata || !chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status);
    return dev_entry(device, bad, [&](Engine &E) {
        return decimate_run(E, (hipStream_t)stream, nullptr, nullptr, d_cdata, true, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks,
                            n_channels, itemsize, flags, valid_begin, valid_end, first_row, n_out, q, n_taps, taps, out_itemsize, n_cols, cols,
                            d_out, false, chunk_status);
    });
}

int mts_project(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_begin,
                long row_end, int n_cols, const int *cols, const double *offset, int n_out, const double *weights, int out_itemsize, void *out,
                int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status || (cache_id && !chunk_keys));
    return host_entry(device, cache_id, bad, [&](Engine &E, DevCache *c) {
        return project_run(E, nullptr, c, chunk_keys, cdata, false, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels, itemsize,
                           flags, row_begin, row_end, n_cols, cols, offset, n_out, weights, out_itemsize, out, true, chunk_status);
    });
}

int mts_dev_project(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths, const long *chunk_row0,
                    const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_begin, long row_end, int n_cols,
                    const int *cols, const double *offset, int n_out, const double *weights, int out_itemsize, void *d_out, int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!d_cdata || !chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status);
    return dev_entry(device, bad, [&](Engine &E) {
        return project_run(E, (hipStream_t)stream, nullptr, nullptr, d_cdata, true, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks,
                           n_channels, itemsize, flags, row_begin, row_end, n_cols, cols, offset, n_out, weights, out_itemsize, d_out, false,
                           chunk_status);
    });
}

int mts_detect(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
               const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
               long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols,
               const float *threshold, int sign, int reference, int exclude_rows, int exclude_cols, long max_events, long *out_row,
               int *out_pos, float *out_amp, long *n_events, int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status || (cache_id && !chunk_keys));
    return host_entry(device, cache_id, bad, [&](Engine &E, DevCache *c) {
        return detect_run(E, nullptr, c, chunk_keys, cdata, false, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels, itemsize, flags,
                          valid_begin, valid_end, row_begin, row_end, n_taps, taps, n_cols, cols, threshold, sign, reference, exclude_rows,
                          exclude_cols, max_events, out_row, out_pos, out_amp, true, n_events, chunk_status);
    });
}

int mts_dev_detect(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                   const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                   long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols,
                   const float *threshold, int sign, int reference, int exclude_rows, int exclude_cols, long max_events, long *d_row,
                   int *d_pos, float *d_amp, long *n_events, int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!d_cdata || !chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status);
    return dev_entry(device, bad, [&](Engine &E) {
        return detect_run(E, (hipStream_t)stream, nullptr, nullptr, d_cdata, true, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels,
                          itemsize, flags, valid_begin, valid_end, row_begin, row_end, n_taps, taps, n_cols, cols, threshold, sign, reference,
                          exclude_rows, exclude_cols, max_events, d_row, d_pos, d_amp, false, n_events, chunk_status);
    });
}

int mts_welch(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
              const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_seg0,
              long seg_begin, long seg_end, int nperseg, long step, const double *taper, int detrend, int csize, int n_cols,
              const int *cols, double *out, int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status || (cache_id && !chunk_keys));
    return host_entry(device, cache_id, bad, [&](Engine &E, DevCache *c) {
        return welch_run(E, nullptr, c, chunk_keys, cdata, false, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels, itemsize, flags,
                         row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend, csize, n_cols, cols, out, true, chunk_status);
    });
}

int mts_dev_welch(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths, const long *chunk_row0,
                  const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_seg0, long seg_begin, long seg_end,
                  int nperseg, long step, const double *taper, int detrend, int csize, int n_cols, const int *cols, double *d_out,
                  int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!d_cdata || !chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status);
    return dev_entry(device, bad, [&](Engine &E) {
        return welch_run(E, (hipStream_t)stream, nullptr, nullptr, d_cdata, true, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels,
                         itemsize, flags, row_seg0, seg_begin, seg_end, nperseg, step, taper, detrend, csize, n_cols, cols, d_out, false,
                         chunk_status);
    });
}

int mts_gram(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
             const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long range_begin,
             long range_end, long window_rows, long group_begin, long group_end, int n_cols, const int *cols, void *out_gram, void *out_sum,
             int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status || (cache_id && !chunk_keys));
    return host_entry(device, cache_id, bad, [&](Engine &E, DevCache *c) {
        return gram_run(E, nullptr, c, chunk_keys, cdata, false, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels, itemsize, flags,
                        range_begin, range_end, window_rows, group_begin, group_end, n_cols, cols, out_gram, out_sum, true, chunk_status);
    });
}

int mts_dev_gram(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths, const long *chunk_row0,
                 const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long range_begin, long range_end, long window_rows,
                 long group_begin, long group_end, int n_cols, const int *cols, void *d_gram, void *d_sum, int *chunk_status)
{
    const bool bad = n_chunks > 0 && (!d_cdata || !chunk_row0 || !c_offsets || !c_lengths || !n_rows || !chunk_status);
    return dev_entry(device, bad, [&](Engine &E) {
        return gram_run(E, (hipStream_t)stream, nullptr, nullptr, d_cdata, true, c_offsets, c_lengths, chunk_row0, n_rows, n_chunks, n_channels,
                        itemsize, flags, range_begin, range_end, window_rows, group_begin, group_end, n_cols, cols, d_gram, d_sum, false,
                        chunk_status);
    });
}

// ---- debug taps ---------------------------------------------------------------------------------
static int debug_compress_stream(int device, const void *stream_bytes, long n, int level, unsigned char *out, long out_cap,
                                 long *out_len, DebugTap *tap)
{
    Engine *E;
    int rc = get_engine(device, &E);
    if (rc) return rc;
    if (level == -1) level = 6;
    if (level < 1 || level > 9) return MTS_E_ARG;
    if (level < 4 && tap && tap->t_full) return MTS_E_UNSUPPORTED;      // (deflate_fast has no candidate tables)
    if (n < 0 || n >= (1l << 31)) return MTS_E_ARG;
    std::lock_guard<std::mutex> lk(E->mu);
    MTS_HIP(hipSetDevice(E->dev));
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
