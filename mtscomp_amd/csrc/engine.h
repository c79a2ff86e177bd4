// What the codec (codec.hip), the decoded-chunk cache (cache.hip) and the reductions (reduce.hip) share: the per-device engine and
// its workspaces, the entry guard, the cache's state, the staged copies, the piece loop and the decoder's entry.  Of the functions
// declared here the engine registry, the arena and the staged copies are defined in api.hip, the cache registry in cache.hip, the
// sub-batch drivers in codec.hip.
#pragma once

#include <string.h>

#include <future>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace mts {

void drop_device_caches();      // frees the decoded-chunk caches of the current device (called when a workspace allocation fails)
void *arena_take(size_t bytes); // a piece of the MTS_ARENA_GB arena (api.hip), or nullptr
void arena_reset();

// grow-only device buffer
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
    DBuf stream, sort_a, sort_b, sort_ws, tables, tokens, segbuf, blk, blkcodes, blkhdr, desc, adler, misc;
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
    // snippets: taps, columns, segment tables, the events, the filtered slab, the outputs of the host entry point
    DBuf wav;
    // ... and what the last call did (mts_waveforms_last_plan): pieces, slabs, slabs begun at a gap, the gather kernel's microseconds
    // (measured, slab by slab, only under MTS_WAVEFORMS_TIME)
    long wav_plan[4] = {0, 0, 0, 0};
    hipEvent_t wav_ev[2] = {nullptr, nullptr};
    // template scores: taps, columns, segment tables, the repacked templates, the filtered slab, the output of the host entry point
    DBuf cor;
    // template events: taps, columns, thresholds, segment tables, the repacked templates, the filtered slab, the score slab, its row
    // maxima, the event bitmap, block counts and offsets, the outputs of the host entry point
    DBuf tm;
    // residuals: taps, columns, segment tables, the subtracted events, the plain templates, the filtered slab, the output of the host
    // entry point
    DBuf res;
    // Welch PSD: taper, twiddles, columns, segment tables, block partials, group sums
    DBuf welch;
    // Gram matrices: columns, slab and group tables, slab partials, the accumulators of the host entry point
    DBuf gram;
    // channel-mixing products: weights, offsets, columns, segment tables, the output of the host entry point
    DBuf proj;
    // filtered select: taps, columns, segment tables, centers, selectors, the filtered slab, the histograms and keys of the host entry
    // point
    DBuf zrank;
    // filtered Gram: taps, columns, slab and segment tables, the filtered slab, the partials, the accumulators of the host entry point
    DBuf zgram;
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
        DBuf *all[] = {&stream, &sort_a, &sort_b, &sort_ws, &tables, &tokens, &segbuf, &blk, &blkcodes, &blkhdr, &desc,
                       &adler, &misc, &h_in, &h_out, &inf_scratch, &inf_desc, &segsums, &fast_lists, &fast_state, &stats, &dec, &det, &wav, &cor, &tm, &res, &welch, &gram, &proj, &zrank, &zgram};
        for (DBuf *b : all) b->release();
        arena_reset();                                   // (every piece of it has just been let go)
        geo_n.clear();
        for (auto &g : stg) g.release();
        if (fast_st) (void)hipStreamDestroy(fast_st);
        fast_st = nullptr;
        for (auto &e : fast_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
};

int get_engine(int device, Engine **out);

// What an entry point begins with: open() finds the engine (MTS_E_NODEV, MTS_E_ARG), enter() takes its lock and makes its device
// current.  The entry's own argument checks stand wherever they stood, between or behind the two.
struct MTS_LOCAL EngineLock {
    Engine *E = nullptr;
    std::unique_lock<std::mutex> lk;
    int open(int device) { return get_engine(device, &E); }
    int enter()
    {
        lk = std::unique_lock<std::mutex>(E->mu);
        MTS_HIP(hipSetDevice(E->dev));
        return MTS_OK;
    }
    Engine *operator->() const { return E; }
    Engine &operator*() const { return *E; }
};

// ---- decoded-chunk cache on the device (Reader random access) ------------------------------------
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
DevCache *find_cache(long id, int *device = nullptr);
// mts_cache_destroy unregisters a cache first and frees it under its engine's lock; an entry point that looked the cache
// up before it took that lock asks again once it holds it, and never touches a cache that has gone in between
bool cache_alive(long id, const DevCache *c);
struct MTS_LOCAL CacheLock : EngineLock {
    DevCache *c = nullptr;
    int dev = 0;
    bool find(long id) { c = find_cache(id, &dev); return c != nullptr; }
    int open() { return EngineLock::open(dev); }
    int enter(long id)
    {
        lk = std::unique_lock<std::mutex>(E->mu);
        if (!cache_alive(id, c)) return MTS_E_ARG;             // (destroyed while this call waited for the engine)
        MTS_HIP(hipSetDevice(E->dev));
        return MTS_OK;
    }
};

void clear_caches_of(int device) MTS_LOCAL;      // empties the caches of a device (the caller holds its engine's lock)

// user memory -> device through the pinned pieces; complete on return
int staged_h2d(Engine &E, void *d_dst, const void *src, size_t n);
// device -> user memory, any number of pieces; the device data must be complete
struct CopyItem { void *dst; const void *src; size_t n; };
int staged_d2h_multi(Engine &E, const std::vector<CopyItem> &segs) MTS_LOCAL;

// a piece's copy on a helper thread; when no thread can be started (std::system_error) the copy is made at once, on this one
template <class F>
std::future<int> copy_beside(F &&f, int k)
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

// Piece after piece: while work(k) runs here, copy_in(k + 1) and copy_out(k - 1) (when there is one) run on helper threads.  Piece
// 0's copy in and the last piece's copy out are made on this thread.  Every helper is joined before the return, on error paths too:
// the copies hold references to the caller's frame.  Of several errors work's comes first, then copy_in's, then copy_out's.
template <class In, class Work, class Out>
int run_pieces(int np, In &&copy_in, Work &&work, Out &&copy_out)
{
    constexpr bool has_out = !std::is_same<typename std::decay<Out>::type, std::nullptr_t>::value;
    int rc;
    if (np > 0 && (rc = copy_in(0))) return rc;
    for (int k = 0; k < np; k++) {
        std::future<int> f_in, f_out;
        if (k + 1 < np) f_in = copy_beside(copy_in, k + 1);
        if constexpr (has_out) { if (k >= 1) f_out = copy_beside(copy_out, k - 1); }
        rc = work(k);
        const int rc_in = f_in.valid() ? f_in.get() : MTS_OK, rc_out = f_out.valid() ? f_out.get() : MTS_OK;
        if (rc || rc_in || rc_out) return rc ? rc : rc_in ? rc_in : rc_out;
    }
    if constexpr (has_out) { if (np > 0) return copy_out(np - 1); }
    return MTS_OK;
}
template <class In, class Work>
int run_pieces(int np, In &&copy_in, Work &&work) { return run_pieces(np, copy_in, work, nullptr); }

size_t pipe_piece_bytes();      // MTS_PIPE_BYTES, read per call
std::vector<int> pipe_pieces(const long *n_rows_or_bounds, bool is_bounds, int n_chunks, u64 row_bytes);

int check_items(int sz, int flags);
int dev_decompress(Engine &E, hipStream_t st, const u8 *d_cdata, const long *c_off, const long *c_len, const long *n_rows,
                   int n_chunks, int nc, int sz, int flags, u8 *d_out, const long *out_off, int *status, int nc_full = 0,
                   bool add_times = false);

}  // namespace mts
