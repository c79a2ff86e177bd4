// The decoded-chunk cache on the device (Reader random access): its registry, its entry points, and cache_ensure, which makes the
// chunks of a call resident.  The entries' own bookkeeping (DevCache) is in engine.h.
#include <stdio.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "engine.h"

using namespace mts;

namespace {
std::mutex g_cache_mu;
std::unordered_map<long, DevCache *> g_caches;
long g_cache_next = 1;
}  // namespace
namespace mts {
DevCache *find_cache(long id, int *device)
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    auto it = g_caches.find(id);
    if (it == g_caches.end()) return nullptr;
    if (device) *device = it->second->device;                  // (read under the lock: the cache may be freed once it is released)
    return it->second;
}
bool cache_alive(long id, const DevCache *c) { return find_cache(id) == c; }
void clear_caches_of(int device)
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    for (auto &kv : g_caches) if (kv.second->device == device) kv.second->clear();      // (the caller holds this device's engine lock)
}
void drop_device_caches()
{
    int dev = -1;
    if (hipGetDevice(&dev) == hipSuccess) clear_caches_of(dev);
}
}  // namespace mts

extern "C" {

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
    std::vector<long> soff(n_chunks), coff(m), clen(m), rows(m), ooff(m);
    std::vector<int> st(m);
    // the compressed bytes: chunks that lie back to back in the caller's buffer (a range read or mapped from a .cbin) keep their
    // distances and cross in ONE staged copy (stage_runs, run_copies: codec_plan.h) -- page-locked memory by DMA as it is, anything
    // else (a mapping of the file, a bytes object) through the page-locked pieces, copied by the host threads while the DMA of the
    // piece before runs
    const u64 ctot = stage_runs(c_offsets, c_lengths, miss.data(), m, soff.data());
    u64 otot = 0;
    for (int k = 0; k < m; k++) {
        const int i = miss[k];
        coff[k] = soff[i]; clen[k] = c_lengths[i]; rows[k] = n_rows[i];
        ooff[k] = (long)otot; otot += align_up((u64)rows[k] * row_bytes, 256);
    }
    if ((rc = E->h_in.ensure(ctot + 256))) return rc;
    if ((rc = E->h_out.ensure(otot + 256))) return rc;
    for (const StageCopy &c : run_copies(c_offsets, c_lengths, soff.data(), miss.data(), m))
        if ((rc = staged_h2d(*E, E->h_in.as<u8>() + c.dst, cdata + c.src, (size_t)c.len))) return rc;
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
    CacheLock E;
    if (!E.find(cache_id) || n_chunks < 0 || n_channels <= 0 || row_begin < 0 || row_end < row_begin) return MTS_E_ARG;
    int rc = E.open();
    if (rc) return rc;
    if (n_chunks == 0) return row_end == 0 ? MTS_OK : MTS_E_ARG;
    if ((rc = E.enter(cache_id))) return rc;
    DevCache *c = E.c;
    const u64 row_bytes = (u64)n_channels * itemsize;
    const u64 call_stamp = ++c->clock;
    long total_rows = 0;
    if ((rc = cache_ensure(c, E.E, n_chunks, chunk_keys, cdata, c_offsets, c_lengths, n_rows, n_channels, itemsize, flags, chunk_status, call_stamp, &total_rows, n_channels))) return rc;
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
    CacheLock E;
    if (!E.find(cache_id) || n_chunks < 0 || n_channels <= 0 || n_req < 0 || out_bytes < 0) return MTS_E_ARG;
    if (itemsize != 1 && itemsize != 2 && itemsize != 4 && itemsize != 8) return MTS_E_ARG;
    int rc = E.open();
    if (rc) return rc;
    if (n_chunks == 0 || n_req == 0) return MTS_OK;
    if ((rc = E.enter(cache_id))) return rc;
    DevCache *c = E.c;
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
    WsLayout L{false};
    const size_t o_gc = L.take(sizeof(GatherChunk) * n_chunks), o_req = L.take(sizeof(GatherReq) * n_req);
    if ((rc = E->misc.ensure(L.end + 256))) return rc;
    if ((rc = E->h_out.ensure((u64)out_bytes + 256))) return rc;
    long total_rows_seen = 0;
    if ((rc = cache_ensure(c, E.E, n_chunks, chunk_keys, cdata, c_offsets, c_lengths, n_rows, n_channels, itemsize, flags, chunk_status, call_stamp, &total_rows_seen, n_leading))) return rc;
    // (cache_ensure ends with the residency check and nothing below allocates: the base pointers stay valid)
    std::vector<GatherChunk> gc(n_chunks);
    long r0 = 0;
    for (int i = 0; i < n_chunks; i++) {
        gc[i].row0 = r0; r0 += n_rows[i];
        if (chunk_status[i] == MTS_CHUNK_OK) { const CacheEntry &e = c->map[chunk_keys[i]]; gc[i].base = e.d; gc[i].pitch = e.cols; }
        else { gc[i].base = nullptr; gc[i].pitch = n_channels; }
    }
    MTS_HIP(hipMemcpyAsync(E->misc.as<u8>() + o_gc, gc.data(), sizeof(GatherChunk) * n_chunks, hipMemcpyHostToDevice, nullptr));
    MTS_HIP(hipMemcpyAsync(E->misc.as<u8>() + o_req, gr.data(), sizeof(GatherReq) * n_req, hipMemcpyHostToDevice, nullptr));
    if (max_items && (rc = launch_gather_slices(nullptr, (const GatherChunk *)(E->misc.as<u8>() + o_gc), n_chunks, (const GatherReq *)(E->misc.as<u8>() + o_req), n_req, max_items,
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

}  // extern "C"
