// C ABI of libmtscomp_hip.so (include/mtscomp_hip.h), the part every other file stands on: the error text, the per-device engine
// registry, the workspace arena, the staged copies between user memory and the device, and the small entry points (allocate, copy,
// compare, synthesize, the transforms alone).  The codec is in codec.hip, the decoded-chunk cache in cache.hip, the reductions in
// reduce.hip.  No CPU fallback anywhere: without a gfx950 device every compute entry point returns MTS_E_NODEV.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "engine.h"
#include "reduce_plan.h"

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

// MTS_ARENA_GB=N (experiment, round 6; default off): the workspaces of a device come out of ONE allocation of N GiB made when
// the first of them is asked for, 2 MiB-aligned pieces handed out one behind the other (a buffer that grows takes a new piece;
// the arena is given back by mts_release).  Asks whether k_match5's three times -- the physical placement of its workspace,
// tools/m5_addr_times.py -- go away when the placement is one big block instead of a dozen allocations made between others.
struct Arena { u8 *base = nullptr; size_t cap = 0, used = 0; bool tried = false; };
static Arena g_arena[64];
static size_t arena_gb() { static const size_t v = [] { const char *e = getenv("MTS_ARENA_GB"); return e ? (size_t)atoll(e) : (size_t)0; }(); return v; }
void *arena_take(size_t bytes)
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
void arena_reset()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return;
    Arena &A = g_arena[dev];
    if (A.base) (void)hipFree(A.base);
    A = Arena();
}

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

int get_engine(int device, Engine **out)
{
    const int n = device_count();
    if (n <= 0) { set_error("no gfx950 device visible (libmtscomp_hip has no CPU path)"); return MTS_E_NODEV; }
    if (device < 0 || device >= n) { set_error("device %d out of range (%d visible)", device, n); return MTS_E_ARG; }
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_engines[device]) { g_engines[device] = new Engine(); g_engines[device]->dev = device; }
    *out = g_engines[device];
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
static bool host_ptr_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

int staged_d2h_multi(Engine &E, const std::vector<CopyItem> &segs)
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

// user memory -> device; complete on return
int staged_h2d(Engine &E, void *d_dst, const void *src, size_t n)
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
size_t pipe_piece_bytes()
{
    const char *e = getenv("MTS_PIPE_BYTES");
    return e ? (size_t)atoll(e) : ((size_t)256 << 20);
}
std::vector<int> pipe_pieces(const long *n_rows_or_bounds, bool is_bounds, int n_chunks, u64 row_bytes)
{
    return cut_pieces(n_rows_or_bounds, is_bounds, n_chunks, row_bytes, pipe_piece_bytes());
}

int check_items(int sz, int flags)
{
    if (sz != 1 && sz != 2 && sz != 4 && sz != 8) { set_error("itemsize %d unsupported", sz); return MTS_E_ARG; }
    if ((flags & MTS_FLAG_FLOAT) && sz != 4 && sz != 8) { set_error("float items of %d bytes unsupported", sz); return MTS_E_ARG; }
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

void mts_release(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    for (Engine *e : g_engines)
        if (e) {
            std::lock_guard<std::mutex> l2(e->mu);
            (void)hipSetDevice(e->dev);
            e->release_all();
            clear_caches_of(e->dev);
        }
}

int mts_delta_transpose(int device, const void *raw, long n_samples, int n_channels, int itemsize, int flags,
                        void *stream_out)
{
    EngineLock E;
    int rc = E.open(device);
    if (rc) return rc;
    if (itemsize != 1 && itemsize != 2 && itemsize != 4 && itemsize != 8) return MTS_E_ARG;
    if (n_samples < 0 || n_channels <= 0) return MTS_E_ARG;
    if ((rc = E.enter())) return rc;
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
    EngineLock E;
    int rc = E.open(device);
    if (rc) return rc;
    if (itemsize != 1 && itemsize != 2 && itemsize != 4 && itemsize != 8) return MTS_E_ARG;
    if (n_samples < 0 || n_channels <= 0) return MTS_E_ARG;
    if ((rc = E.enter())) return rc;
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
    EngineLock E;
    int rc = E.open(device);
    if (rc) return rc;
    if ((rc = E.enter())) return rc;
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
    EngineLock E;
    int rc = E.open(device);
    if (rc) return rc;
    if (nbytes < 0 || !n_diff) return MTS_E_ARG;
    if (((uintptr_t)d_a | (uintptr_t)d_b) & 15) { set_error("mts_dev_compare: buffers must be 16-byte aligned"); return MTS_E_ARG; }
    if ((rc = E.enter())) return rc;
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

}  // extern "C"
