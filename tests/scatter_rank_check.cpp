// The rank arithmetic of the one-pass hash sort's scatter (mtscomp_amd/csrc/op_rank.h, used by k_op_scatter) replayed on the CPU:
// one slice of 16 waves x 8 instructions x 64 lanes, the lane-ordered LDS atomics emulated as a loop over the lanes.
//   phase 1  every key adds one to its bucket's 16-bit half of its wave's counter word and keeps what the atomic returned
//   phase 2  the workgroup's scan turns the counters into every wave's first places (both halves of a word at once)
//   phase 3  place = first place of the key's wave and bucket (a plain read) + the rank kept in phase 1
// The places must be a stable counting sort of the slice: a permutation of 0 .. keys - 1, buckets ascending, positions ascending
// inside a bucket -- and the places the kernel gave before (a second atomic on the scanned word instead of the kept rank).
// No GPU, not loaded into Python; built with the sanitizers (Makefile: scatter_rank_check).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <numeric>
#include <vector>

#include "op_rank.h"

using namespace mts;
typedef uint32_t u32;

static const int WAVES = 16, KPL = 8, LANES = 64, SLICE = WAVES * KPL * LANES, LMAX = 1024;

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "%s: ", name); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "  (%s, line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

// phase 2 as the kernel does it: thread j takes buckets 2 j and 2 j + 1
static void scan_counters(std::vector<u32> &cw)
{
    u32 run_all = 0;
    for (int j = 0; j < LMAX / 2; j++) {
        u32 c[WAVES], tot = 0;
        for (int w = 0; w < WAVES; w++) { c[w] = cw[w * (LMAX / 2) + j]; tot += c[w]; }
        const u32 c0 = tot & 0xffffu, c1 = tot >> 16;
        const u32 st0 = run_all, st1 = st0 + c0;
        run_all += c0 + c1;
        u32 run = st0 | (st1 << 16);
        for (int w = 0; w < WAVES; w++) { cw[w * (LMAX / 2) + j] = run; run += c[w]; }
    }
}

static void run_case(const char *name, int nkeys, const std::function<u32(int)> &bucket_of)
{
    std::vector<u32> id(SLICE);
    for (int i = 0; i < SLICE; i++) { id[i] = bucket_of(i); CHECK(id[i] < (u32)LMAX, "bucket %u of key %d", id[i], i); }
    auto key = [](int w, int k, int lane) { return w * KPL * LANES + k * LANES + lane; };

    // the new kernel
    std::vector<u32> cw(WAVES * (LMAX / 2), 0), idr(SLICE), slot(SLICE, ~0u);
    for (int w = 0; w < WAVES; w++)
        for (int k = 0; k < KPL; k++)
            for (int lane = 0; lane < LANES; lane++) {
                const int i = key(w, k, lane);
                idr[i] = id[i];
                if (i >= nkeys) continue;
                u32 &word = cw[w * (LMAX / 2) + op_cw_word(id[i])];
                const u32 old = word;
                word += op_cw_one(id[i]);
                idr[i] = op_pack_rank(id[i], old);
                CHECK(op_rank_id(idr[i]) == id[i] && (idr[i] >> OP_ID_BITS) < (u32)(KPL * LANES), "key %d: bucket %u rank %u", i, op_rank_id(idr[i]), idr[i] >> OP_ID_BITS);
            }
    scan_counters(cw);
    for (int i = 0; i < nkeys; i++) slot[i] = op_slot(idr[i], cw[(i / (KPL * LANES)) * (LMAX / 2) + op_cw_word(id[i])]);

    // the kernel as it was: count, scan, then a second atomic on the scanned word
    std::vector<u32> cw2(WAVES * (LMAX / 2), 0), slot2(SLICE, ~0u);
    for (int i = 0; i < nkeys; i++) cw2[(i / (KPL * LANES)) * (LMAX / 2) + (id[i] >> 1)] += 1u << (16 * (id[i] & 1));
    scan_counters(cw2);
    for (int w = 0; w < WAVES; w++)
        for (int k = 0; k < KPL; k++)
            for (int lane = 0; lane < LANES; lane++) {
                const int i = key(w, k, lane);
                if (i >= nkeys) continue;
                u32 &word = cw2[w * (LMAX / 2) + (id[i] >> 1)];
                const u32 sh = 16 * (id[i] & 1);
                slot2[i] = (word >> sh) & 0xffffu;
                word += 1u << sh;
            }

    // a stable counting sort of the slice
    std::vector<int> order(nkeys);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return id[a] < id[b]; });
    std::vector<int> at(nkeys, -1);
    for (int i = 0; i < nkeys; i++) {
        CHECK(slot[i] < (u32)nkeys, "key %d: place %u of %d", i, slot[i], nkeys);
        CHECK(at[slot[i]] < 0, "keys %d and %d share place %u", at[slot[i]], i, slot[i]);
        at[slot[i]] = i;
        CHECK(slot[i] == slot2[i], "key %d: place %u, the two-atomic kernel's %u", i, slot[i], slot2[i]);
    }
    for (int p = 0; p < nkeys; p++) CHECK(at[p] == order[p], "place %d holds key %d (bucket %u), a stable sort puts key %d (bucket %u) there", p, at[p], id[at[p]], order[p], id[order[p]]);
    u32 half_max = 0;
    {
        std::vector<u32> per(WAVES * LMAX, 0);
        for (int i = 0; i < nkeys; i++) half_max = std::max(half_max, ++per[(i / (KPL * LANES)) * LMAX + id[i]]);
    }
    std::printf("%-36s %5d keys, largest per-wave count of a bucket %3u: ok\n", name, nkeys, half_max);
}

int main()
{
    u32 lcg = 12345;
    auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return lcg >> 8; };
    run_case("one bucket, even id", SLICE, [](int) { return 6u; });
    run_case("one bucket, odd id", SLICE, [](int) { return 7u; });
    run_case("one bucket, last id", SLICE, [](int) { return 1023u; });
    {
        std::vector<u32> b(SLICE);
        for (auto &x : b) x = 40u + (rnd() & 1u);
        run_case("two buckets in one counter word", SLICE, [&](int i) { return b[i]; });
        for (auto &x : b) { const u32 r = rnd() % 100; x = r < 45 ? 40u : r < 90 ? 41u : rnd() % 1024; }
        run_case("two popular buckets and the rest", SLICE, [&](int i) { return b[i]; });
        run_case("ends in the middle of a wave", 5 * KPL * LANES + 3 * LANES + 37, [&](int i) { return b[i]; });
        run_case("37 keys", 37, [&](int i) { return b[i]; });
        run_case("ends with a whole wave", 9 * KPL * LANES, [&](int i) { return b[i]; });
        for (auto &x : b) x = rnd() % 1024;
        run_case("random over 1024 buckets", SLICE, [&](int i) { return b[i]; });
    }
    run_case("1024 distinct buckets, ascending", SLICE, [](int i) { return (u32)(i % 1024); });
    run_case("1024 distinct buckets, descending", SLICE, [](int i) { return (u32)(1023 - i % 1024); });
    run_case("1024 distinct buckets, strided", SLICE, [](int i) { return (u32)((i * 613) % 1024); });
    std::printf("scatter_rank_check: all cases passed\n");
    return 0;
}
