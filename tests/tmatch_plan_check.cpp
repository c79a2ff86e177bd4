// TmatchSlabs (csrc/reduce_plan.h) swept on the CPU: the slabs of every piece of random calls, at every slab bound, exclusion radius,
// template shape and recording edge that takes another path.  Built with the address and undefined-behaviour sanitizers as a program
// of its own (csrc/Makefile: tmatch_plan_check) and run by tests/test_tmatch_plan.py.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "reduce_plan.h"

using namespace mts;

static long n_checked = 0;

#define CHECK(cond)                                                                                                                   \
    do {                                                                                                                              \
        if (!(cond)) {                                                                                                                \
            printf("FAILED %s (line %d): rows [%ld, %ld) of [%ld, %ld) R %ld before %ld T %ld cols %ld out %ld bytes %llu max %ld\n", \
                   #cond, __LINE__, p0, p1, vb, ve, R, before, T, n_cols, n_out, (unsigned long long)bytes, max_rows);                 \
            exit(1);                                                                                                                  \
        }                                                                                                                             \
    } while (0)

// one piece [p0, p1) of a call on rows [row_begin, row_end)
static void check(long row_begin, long row_end, long p0, long p1, long R, long before, long T, long vb, long ve, long n_cols, long n_out,
                  uint64_t bytes, long max_rows)
{
    const TmatchSlabs SL(row_end - row_begin, R, before, T, vb, ve, n_cols, n_out, bytes, max_rows);
    const long after = T - before;
    CHECK(SL.own >= 1 && SL.own <= row_end - row_begin && SL.sc_rows == SL.own + 2 * R && SL.z_rows == SL.sc_rows + T - 1);
    // within the bounds, or one row with its neighbours
    CHECK(SL.own == 1 || ((uint64_t)SL.z_rows * n_cols * 4 <= bytes && (uint64_t)SL.sc_rows * n_out * 4 <= bytes && SL.z_rows <= max_rows));
    // the largest such count
    if (SL.own < row_end - row_begin)
        CHECK((uint64_t)(SL.z_rows + 1) * n_cols * 4 > bytes || (uint64_t)(SL.sc_rows + 1) * n_out * 4 > bytes || SL.z_rows + 1 > max_rows);
    long next = p0;
    for (long s0 = p0; s0 < p1; s0 += SL.own) {
        const TmatchSlab S = SL.at(s0, p1);
        CHECK(S.s0 == next && S.s1 > S.s0 && S.s1 <= p1 && S.s1 - S.s0 <= SL.own);          // the slabs partition the piece in order
        CHECK(S.sa >= vb && S.sb <= ve && S.sa <= S.s0 && S.s1 <= S.sb);                    // the owned rows have scores
        CHECK(S.sb - S.sa <= SL.sc_rows && S.b - S.a <= SL.z_rows && S.a <= S.b && S.a >= vb && S.b <= ve);
        for (long t : {S.s0, S.s1 - 1})                                                     // every row of the recording within R has a score
            CHECK(S.sa <= std::max(vb, t - R) && std::min(ve, t + R + 1) <= S.sb);
        // every row of the recording that a score reads is filtered
        const long lo = std::max(vb, S.sa - before), hi = std::min(ve, S.sb - 1 - before + T);
        if (lo < hi) CHECK(S.a <= lo && hi <= S.b);
        if (S.b > S.a) CHECK(S.a >= S.sa - before && S.b <= S.sb + after - 1);              // and no other
        next = S.s1;
    }
    CHECK(next == p1);
    n_checked++;
}

int main()
{
    std::mt19937 rng(2024);
    const long shapes[][2] = {{20, 61}, {0, 1}, {1, 1}, {0, 7}, {7, 7}, {3, 9}, {256, 256}, {0, 256}};
    const long radii[] = {0, 1, 2, 63, 64, 255};
    for (unsigned seed = 0; seed < 12; seed++)
        for (const auto &sh : shapes)
            for (long R : radii) {
                const long before = sh[0], T = sh[1];
                const long vb = 0, ve = 1 + (long)(rng() % (seed % 2 ? 3000 : 700));
                long row_begin = (long)(rng() % ve), row_end = row_begin + 1 + (long)(rng() % (ve - row_begin));
                if (seed % 5 == 0) { row_begin = 0; row_end = ve; }
                const long n_cols = 1 + (long)(rng() % (seed % 3 ? 8 : 1024)), n_out = 1 + (long)(rng() % (seed % 4 ? 5 : 1024));
                const long n = row_end - row_begin;
                const uint64_t one = 4 * (uint64_t)std::max(n_cols, n_out);
                const uint64_t sizes[] = {1, one, one * (uint64_t)(2 * R + T), one * (uint64_t)(2 * R + T + 1), one * (uint64_t)(2 * R + T + n / 5 + 1),
                                          256ull << 20, ~0ull >> 1};
                const long maxes[] = {1l << 22, 2 * R + T, 2 * R + T + 3, 1};
                for (uint64_t bytes : sizes)
                    for (long max_rows : maxes) {
                        check(row_begin, row_end, row_begin, row_end, R, before, T, vb, ve, n_cols, n_out, bytes, max_rows);
                        const long c1 = row_begin + n / 3, c2 = row_begin + 2 * n / 3;             // three pieces
                        check(row_begin, row_end, row_begin, c1, R, before, T, vb, ve, n_cols, n_out, bytes, max_rows);
                        check(row_begin, row_end, c1, c2, R, before, T, vb, ve, n_cols, n_out, bytes, max_rows);
                        check(row_begin, row_end, c2, row_end, R, before, T, vb, ve, n_cols, n_out, bytes, max_rows);
                    }
            }
    printf("tmatch_plan_check: %ld plans passed\n", n_checked);
    return 0;
}
