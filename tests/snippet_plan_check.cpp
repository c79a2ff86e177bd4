// SnippetPlan (csrc/reduce_plan.h) swept on the CPU: random ascending event rows with duplicates, at every cap, gap, snippet shape
// and recording edge that takes another path.  Built with the address and undefined-behaviour sanitizers as a program of its own
// (csrc/Makefile: snippet_plan_check) and run by tests/test_snippet_plan.py.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "reduce_plan.h"

using namespace mts;

static long n_checked = 0;

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            printf("FAILED %s (line %d): n %ld before %ld after %ld vb %ld ve %ld cap %ld gap %ld seed %u\n", #cond, __LINE__, \
                   (long)row.size(), before, after, vb, ve, cap, gap, seed);                                                 \
            exit(1);                                                                                                         \
        }                                                                                                                    \
    } while (0)

static void check(const std::vector<long> &row, long e0, long e1, long before, long after, long vb, long ve, long cap, long gap, unsigned seed)
{
    const long T = before + after;
    const SnippetPlan P(row.data(), e0, e1, before, after, vb, ve, cap, gap);
    long next = e0, max_rows = 0;
    for (const SnippetSlab &S : P.slabs) {
        CHECK(S.e0 == next && S.e1 > S.e0 && S.e1 <= e1);                     // the slabs partition the events in order
        CHECK(S.a == std::max(vb, row[S.e0] - before) && S.b == std::min(ve, row[S.e1 - 1] + after));
        CHECK(S.a <= S.b && S.a >= vb && S.b <= ve);                          // (empty: the snippets lie wholly outside the recording)
        CHECK(S.b - S.a <= std::max(cap, T));
        long b = 0;                                                           // the rows filtered by the events before e
        for (long e = S.e0; e < S.e1; e++) {
            const long a = std::max(vb, row[e] - before), bb = std::min(ve, row[e] + after);
            CHECK(S.a <= a && bb <= S.b);                                     // every row of the recording that the event reads
            if (e > S.e0 && gap >= 0) CHECK(a - b <= gap);                    // no slab spans a gap above the setting
            b = e > S.e0 ? std::max(b, bb) : bb;
        }
        // a cut has a reason: the next event fits neither the cap nor the gap
        if (S.e1 < e1) {
            const long a = std::max(vb, row[S.e1] - before), bb = std::min(ve, row[S.e1] + after);
            CHECK(bb - S.a > std::max(cap, T) || (gap >= 0 && a - S.b > gap));
        }
        max_rows = std::max(max_rows, S.b - S.a);
        next = S.e1;
    }
    CHECK(next == e1 || (e1 <= e0 && P.slabs.empty()));
    CHECK(P.max_rows == max_rows);
    n_checked++;
}

int main()
{
    std::mt19937 rng(12345);
    const long shapes[][2] = {{20, 41}, {0, 1}, {1, 0}, {5, 0}, {0, 7}, {3, 3}, {2000, 2096}};
    for (unsigned seed = 0; seed < 60; seed++) {
        for (const auto &sh : shapes) {
            const long before = sh[0], after = sh[1], T = before + after;
            const long vb = (seed % 3 == 0) ? 0 : (long)(rng() % 1000), len = 1 + (long)(rng() % (seed % 2 ? 200000 : 3000)), ve = vb + len;
            const int n = (int)(rng() % 400);
            // clusters, duplicates, far-apart events, events on the first and the last row of the recording
            std::vector<long> row;
            long r = vb;
            for (int i = 0; i < n; i++) {
                const unsigned k = rng() % 8;
                const long step = k < 3 ? 0 : k < 6 ? (long)(rng() % (2 * T + 2)) : k < 7 ? (long)(rng() % 5000) : (long)(rng() % 20000);
                r = std::min(ve - 1, r + step);
                row.push_back(r);
            }
            if (n > 2 && seed % 4 == 1) { row[0] = vb; row[n - 1] = ve - 1; }
            const long caps[] = {T, T + 1, 3 * T, 1l << 40, 1, 0};
            const long gaps[] = {0, 1, 4096, -1};
            for (long cap : caps)
                for (long gap : gaps) {
                    check(row, 0, n, before, after, vb, ve, cap, gap, seed);
                    if (n > 4) check(row, n / 3, 2 * n / 3, before, after, vb, ve, cap, gap, seed);       // the events of one piece
                    check(row, n / 2, n / 2, before, after, vb, ve, cap, gap, seed);                      // none
                }
        }
    }
    printf("snippet_plan_check: %ld plans passed\n", n_checked);
    return 0;
}
