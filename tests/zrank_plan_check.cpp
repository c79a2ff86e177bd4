// The block arithmetic of k_zrank_hist (csrc/reduce_plan.h: zrank_blocks, zrank_block_rows, zrank_segment) swept on the CPU: for every
// (s0, s1, grid origin, window_rows, H) of a small exhaustive range the segments of all blocks partition [s0, s1) in order, no segment
// crosses a window of the grid and every segment names the window its rows lie in; then the same at rows and windows near 2^62.  Built
// with the address and undefined-behaviour sanitizers as a program of its own (csrc/Makefile: zrank_plan_check) and run by
// tests/test_zrank_plan.py.
#include <stdio.h>
#include <stdlib.h>

#include "reduce_plan.h"

using namespace mts;

static long n_checked = 0;

#define CHECK(cond)                                                                                                                \
    do {                                                                                                                           \
        if (!(cond)) {                                                                                                             \
            printf("FAILED %s (line %d): rows [%ld, %ld) grid from %ld windows of %ld H %ld\n", #cond, __LINE__, s0, s1, row_begin, \
                   window_rows, H);                                                                                                \
            exit(1);                                                                                                               \
        }                                                                                                                          \
    } while (0)

static void check(long s0, long s1, long row_begin, long window_rows, long H)
{
    const long nb = zrank_blocks(s0, s1, H);
    CHECK(nb == (s1 > s0 ? (s1 - s0 - 1) / H + 1 : 0));
    long next = s0;
    for (long b = 0; b < nb; b++) {
        const ZrankSeg B = zrank_block_rows(s0, s1, H, b);
        CHECK(B.r0 == next && B.r0 == s0 + b * H && B.r1 > B.r0 && B.r1 - B.r0 <= H && B.r1 <= s1);     // the blocks partition the rows in order
        CHECK(B.r1 == s1 || B.r1 - B.r0 == H);
        for (long r = B.r0; r < B.r1;) {
            const ZrankSeg S = zrank_segment(r, B.r1, row_begin, window_rows);
            CHECK(S.r0 == r && S.r1 > S.r0 && S.r1 <= B.r1);                                          // so do a block's segments
            CHECK(S.win >= 0 && S.win == (S.r0 - row_begin) / window_rows && S.win == (S.r1 - 1 - row_begin) / window_rows);  // one window, the right one
            CHECK(S.r1 == B.r1 || (S.r1 - row_begin) % window_rows == 0);                            // and it ends at the block's end or the window's
            r = S.r1;
        }
        next = B.r1;
    }
    CHECK(next == (s1 > s0 ? s1 : s0));
    n_checked++;
}

int main()
{
    // exhaustive: every slab [s0, s1) of a grid that begins at or before it
    for (long H = 1; H <= 9; H++)
        for (long window_rows = 1; window_rows <= 11; window_rows++)
            for (long row_begin = 0; row_begin <= 6; row_begin++)
                for (long s0 = row_begin; s0 <= row_begin + 13; s0++)
                    for (long s1 = s0; s1 <= s0 + 25; s1++) check(s0, s1, row_begin, window_rows, H);
    // the kernel's H, around the sizes the GPU tests use, and one window over everything
    for (long H : {4096l, 4095l, 4097l})
        for (long window_rows : {1l, 7l, H - 1, H, H + 1, 5000l, 30000l, 1l << 40})
            for (long row_begin : {0l, 3l, 12345l})
                for (long d0 : {0l, 1l, 4095l, 4096l, 4999l})
                    for (long n : {1l, 2l, 4095l, 4096l, 4097l, 3 * 4096l + 1234})
                        check(row_begin + d0, row_begin + d0 + n, row_begin, window_rows, H);
    // far rows: nothing overflows next to 2^62 (a window's end is never formed as a product)
    const long far = 1l << 62;
    for (long window_rows : {1l, 4096l, (1l << 32) - 1, 1l << 61, far})
        for (long row_begin : {0l, far - 100000})
            for (long s0 : {far - 99999, far - 5000, far - 1})
                check(s0, far, row_begin, window_rows, 4096);
    printf("zrank_plan_check: %ld plans passed\n", n_checked);
    return 0;
}
