// The slab arithmetic of the filtered Gram (csrc/reduce_plan.h: gram_group_rows, gram_cut_slabs, zgram_cap_rows, zgram_slabs) swept on
// the CPU.  For every grid (range, window_rows), group and slab size, column count and byte bound of a small exhaustive range, and
// for every way of cutting the call's groups into pieces at group boundaries: every row of every group lies in exactly one z slab;
// every z slab starts and ends on a Gram-slab boundary of its group or at the group's end; a Gram slab never straddles two z slabs;
// the bound is kept (rounded down to whole Gram slabs, never less than one); groups of 1 row and windows of GROUP_ROWS + 1 rows
// work.  Then the library's own sizes.  Built with the address and undefined-behaviour sanitizers as a program of its own
// (csrc/Makefile: zgram_plan_check) and run by tests/test_zgram_plan.py.
#include <stdio.h>
#include <stdlib.h>

#include "reduce_plan.h"

using namespace mts;

static long n_checked = 0;

#define CHECK(cond)                                                                                                                  \
    do {                                                                                                                             \
        if (!(cond)) {                                                                                                               \
            printf("FAILED %s (line %d): range [%ld, %ld) windows of %ld groups of %ld slabs of %ld, %d columns, %llu bytes, %ld slabs a launch\n", \
                   #cond, __LINE__, rb, re, window_rows, GR, SR, n_cols, (unsigned long long)bytes, cap_slabs);                      \
            exit(1);                                                                                                                 \
        }                                                                                                                            \
    } while (0)

// groups [g0, g1) of the grid as one piece
static void check(long rb, long re, long window_rows, long GR, long SR, int n_cols, uint64_t bytes, long cap_slabs, long g0, long g1)
{
    const long K = (window_rows + GR - 1) / GR, n = re - rb;
    const long total = n / window_rows * K + (n % window_rows + GR - 1) / GR;
    CHECK(0 <= g0 && g0 < g1 && g1 <= total);
    std::vector<long> slab_rows, gfirst, glo, ghi;
    long next = -1;
    for (long g = g0; g < g1; g++) {
        long lo, hi;
        gram_group_rows(rb, re, window_rows, GR, g, &lo, &hi);
        CHECK(rb <= lo && lo < hi && hi <= re && hi - lo <= GR);
        CHECK((lo - rb) / window_rows == (hi - 1 - rb) / window_rows);                 // one window
        CHECK((lo - rb) % window_rows % GR == 0);                                      // aligned to the window's start
        CHECK(next < 0 || lo == next);                                                 // adjacent
        CHECK(hi - lo == GR || hi == re || (hi - rb) % window_rows == 0);              // short only at a window's or the range's end
        next = hi;
        glo.push_back(lo); ghi.push_back(hi);
        gfirst.push_back((long)slab_rows.size() / 2);
        gram_cut_slabs(lo, hi, SR, slab_rows);
        CHECK((long)slab_rows.size() / 2 - gfirst.back() == (hi - lo + SR - 1) / SR);
    }
    const long n_slabs = (long)slab_rows.size() / 2;
    gfirst.push_back(n_slabs);
    if (g0 == 0 && g1 == total) CHECK(glo[0] == rb && next == re);
    const long cap = zgram_cap_rows(bytes, n_cols, SR);
    CHECK(cap >= SR && cap % SR == 0);
    CHECK(cap == SR || (uint64_t)cap * 4 * (uint64_t)n_cols <= bytes);                 // the bound, unless it holds less than one Gram slab
    CHECK((uint64_t)(cap + SR) * 4 * (uint64_t)n_cols > bytes || cap == (1l << 40) / SR * SR);   // and no slab less than it allows
    const std::vector<ZgramSlab> Z = zgram_slabs(slab_rows.data(), 0, n_slabs, cap, cap_slabs);
    long s = 0, row = glo[0];
    for (const ZgramSlab &z : Z) {
        CHECK(z.s0 == s && z.s1 > z.s0 && z.s1 <= n_slabs);                            // every Gram slab in exactly one z slab, in order
        CHECK(z.s1 - z.s0 <= cap_slabs);
        const long a = slab_rows[2 * z.s0], b = slab_rows[2 * z.s1 - 1];
        CHECK(a == row && b > a && b - a <= cap);                                      // so every row; the bound in rows
        // its ends: a Gram-slab boundary of the group they lie in, or the group's end
        const long ga = std::upper_bound(gfirst.begin(), gfirst.end(), z.s0) - gfirst.begin() - 1;
        const long gb = std::upper_bound(gfirst.begin(), gfirst.end(), z.s1 - 1) - gfirst.begin() - 1;
        CHECK(glo[ga] <= a && a < ghi[ga] && (a - glo[ga]) % SR == 0);
        CHECK(glo[gb] < b && b <= ghi[gb] && ((b - glo[gb]) % SR == 0 || b == ghi[gb]));
        for (long q = z.s0; q < z.s1; q++) {                                           // the Gram slabs inside: adjacent rows, whole
            CHECK(slab_rows[2 * q] >= a && slab_rows[2 * q + 1] <= b && slab_rows[2 * q + 1] - slab_rows[2 * q] <= SR);
            if (q > z.s0) CHECK(slab_rows[2 * q] == slab_rows[2 * q - 1]);
        }
        // greedy: the next Gram slab did not fit
        if (z.s1 < n_slabs) CHECK(z.s1 - z.s0 == cap_slabs || slab_rows[2 * z.s1 + 1] - a > cap);
        s = z.s1; row = b;
    }
    CHECK(s == n_slabs && row == ghi.back());
    n_checked++;
}

// every run of groups [g0, g1) of the grid
static void check_grid(long rb, long re, long window_rows, long GR, long SR, int n_cols, uint64_t bytes, long cap_slabs)
{
    const long K = (window_rows + GR - 1) / GR, n = re - rb;
    const long total = n / window_rows * K + (n % window_rows + GR - 1) / GR;
    for (long g0 = 0; g0 < total; g0++)
        for (long g1 = g0 + 1; g1 <= total; g1++) check(rb, re, window_rows, GR, SR, n_cols, bytes, cap_slabs, g0, g1);
}

int main()
{
    // exhaustive, small: groups of 1 row (GR = 1; a window of GR + 1 rows leaves one), slabs of 1 row, bounds below one Gram slab
    for (long GR : {1l, 2l, 4l, 6l})
        for (long SR : {1l, 2l, 3l})
            if (GR % SR == 0 || GR == 1)
                for (long window_rows : {1l, 2l, GR - 1 > 0 ? GR - 1 : 1l, GR, GR + 1, 2 * GR + 1, 100l})
                    for (long rb : {0l, 5l})
                        for (long n = 1; n <= 11; n++)
                            for (int n_cols : {1, 3})
                                for (uint64_t bytes : {1, 12, 24, 25, 48, 1 << 20})
                                    for (long cap_slabs : {1l, 2l, 65535l}) check_grid(rb, rb + n, window_rows, GR, SR, n_cols, bytes, cap_slabs);
    // the library's sizes: a group of GROUP_ROWS + 1 rows' window, the GPU tests' bounds (one Gram slab a z slab) and the default
    const long GR = 1l << 20, SR = 4096;
    for (long window_rows : {4095l, 4096l, 4097l, 3 * 4096l + 5, GR, GR + 1, GR + 4097})
        for (long n : {1l, 4097l, GR + 1, GR + 4097, 2 * GR + 3})
            for (int n_cols : {1, 2, 5, 65, 385, 1024, 16384})
                for (uint64_t bytes : {(uint64_t)1, (uint64_t)SR * 4 * n_cols, (uint64_t)SR * 4 * n_cols * 2 - 1, (uint64_t)SR * 4 * n_cols * 3, (uint64_t)256 << 20, (uint64_t)1 << 62}) {
                    const long K = (window_rows + GR - 1) / GR;
                    const long total = n / window_rows * K + (n % window_rows + GR - 1) / GR;
                    for (long cap_slabs : {1l, 292l, 65535l}) {
                        check(3, 3 + n, window_rows, GR, SR, n_cols, bytes, cap_slabs, 0, total);
                        check(3, 3 + n, window_rows, GR, SR, n_cols, bytes, cap_slabs, total - 1, total);
                        if (total > 1) check(3, 3 + n, window_rows, GR, SR, n_cols, bytes, cap_slabs, 0, total - 1);
                    }
                }
    printf("zgram_plan_check: %ld plans passed\n", n_checked);
    return 0;
}
