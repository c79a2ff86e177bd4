// MeanParts (csrc/reduce_plan.h) swept on the CPU: the events of a slab grouped by label and cut into parts, for random labels -- one
// label, one event a label, labels without events, long runs -- at every part size that takes another path.  Built with the address
// and undefined-behaviour sanitizers as a program of its own (csrc/Makefile: mean_plan_check) and run by tests/test_mean_plan.py.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "reduce_plan.h"

using namespace mts;

static long n_checked = 0;

#define CHECK(cond)                                                                                                            \
    do {                                                                                                                       \
        if (!(cond)) {                                                                                                         \
            printf("FAILED %s (line %d): n %ld e0 %ld e1 %ld labels %d part %ld seed %u\n", #cond, __LINE__, (long)label.size(), \
                   e0, e1, n_labels, part, seed);                                                                              \
            exit(1);                                                                                                           \
        }                                                                                                                      \
    } while (0)

static void check(const std::vector<int> &label, long e0, long e1, int n_labels, long part, unsigned seed)
{
    const MeanParts M(label.data(), e0, e1, part);
    const long n = e1 > e0 ? e1 - e0 : 0, cap = part < 1 ? 1 : part;
    CHECK((long)M.perm.size() == n);
    // the perm is a permutation of [e0, e1), labels ascending, the order within a label the list's (stable)
    std::vector<char> seen((size_t)n, 0);
    for (long k = 0; k < n; k++) {
        const long e = M.perm[(size_t)k];
        CHECK(e >= e0 && e < e1 && !seen[(size_t)(e - e0)]);
        seen[(size_t)(e - e0)] = 1;
        if (k) {
            const long p = M.perm[(size_t)k - 1];
            CHECK(label[(size_t)p] < label[(size_t)e] || (label[(size_t)p] == label[(size_t)e] && p < e));
        }
    }
    // the parts partition the perm in order; none is empty or longer than the cap; a part holds one label, and that label's events
    long next = e0;
    std::vector<long> per((size_t)n_labels, 0), want((size_t)n_labels, 0);
    for (long e = e0; e < e1; e++) want[(size_t)label[(size_t)e]]++;
    for (size_t q = 0; q < M.parts.size(); q++) {
        const MeanPart &P = M.parts[q];
        CHECK(P.first == next && P.count >= 1 && (long)P.count <= cap && P.first + P.count <= e1);
        CHECK(P.label >= 0 && P.label < n_labels);
        for (long k = 0; k < P.count; k++) CHECK(label[(size_t)M.perm[(size_t)(P.first - e0 + k)]] == P.label);
        // a cut has a reason: the label changes, or the part before is full
        if (q) CHECK(M.parts[q - 1].label < P.label || (M.parts[q - 1].label == P.label && (long)M.parts[q - 1].count == cap));
        per[(size_t)P.label] += P.count;
        next = P.first + P.count;
    }
    CHECK(next == e1 || (n == 0 && M.parts.empty()));
    for (int l = 0; l < n_labels; l++) CHECK(per[(size_t)l] == want[(size_t)l]);
    n_checked++;
}

int main()
{
    std::mt19937 rng(4321);
    const int label_counts[] = {1, 2, 5, 128, 300, 4096};
    for (unsigned seed = 0; seed < 40; seed++) {
        for (int n_labels : label_counts) {
            const int n = seed % 5 == 0 ? (int)(rng() % 6) : (int)(rng() % 3000);
            std::vector<int> label;
            for (int i = 0; i < n; i++) {
                const unsigned k = rng() % 4;
                // uniform labels, a dominant label, runs of one label, the last label
                label.push_back(k == 0 ? (int)(rng() % (unsigned)n_labels) : k == 1 ? 0 : k == 2 && i ? label[(size_t)i - 1] : n_labels - 1 - (int)(rng() % 2u) % n_labels);
            }
            if (seed % 7 == 3) for (int i = 0; i < n; i++) label[(size_t)i] = i % n_labels;                   // one event a label, round and round
            const long parts[] = {1, 2, 3, 16, 64, 256, 1l << 20, 0, -5};
            for (long part : parts) {
                check(label, 0, n, n_labels, part, seed);
                if (n > 4) check(label, n / 3, 2 * n / 3, n_labels, part, seed);                              // the events of one slab
                check(label, n / 2, n / 2, n_labels, part, seed);                                             // none
            }
        }
    }
    printf("mean_plan_check: %ld plans passed\n", n_checked);
    return 0;
}
