"""The CPU twin of tests/test_gpu_prefix_reads.py: what the cases of tests/prefix_cases.py ARE, stated by stdlib zlib, the
pure-Python stream reader and the oracle's transforms alone.  Nothing computed by the device enters here.

Every case: the stream inflates to the oracle's transform of the array, the block table's bytes add up to it, and the oracle's
inverse transform of the first n_need stream bytes -- with k channels, on a stream laid out for 130 -- is arr[:, :k].  Then the
boundary classes: each must be reached by at least one (case, k), so that the GPU test cannot cover nothing without failing here.
"""
import collections
import zlib

import numpy as np
import pytest

from tests import prefix_cases as P

CASES = P.cases()


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_case_is_what_it_says(case):
    stream = zlib.decompress(case.z)
    assert stream == P.stream_of(case.arr, case.flags)
    assert case.table[-1][1] == len(stream) and sum(t[3] for t in case.table) == len(stream)
    assert [t[4] for t in case.table] == [0] * (len(case.table) - 1) + [1]
    assert case.arr.shape == (case.rows, P.NC)
    for k in case.ks:
        need = case.n_need(k)
        i = case.cover(k)
        assert case.table[i][1] >= need and (i == 0 or case.table[i - 1][1] < need)
        assert 2 < case.l_min(k) <= len(case.z) - 4
        assert np.array_equal(P.prefix_inverse(case, k), case.arr[:, :k]), k
        # what the bytes up to L_min hold is enough for zlib too, and one byte less is not (unless the block's last bits are padding
        # or an end-of-block code zlib does not need to see)
        got = zlib.decompressobj().decompress(case.z[:case.l_min(k)], max(need, 1))
        assert len(got) >= need and got[:need] == stream[:need]


def test_every_boundary_class_is_reached():
    count = collections.Counter()
    first = {}
    for case, k in P.pairs():
        for c in case.classes(k):
            count[c] += 1
            first.setdefault(c, (case.name, k))
    for c in P.CLASSES:
        print('%-18s %4d  first: %s' % (c, count[c], first.get(c)))
    assert set(count) <= set(P.CLASSES)
    for c in P.CLASSES:
        assert count[c] >= 1, c
    # the writers the GPU test lists by name
    writers = collections.Counter(c.writer for c in CASES)
    assert all(writers[w] >= 1 for w in ('zlib1', 'zlib6', 'zlib9', 'fixed', 'stored', 'sync', 'full', 'writer')), writers


def test_the_flush_cuts_put_an_empty_stored_block_where_they_say():
    for case in CASES:
        if case.writer not in ('sync', 'full'):
            continue
        k = case.ks[0]
        cut = case.n_need(k) + int(case.name.split('sync')[1][:2]) if case.writer == 'sync' else case.n_need(k)
        empties = [i for i, t in enumerate(case.table) if t[2] == 0 and t[3] == 0]
        assert len(empties) == 1 and case.table[empties[0]][1] == cut, case.name
        if case.writer == 'full':                                    # an ordinary block ends exactly at n_need, the empty one follows
            assert case.cover(k) == empties[0] - 1 and 'exact' in case.classes(k)


def test_sweep_lengths():
    case = CASES[0]
    for k in case.ks:
        ls = case.lengths(k)
        assert ls[0] == 2 and ls[-1] == len(case.z) and all(case.l_min(k) + d in ls for d in range(-2, 3))
        assert all(len(case.z) - d in ls for d in range(6)) and 24 <= len(ls) <= 35
