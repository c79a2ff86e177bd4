"""k_match5's ring phase (match.hip): commit() and the mask phase of a 64-slot group exist once per phase (group & 3), and the
ninth word of every filter-table row is a copy of word 0, which the upper half-wave reads as "the word behind word 7".  What that
can break is a candidate seen through word 8 by a lane of the upper half, in one phase, in one of the four tables.

The stream: 700 records of 8 bytes whose starts share b'abc' -- ONE hash run in position order, a slot per record.  Bytes 3..7 are
pseudo-random per record, the first k of them 0x55 in every record: every candidate passes the tables below level k, and table k
has to find the planted one.  Records 300..555 (256 consecutive slots: all four phases, both half-waves) copy the tail of the
record j before them; the j put the planted candidate in every word of the 128 bits behind a lane, word 0 and its copy included.
At level 6 (chain budget 128) every target's match is 8 j back, which is asserted on the oracle's table before the device's
is compared with it; at levels 4 and 5 (budgets 16 and 32) most planted candidates are out of budget: tables only.
"""
import functools

import numpy as np
import pytest

from mtscomp_amd import hip
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RECORDS = 700
FIRST, LAST = 300, 555                                           # the targets, in ascending order
BACK = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)
LEVELS = (4, 5, 6)
M64 = (1 << 64) - 1


def stream(k, j):
    rec = np.zeros((RECORDS, 8), dtype=np.uint8)
    rec[:, 0:3] = np.frombuffer(b'abc', dtype=np.uint8)
    for r in range(RECORDS):
        z = ((r + 1) * 0x9E3779B97F4A7C15) & M64
        v = z ^ (z >> 29)
        rec[r, 3:8] = [(v >> (8 * b)) & 0xff for b in range(5)]
    rec[:, 3:3 + k] = 0x55
    for r in range(FIRST, LAST + 1):
        rec[r, 3:8] = rec[r - j, 3:8]
    return rec.tobytes()


@functools.lru_cache(maxsize=None)
def reference(k, j, level):
    """(stream, oracle t_full, oracle t_quarter): made once, shared by the three slice settings, never written to."""
    data = stream(k, j)
    assert len(data) == 5600
    tf, tq = O.match_tables(data, level)
    if level == 6:
        targets = 8 * np.arange(FIRST, LAST + 1)
        dist = tf[targets] & 0xffff
        assert (dist == 8 * j).all(), 'generator: k %d, j %d: %d of 256 targets do not match 8 j back in the oracle (first: record %d, dist %d)' % (
            k, j, int((dist != 8 * j).sum()), FIRST + int(np.argmax(dist != 8 * j)), int(dist[np.argmax(dist != 8 * j)]))
    tf.setflags(write=False)
    tq.setflags(write=False)
    return data, tf, tq


@pytest.mark.parametrize('k', [0, 1, 2, 3])
@pytest.mark.parametrize('env', [None, '1', '64'])
def test_planted_candidates(monkeypatch, env, k):
    """MTS_MATCH_SLICES '1': one workgroup per tile, a wave's ring wraps many times; '64': one group per wave, every group stages
    its history again (the history commits' phases)."""
    if env is None:
        monkeypatch.delenv('MTS_MATCH_SLICES', raising=False)
    else:
        monkeypatch.setenv('MTS_MATCH_SLICES', env)
    for j in BACK:
        for level in LEVELS:
            data, tf, tq = reference(k, j, level)
            gf, gq = hip.debug_match_tables(data, level)
            for label, got, want in (('t_full', gf, tf), ('t_quarter', gq, tq)):
                d = np.nonzero(got != want)[0]
                if d.size:
                    p = int(d[0])
                    raise AssertionError('MTS_MATCH_SLICES=%s, k %d, j %d, level %d, %s: %d wrong, first at %d (record %d + %d): '
                                         'device (len %d, dist %d), oracle (len %d, dist %d)' % (
                                             env, k, j, level, label, d.size, p, p // 8, p % 8,
                                             int(got[p]) >> 16, int(got[p]) & 0xffff, int(want[p]) >> 16, int(want[p]) & 0xffff))
