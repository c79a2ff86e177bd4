"""k_gather_slices (transform.hip) and the decoded-chunk cache under it (cache.hip), through hip.cache_read_slices against numpy.
The compressed chunks come from stdlib zlib over the oracle's transform, so nothing but the inflate, the inverse transform, the
cache and the gather is on the device.  All comparisons are exact.

G1  every item size and kind x row steps {1, 2, 7, more than a chunk} x column steps {1, 2, 5, n_channels}
G2  one launch with an empty, a 1 x 1, a more-than-4096-workgroups and an every-chunk request (the grid is capped: the stride loop runs)
G3  chunk tables of 1, 2 and 40 chunks, zero-row chunks at the front, in the middle and at the end: the kernel's bisection
G4  a failed chunk between two good ones
G5  a cache of two entries under 50 calls that alternate narrow and whole decodes, and one call larger than the cache
"""
import zlib

import numpy as np
import pytest

from mtscomp_amd import hip
from oracle import oracle as O
from tests import prefix_cases as P

pytestmark = pytest.mark.gpu

NC = 67
INT_FLAGS = O.make_flags(True, False, 'F')
FLOAT_FLAGS = O.make_flags(False, False, 'F')


def data(dtype, rows, nc, seed):
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        rs = np.random.RandomState(seed)
        return (rs.randn(rows, nc) * 100 + np.arange(nc)).astype(dtype)
    return P.signal(dtype, rows, seed, nc=nc)


def flags_of(dtype):
    return FLOAT_FLAGS if np.dtype(dtype).kind == 'f' else INT_FLAGS


def pack(arr, bounds, level=6):
    """The chunks arr[bounds[i]:bounds[i + 1]] as zlib streams -> (bytes, offsets, lengths, rows)."""
    f = flags_of(arr.dtype)
    zs = [zlib.compress(P.stream_of(arr[a:b], f), level) for a, b in zip(bounds[:-1], bounds[1:])]
    lens = [len(z) for z in zs]
    offs = [int(x) for x in np.concatenate(([0], np.cumsum(lens)))[:-1]]
    return b''.join(zs), offs, lens, [b - a for a, b in zip(bounds[:-1], bounds[1:])]


def read(cid, keys, packed, arr, reqs, n_leading=None, send=None):
    buf, offs, lens, rows = packed
    if send is not None:
        lens = [n if s else 0 for n, s in zip(lens, send)]
    return hip.cache_read_slices(cid, keys, buf, offs, lens, rows, arr.shape[1], arr.dtype, flags_of(arr.dtype), reqs, n_leading=n_leading)


def check(got, arr, reqs):
    assert len(got) == len(reqs)
    for g, (rb, re, rs, cb, ce, cs) in zip(got, reqs):
        want = arr[rb:re:rs, cb:ce:cs]
        assert g.shape == want.shape and g.dtype == arr.dtype and np.array_equal(g, want), (rb, re, rs, cb, ce, cs)


@pytest.fixture
def cache():
    cid = hip.cache_create(1 << 30)
    yield cid
    hip.cache_destroy(cid)


@pytest.mark.parametrize('dtype', ['uint8', 'int16', 'int32', 'int64', 'float32', 'float64'])
def test_g1_type_and_stride_grid(dtype, cache):
    arr = data(dtype, 4063, NC, 3)
    packed = pack(arr, [0, 2000, 4000, 4063])
    reqs = [(3, 4061, rs, 1, NC, cs) for rs in (1, 2, 7, 2500) for cs in (1, 2, 5, NC)]
    reqs += [(0, 4063, rs, 0, NC, cs) for rs, cs in ((1, 1), (2500, NC))]
    st, got = read(cache, [0, 1, 2], packed, arr, reqs)
    assert st == [0, 0, 0]
    check(got, arr, reqs)
    st, got = read(cache, [0, 1, 2], packed, arr, reqs[::-1], send=[0, 0, 0])          # resident now: no bytes
    assert st == [0, 0, 0]
    check(got, arr, reqs[::-1])


@pytest.mark.parametrize('dtype', ['uint8', 'int64'])
def test_g2_unequal_requests_in_one_launch(dtype, cache):
    rs = np.random.RandomState(5)
    arr = rs.randint(0, 200, size=(2100, 512)).astype(dtype)
    packed = pack(arr, [0, 700, 1400, 2100], level=1)
    reqs = [(5, 5, 1, 0, 512, 1), (2099, 2100, 1, 511, 512, 1), (0, 2100, 1, 0, 512, 1), (699, 1402, 1, 3, 500, 7), (7, 7, 3, 2, 2, 1)]
    assert 2100 * 512 > 4096 * 256
    st, got = read(cache, [0, 1, 2], packed, arr, reqs)
    assert st == [0, 0, 0]
    check(got, arr, reqs)


def _tables():
    rs = np.random.RandomState(8)
    many = [0, 0] + [int(x) for x in rs.choice([1, 2, 63], size=18)] + [0] + [int(x) for x in rs.choice([1, 2, 63, 0], size=17)] + [0, 0]
    assert len(many) == 40 and many.count(0) >= 5
    return {'one': [63], 'two': [2, 63], 'forty': many}


@pytest.mark.parametrize('name', ['one', 'two', 'forty'])
def test_g3_chunk_tables(name, cache):
    rows = _tables()[name]
    bounds = [int(x) for x in np.concatenate(([0], np.cumsum(rows)))]
    arr = data('int16', bounds[-1], NC, 11)
    packed = pack(arr, bounds)
    reqs = [(0, bounds[-1], 1, 0, NC, 1)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        if a == b:
            reqs.append((a, a, 1, 0, NC, 1))                        # an empty request at a zero-row chunk
            continue
        reqs += [(a, a + 1, 1, 0, NC, 1), (b - 1, b, 1, 1, NC, 2), (a, b, 1, 0, NC, 5), (a, bounds[-1], 3, NC - 1, NC, 1), (0, b, 2, 0, 1, 1)]
        if b < bounds[-1]:
            reqs.append((b - 1, b + 1, 1, 0, NC, 1))
    st, got = read(cache, list(range(len(rows))), packed, arr, reqs)
    assert st == [0] * len(rows)
    check(got, arr, reqs)
    assert list(hip.cache_query(cache, list(range(len(rows))))) == [NC] * len(rows)


def test_g4_a_failed_chunk_in_the_middle(cache):
    arr = data('int16', 4063, NC, 13)
    buf, offs, lens, rows = pack(arr, [0, 2000, 4000, 4063])
    bad = bytearray(buf)
    bad[offs[1] + lens[1] // 2] ^= 0x10
    reqs = [(0, 2000, 1, 0, NC, 1), (4000, 4063, 1, 0, NC, 1), (1990, 4010, 1, 0, NC, 1), (1, 4063, 3, 2, NC, 7)]
    st, got = read(cache, [0, 1, 2], (bytes(bad), offs, lens, rows), arr, reqs)
    assert st == [0, hip.CHUNK_CORRUPT, 0]
    assert np.array_equal(got[0], arr[0:2000]) and np.array_equal(got[1], arr[4000:4063])
    assert np.array_equal(got[2][:10], arr[1990:2000]) and np.array_equal(got[2][-10:], arr[4000:4010])
    r = np.arange(1, 4063, 3)
    good = (r < 2000) | (r >= 4000)
    assert np.array_equal(got[3][good], arr[1:4063:3, 2:NC:7][good])
    assert list(hip.cache_query(cache, [0, 1, 2])) == [NC, 0, NC]
    st, got = read(cache, [0, 1, 2], (buf, offs, lens, rows), arr, reqs[2:3])           # the intact bytes: decoded and kept
    assert st == [0, 0, 0] and np.array_equal(got[0], arr[1990:4010])


def test_g5_cache_accounting():
    K = 50                                                           # 3 narrow entries do not fit where 2 whole ones do
    arrs = [data('int16', 2000, NC, 20 + j) for j in range(3)]
    packs = [pack(a, [0, 2000]) for a in arrs]
    whole = (2000 * NC * 2 + 4095) // 4096 * 4096
    narrow = (2000 * K * 2 + 4095) // 4096 * 4096
    capacity = 2 * whole
    assert 3 * narrow > capacity
    cid = hip.cache_create(capacity)
    try:
        visits = [0, 0, 0]
        for i in range(50):
            j = i % 3
            k = K if visits[j] % 2 == 0 else None
            visits[j] += 1
            cols = k or NC
            reqs = [(0, 2000, 1, 0, cols, 1), (i, 2000 - i, 7, cols - 1, cols, 1)]
            st, got = read(cid, [j], packs[j], arrs[j], reqs, n_leading=k)
            assert st == [0]
            check(got, arrs[j], reqs)
            held = list(hip.cache_query(cid, [0, 1, 2]))
            assert held[j] == cols and sum(1 for h in held if h) <= 2, (i, held)
        for j in range(3):
            try:
                st, got = read(cid, [j], packs[j], arrs[j], [(0, 2000, 1, 0, K, 1)], n_leading=K, send=[0])
            except hip.HipError as e:
                assert e.code == hip.E_MISS
                continue
            assert st == [0] and np.array_equal(got[0], arrs[j][:, :K])
        # one call whose chunks alone exceed the capacity: the cache overshoots rather than fails
        buf = b''.join(p[0] for p in packs)
        lens = [p[2][0] for p in packs]
        offs = [0, lens[0], lens[0] + lens[1]]
        allrows = np.concatenate(arrs)
        reqs = [(0, 6000, 1, 0, NC, 1), (1999, 4001, 1, 0, NC, 3)]
        st, got = hip.cache_read_slices(cid, [0, 1, 2], buf, offs, lens, [2000] * 3, NC, np.int16, INT_FLAGS, reqs)
        assert st == [0, 0, 0]
        check(got, allrows, reqs)
        assert sum(1 for h in hip.cache_query(cid, [0, 1, 2]) if h) <= 2
    finally:
        hip.cache_destroy(cid)
