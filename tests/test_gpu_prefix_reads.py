"""mts_cache_read_slices_leading against numpy on the catalogue of tests/prefix_cases.py (certified device-free by
tests/test_prefix_cases.py): the chain walk that stops early (InfChunk::n_need), the inverse transform with nc = n_leading on a
stream laid out for 130 channels, and the (rows, n_leading) cache entries.  All comparisons are exact.

Every prefix call works on a POISONED engine -- a different whole chunk of the same shape has just been decoded through it, so
the stream and token buffers hold plausible wrong bytes behind what the prefix decode writes -- and on a fresh key.

S1 safety      any truncation of an intact chunk gives E_MISS or the right bytes, never a wrong answer or a per-chunk verdict
S2 liveness    L = len(z) and L = L_min + PREFIX_SLACK_BYTES succeed for what the project's encoder and zlib level 1 / 6 / 9 write
S3             streams the fast path cannot follow: E_MISS or right with n_leading, right without, right through the Reader
S4             the wanted prefix ends inside the FINAL block: len(z) succeeds, len(z) - 1 .. 4 succeed or miss
S5             four chunks of mixed residency in one call; S6 refusals; S7 the Reader on every integer type, lanes, small cache
"""
import ctypes as C
import itertools
import json
import zlib

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests import prefix_cases as P
from tests.deflate_shape import blocks

pytestmark = pytest.mark.gpu

# Bytes behind L_min (the byte that holds the last bit of the block that completes the prefix) a prefix decode needs before it
# answers: 0 -- the header's "whole deflate blocks" holds to the byte.  Reader._lane_read_slices adds 32768 to its estimate.
PREFIX_SLACK_BYTES = 0
LIVE = ('zlib1', 'zlib6', 'zlib9', 'full', 'device')
MISS = 'miss'
_key = itertools.count(1000)


def poison(case):
    if case.rows:
        st, _ = hip.decompress_chunks([P.poison(case.dtype.name, case.rows)], [case.rows], P.NC, case.dtype, P.FLAGS[0])
        assert st == [0]


def requests(case, k):
    """The whole (R, k) rectangle and a strided one that ends at column k."""
    return [(0, case.rows, 1, 0, k, 1), (min(1, case.rows), case.rows, 3, (k - 1) % 2, k, 2)]


def read_prefix(cid, case, k, length, key=None, reqs=None, poisoned=True):
    """One call with the first `length` bytes of the chunk: MISS, or (status, arrays)."""
    if poisoned:
        poison(case)
    try:
        st, got = hip.cache_read_slices(cid, [next(_key) if key is None else key], case.z[:length], [0], [length], [case.rows], P.NC,
                                        case.dtype, case.flags, reqs or requests(case, k), n_leading=k)
    except hip.HipError as e:
        assert e.code == hip.E_MISS, (case, k, length, e)
        return MISS
    return st[0], got


def right(case, k, got, reqs=None):
    return all(g.dtype == case.dtype and np.array_equal(g, case.arr[rb:re:rs, cb:ce:cs])
               for g, (rb, re, rs, cb, ce, cs) in zip(got, reqs or requests(case, k)))


def sweep(cid, case, k, lengths=None):
    """S1 for one (case, k): {length: MISS | 'ok'}; anything else fails."""
    out = {}
    for length in lengths or case.lengths(k):
        r = read_prefix(cid, case, k, length)
        if r != MISS:
            assert r[0] == hip.CHUNK_OK, '%s k=%d L=%d (L_min %d, len %d): status %d' % (case, k, length, case.l_min(k), len(case.z), r[0])
            assert right(case, k, r[1]), '%s k=%d L=%d (L_min %d, len %d): wrong bytes' % (case, k, length, case.l_min(k), len(case.z))
        out[length] = MISS if r == MISS else 'ok'
    return out


@pytest.fixture
def cache():
    cid = hip.cache_create(1 << 30)
    yield cid
    hip.cache_destroy(cid)


@pytest.mark.parametrize('case', P.cases(), ids=repr)
def test_s1_s2_truncations_miss_or_are_right(case, cache):
    for k in case.ks:
        got = sweep(cache, case, k)
        first_ok = min([x for x, v in got.items() if v == 'ok'], default=None)
        print('%s k=%d: n_need %d, block %d of %d, L_min %d, len %d, first ok %s' % (case, k, case.n_need(k), case.cover(k), len(case.table),
                                                                                      case.l_min(k), len(case.z), first_ok))
        if case.writer in LIVE:
            assert got[len(case.z)] == 'ok', '%s k=%d: the whole chunk missed' % (case, k)
            assert got[min(case.l_min(k) + PREFIX_SLACK_BYTES, len(case.z))] == 'ok', '%s k=%d: L_min %d missed' % (case, k, case.l_min(k))


DEVICE_CASES = [c for c in P.cases() if c.writer in ('zlib1', 'zlib6', 'zlib9') and c.dtype == np.int16 and c.rows]


@pytest.mark.parametrize('case', DEVICE_CASES, ids=repr)
def test_s2_the_projects_own_encoder(case, cache):
    """Writer (a): the chunk as hip.compress_chunks writes it -- zlib's bytes, or the test ends here -- analysed from the device's bytes."""
    z = hip.compress_chunks(case.arr, [0, case.rows], case.flags, int(case.writer[4:]))[0]
    assert z == case.z
    dev = P.Case('device_' + case.name, case.arr, case.flags, z, case.ks, 'device')
    assert [(b['bit_end'], b['nout']) for b in blocks(np.frombuffer(z, dtype=np.uint8))] == [(t[0], t[3]) for t in dev.table]
    for k in dev.ks:
        lm = dev.l_min(k)
        got = sweep(cache, dev, k, [lm - 2, min(lm + PREFIX_SLACK_BYTES, len(z)), len(z)])
        assert got[len(z)] == 'ok' and got[min(lm + PREFIX_SLACK_BYTES, len(z))] == 'ok', (dev, k, got)


def test_slack_is_below_the_readers_margin():
    assert 0 <= PREFIX_SLACK_BYTES < 32768


HARD = [c for c in P.cases() if c.writer in ('fixed', 'stored', 'sync') or 'fixed_long' in c.name]


def _reader_file(tmp_path, case):
    """A one-chunk file around the case's stream, assembled as in test_partial_reads_check_the_whole_chunk_by_default."""
    raw = tmp_path / 'x.bin'
    case.arr.tofile(raw)
    mtscomp_amd.compress(raw, tmp_path / 'x.cbin', tmp_path / 'x.ch', sample_rate=float(case.rows), n_channels=P.NC, dtype=case.dtype,
                         chunk_duration=1., do_time_diff=bool(case.flags & 1), do_spatial_diff=bool(case.flags & 2), check_after_compress=False)
    hdr = json.loads((tmp_path / 'x.ch').read_text())
    assert len(hdr['chunk_offsets']) == 2
    hdr['chunk_offsets'] = [0, len(case.z)]
    (tmp_path / 'y.cbin').write_bytes(case.z)
    (tmp_path / 'y.ch').write_text(json.dumps(hdr))
    return mtscomp_amd.decompress(tmp_path / 'y.cbin', tmp_path / 'y.ch', partial_decode=True)


@pytest.mark.parametrize('case', HARD, ids=repr)
def test_s3_streams_the_fast_path_cannot_follow(case, cache, tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    for k in case.ks:
        r = read_prefix(cache, case, k, len(case.z))
        assert r == MISS or (r[0] == hip.CHUNK_OK and right(case, k, r[1])), (case, k)
        poison(case)
        whole = [(0, case.rows, 1, 0, P.NC, 1)]
        st, got = hip.cache_read_slices(cache, [next(_key)], case.z, [0], [len(case.z)], [case.rows], P.NC, case.dtype, case.flags, whole)
        assert st == [0] and np.array_equal(got[0], case.arr), (case, k)
    rd = _reader_file(tmp_path, case)
    try:
        for k in case.ks:
            a, b = case.rows // 7, case.rows - 3
            assert np.array_equal(rd[a:b, :k], case.arr[a:b, :k]), (case, k)
    finally:
        rd.close()


FINAL = [(c, k) for c, k in P.pairs() if 'final' in c.classes(k) and c.rows]


def test_s4_the_prefix_ends_inside_the_final_block(cache):
    """A partial decode whose covering block carries BFINAL never looks at the check value: every byte of the chunk is enough,
    and a chunk cut inside its 4-byte trailer is still intact as far as the prefix is concerned (OK or a miss, never CORRUPT)."""
    assert any(c.name == 'i16_63_one_dynamic_block' for c, _ in FINAL) and len({c.name for c, _ in FINAL}) >= 4
    for case, k in FINAL:
        n = len(case.z)
        got = sweep(cache, case, k, [n - d for d in range(5)])
        print('%s k=%d: %s' % (case, k, [got[n - d] for d in range(5)]))
        assert got[n] == 'ok', (case, k)


def _four(seed0=40):
    arrs = [P.signal('int16', 2000, seed0 + i) for i in range(4)]
    zs = [zlib.compress(P.stream_of(a, P.FLAGS[0]), 6) for a in arrs]
    return arrs, zs


def _call(cid, keys, parts, rows, dtype, flags, reqs, k=None):
    lens = [len(p) for p in parts]
    offs = [int(x) for x in np.concatenate(([0], np.cumsum(lens)))[:-1]]
    return hip.cache_read_slices(cid, keys, b''.join(parts), offs, lens, rows, P.NC, dtype, flags, reqs, n_leading=k)


def test_s5_mixed_residency_in_one_call():
    arrs, zs = _four()
    f, k, k_narrow, k_wide, rows = P.FLAGS[0], 16, 3, 64, [2000] * 4
    cold = P.Case('cold', arrs[2], f, zs[2], (k,), 'zlib6')
    narrow = P.Case('narrow', arrs[1], f, zs[1], (k,), 'zlib6')
    allrows = np.concatenate(arrs)
    reqs = [(0, 8000, 1, 0, k, 1), (1500, 6500, 7, 1, k, 3), (1999, 6001, 1, k - 1, k, 1), (3990, 4010, 1, 0, 1, 1)]
    poison_case = cold

    def setup(cid):
        st, _ = _call(cid, [0], [zs[0]], [2000], np.int16, f, [(0, 1, 1, 0, 1, 1)])
        assert st == [0]
        st, _ = _call(cid, [1], [zs[1][:narrow.l_min(k_narrow) + PREFIX_SLACK_BYTES]], [2000], np.int16, f, [(0, 1, 1, 0, 1, 1)], k=k_narrow)
        assert st == [0]
        st, _ = _call(cid, [3], [zs[3]], [2000], np.int16, f, [(0, 1, 1, 0, 1, 1)], k=k_wide)
        assert st == [0]
        assert list(hip.cache_query(cid, [0, 1, 2, 3])) == [P.NC, k_narrow, 0, k_wide]
        poison(poison_case)

    cid = hip.cache_create(1 << 30)
    try:
        setup(cid)
        parts = [b'', zs[1][:narrow.l_min(k) + PREFIX_SLACK_BYTES], zs[2][:cold.l_min(k) + PREFIX_SLACK_BYTES], b'']
        st, got = _call(cid, [0, 1, 2, 3], parts, rows, np.int16, f, reqs, k=k)
        assert st == [0] * 4
        for g, (rb, re, rs, cb, ce, cs) in zip(got, reqs):
            assert np.array_equal(g, allrows[rb:re:rs, cb:ce:cs]), (rb, re, rs, cb, ce, cs)
        held = [P.NC, k, k, k_wide]
        assert list(hip.cache_query(cid, [0, 1, 2, 3])) == held
        for key, cols in enumerate(held):                                   # every entry's content, with no bytes sent
            st, got = _call(cid, [key], [b''], [2000], np.int16, f, [(0, 2000, 1, 0, cols, 1)], k=cols if cols < P.NC else None)
            assert st == [0] and np.array_equal(got[0], arrs[key][:, :cols]), key
    finally:
        hip.cache_destroy(cid)
    cid = hip.cache_create(1 << 30)
    try:
        setup(cid)
        parts = [b'', zs[1][:narrow.l_min(k) + PREFIX_SLACK_BYTES], zs[2][:cold.l_min(k) - 2], b'']
        with pytest.raises(hip.HipError) as e:
            _call(cid, [0, 1, 2, 3], parts, rows, np.int16, f, reqs, k=k)
        assert e.value.code == hip.E_MISS
        st, got = _call(cid, [0, 1, 2, 3], zs, rows, np.int16, f, [(0, 8000, 1, 0, P.NC, 1)])
        assert st == [0] * 4 and np.array_equal(got[0], allrows)            # no entry was left holding wrong data
        assert list(hip.cache_query(cid, [0, 1, 2, 3])) == [P.NC] * 4
    finally:
        hip.cache_destroy(cid)


def _raw_leading(cid, z, rows, nc, itemsize, flags, n_leading, req):
    L = hip.lib()
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_long))  # noqa: E731
    keys, zero, ln, nr = (np.array([v], dtype=np.int64) for v in (next(_key), 0, len(z), rows))
    cdata = np.frombuffer(z + bytes(16), dtype=np.uint8)
    out = np.zeros(1 << 16, dtype=np.uint8)
    status = np.zeros(1, dtype=np.int32)
    rq = np.array(req, dtype=np.int64)
    return L.mts_cache_read_slices_leading(cid, 1, lp(keys), cdata.ctypes.data_as(C.c_void_p), lp(zero), lp(ln), lp(nr), nc, itemsize, flags,
                                           n_leading, 1, lp(rq), out.ctypes.data_as(C.c_void_p), lp(zero), out.size,
                                           status.ctypes.data_as(C.POINTER(C.c_int)))


def test_s6_refusals(cache):
    E_ARG = -1
    a = P.signal('int16', 63, 5)
    f = P.FLAGS[0]
    z = zlib.compress(P.stream_of(a, f), 6)
    req = (0, 10, 1, 0, 3, 1)
    assert _raw_leading(cache, z, 63, P.NC, 2, f, 3, req) == 0                                   # (the call itself is fine)
    assert _raw_leading(cache, z, 63, P.NC, 2, f & ~hip.FLAG_ORDER_F, 3, req) == E_ARG           # order C, leading channels only
    assert _raw_leading(cache, z, 63, P.NC, 4, f | hip.FLAG_FLOAT, 3, req) == E_ARG              # a float dtype
    assert _raw_leading(cache, z, 63, P.NC, 2, f, 0, req) == E_ARG
    assert _raw_leading(cache, z, 63, P.NC, 2, f, P.NC + 1, req) == E_ARG
    assert _raw_leading(cache, z, 63, P.NC, 2, f, 3, (0, 10, 1, 0, 4, 1)) == E_ARG               # columns end past n_leading
    with pytest.raises(hip.HipError) as e:
        hip.cache_read_slices(cache, [next(_key)], z, [0], [len(z)], [63], P.NC, np.float32, f, [req], n_leading=3)
    assert e.value.code == E_ARG
    # a resident entry narrower than asked for, no bytes: a miss that changes nothing
    key = next(_key)
    st, _ = hip.cache_read_slices(cache, [key], z, [0], [len(z)], [63], P.NC, np.int16, f, [req], n_leading=3)
    assert st == [0] and list(hip.cache_query(cache, [key])) == [3]
    with pytest.raises(hip.HipError) as e:
        hip.cache_read_slices(cache, [key], b'', [0], [0], [63], P.NC, np.int16, f, [(0, 10, 1, 0, 4, 1)], n_leading=4)
    assert e.value.code == hip.E_MISS and list(hip.cache_query(cache, [key])) == [3]
    st, got = hip.cache_read_slices(cache, [key], b'', [0], [0], [63], P.NC, np.int16, f, [req], n_leading=3)
    assert st == [0] and np.array_equal(got[0], a[0:10, 0:3])


ROWS_S7 = 3 * 2000 + 63


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """One file per integer dtype: 3 chunks of 2000 rows and one of 63."""
    d = tmp_path_factory.mktemp('prefix_reader')
    out = {}
    for dt in ('uint8', 'int16', 'int32', 'int64'):
        arr = P.signal(dt, ROWS_S7, 21)
        raw = d / (dt + '.bin')
        arr.tofile(raw)
        mtscomp_amd.compress(raw, d / (dt + '.cbin'), d / (dt + '.ch'), sample_rate=2000., n_channels=P.NC, dtype=arr.dtype, chunk_duration=1.,
                             check_after_compress=False)
        out[dt] = (d / (dt + '.cbin'), d / (dt + '.ch'), arr)
    return out


@pytest.mark.parametrize('small_cache', [False, True], ids=['roomy', 'two_entries'])
@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('dt', ['uint8', 'int16', 'int32', 'int64'])
def test_s7_reader_prefix_reads(files, dt, lanes, small_cache, monkeypatch, tmp_path):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    cbin, ch, arr = files[dt]
    entry = (2000 * P.NC * arr.itemsize + 4095) // 4096 * 4096
    capacity = 2 * entry
    if small_cache:
        monkeypatch.setenv('MTSCOMP_DEVICE_CACHE_GB', repr(capacity / 2 ** 30))
    else:
        monkeypatch.delenv('MTSCOMP_DEVICE_CACHE_GB', raising=False)
    codec = api.HipCodec(devices=[0] * lanes) if lanes > 1 else None
    r = mtscomp_amd.decompress(cbin, ch, partial_decode=True, codec=codec)
    rng = np.random.RandomState(100 + lanes + 10 * small_cache)
    try:
        assert r.n_chunks == 4 and (not small_cache or r._dev_cache_bytes == capacity)
        for i in range(40):
            chunk = int(rng.randint(0, 4))
            a = 2000 * chunk + int(rng.randint(0, 40))
            b = min(a + int(rng.randint(1, 2100 if i % 5 == 4 else 1900)), ROWS_S7)
            step = int(rng.choice([1, 1, 3]))
            if i % 3 == 0:
                cols = slice(0, int(rng.choice([1, 2, 3, 16, 63, 64, 65])))          # narrow: a prefix decode
            elif i % 3 == 1:
                cols = slice(int(rng.randint(0, 5)), int(rng.randint(66, P.NC + 1)), int(rng.choice([1, 2])))       # wider: whole chunks
            else:
                cols = slice(None)
            assert np.array_equal(r[a:b:step, cols], arr[a:b:step, cols]), (i, a, b, step, cols)
            if small_cache:
                for cid in (r._dev_caches or []):
                    if cid is None:
                        continue
                    held = hip.cache_query(cid, list(range(4)))
                    used = sum(((r.chunk_bounds[j + 1] - r.chunk_bounds[j]) * int(h) * arr.itemsize + 4095) // 4096 * 4096 for j, h in enumerate(held) if h)
                    assert used <= capacity, (i, list(held))
    finally:
        r.close()
