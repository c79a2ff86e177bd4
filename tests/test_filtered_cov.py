"""Reader.cov with taps= / reference=, host side, on the oracle codec of tests/filtered_gram_oracle.py: the results against
gram_oracle.check_cov_result on the oracle's z, the untouched unfiltered path, the halo feed (every part's chunks adjacent and covering
its support), bit-identity across lanes and call budgets, windows stitched across call cuts, detect's argument errors, damaged chunks
and cache use.  The kernel: tests/test_gpu_filtered_gram.py."""
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.detect_oracle import DetectOracleCodec
from tests.filtered_gram_oracle import FilteredGramOracleCodec, call_rows
from tests.filtered_select_oracle import support, z_rows
from tests.gram_oracle import GramOracleCodec, check_cov_result

ROOT = Path(__file__).resolve().parent.parent
HP = api.highpass_taps(300, 30000, 21)


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _write(tmp, arr, codec, **kw):
    raw = tmp / 'data.bin'
    arr.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'data.cbin', tmp / 'data.ch', sample_rate=1000., n_channels=arr.shape[1], dtype=arr.dtype,
                         chunk_duration=1., codec=codec, check_after_compress=False, **kw)
    return mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', codec=codec, check_after_decompress=False)


def _recording(rows=4500, nc=6, seed=0, dtype='int16'):
    rs = np.random.RandomState(seed)
    x = rs.randn(rows, nc) * 300 + rs.randn(nc) * 1000 + 500 * np.sin(np.arange(rows) / 40.)[:, None]
    return x.astype(dtype)


def _cols(channels, nc):
    if isinstance(channels, (int, np.integer)):
        return [int(channels) % nc]
    if isinstance(channels, slice):
        return list(range(*channels.indices(nc)))
    return [int(c) % nc for c in channels]


def _z(x, cols, taps, reference):
    """The oracle's z of the whole recording x over the columns `cols`."""
    return z_rows(x[:, cols], 0, 0, x.shape[0], 0, x.shape[0], [1.0] if taps is None else taps, 1 if reference else 0)


def _check(r, x, start, stop, window, channels, taps, reference, ddof=1):
    cols = _cols(channels, x.shape[1])
    i0, i1 = r._row_range(start, stop)
    got = r.cov(start, stop, channels=channels, window=window, ddof=ddof, taps=taps, reference=reference)
    assert got.gram.dtype == np.float64 and got.sum.dtype == np.float64 and got.count.dtype == np.int64
    assert got.reference == reference and got.taps.dtype == np.float64 and got.taps.tolist() == ([1.0] if taps is None else list(taps))
    w = window or max(i1 - i0, 1)
    assert (got.start, got.stop, got.window) == (i0, i1, w) and got.channels.tolist() == cols
    check_cov_result(got, _z(x, cols, taps, reference), i0, i1, window, ddof=ddof)
    return got


def test_results_within_the_bound_of_the_oracles_z(tmp_cfg):
    x = _recording(rows=4500, nc=6, seed=1)
    r = _write(tmp_cfg, x, FilteredGramOracleCodec(n_lanes=2, capacity_chunks=8))
    for taps, reference in ((HP, 'median'), (None, 'median'), ([0.5, 0.5], None), (HP, None)):
        for window in (None, 7, 1000, 3001):
            for channels in (slice(None), [5, 0, 2, 2, 1]):
                start, stop = (995, 1030) if window == 7 else (10, -3)
                _check(r, x, start, stop, window, channels, taps, reference, ddof=0 if window == 1000 else 1)
    one = _check(r, x, 0, None, 1500, 3, HP, None)                     # an int channel: C = 1, nothing squeezed
    assert one.gram.shape == (3, 1, 1)
    # no rows, no channels: no call
    n_calls = len(r.codec.filtered_gram_calls)
    assert r.cov(100, 100, taps=HP).gram.shape == (0, 6, 6)
    e = r.cov(channels=[], window=1000, taps=HP, reference='median')
    assert e.gram.shape == (5, 0, 0) and e.count.tolist() == [1000, 1000, 1000, 1000, 500] and e.reference == 'median'
    assert len(r.codec.filtered_gram_calls) == n_calls
    assert not r.codec.gram_calls                                      # the filtered path makes no gram call
    # with the median reference the result depends on the column set; without one it does not
    a = r.cov(channels=[0, 1, 2], taps=HP, reference='median').gram[0, :2, :2]
    b = r.cov(channels=[0, 1], taps=HP, reference='median').gram[0]
    assert a.tobytes() != b.tobytes()
    a = r.cov(channels=[0, 1, 2], taps=HP).gram[0, :2, :2]
    assert np.allclose(a, r.cov(channels=[0, 1], taps=HP).gram[0], rtol=1e-12)
    r.close()


def test_nan_poisons_the_window_with_the_median_reference(tmp_cfg):
    rs = np.random.RandomState(4)
    x = (rs.randn(2400, 5) * 10).astype(np.float32)
    x[100, 1] = np.nan
    r = _write(tmp_cfg, x, FilteredGramOracleCodec(n_lanes=2, capacity_chunks=8), do_time_diff=False)
    got = r.cov(window=700, reference='median')
    assert np.isnan(got.gram[0]).all() and np.isnan(got.cov[0]).all() and np.isfinite(got.gram[1:]).all()
    plain = r.cov(window=700, taps=[1.0])
    assert np.isnan(plain.gram[0][1]).all() and np.isnan(plain.gram[0][:, 1]).all()
    assert np.isfinite(plain.gram[0][[0, 2, 3, 4]][:, [0, 2, 3, 4]]).all() and np.isfinite(plain.gram[1:]).all()
    r.close()


def test_unfiltered_calls_are_what_they_were(tmp_cfg):
    """With both arguments None: the codec's gram is called with the arguments the commit before taps= / reference= passed, and a
    codec without filtered_gram serves it."""
    x = _recording(rows=5200, nc=4, seed=5)
    r = _write(tmp_cfg, x, FilteredGramOracleCodec(n_lanes=2, capacity_chunks=8))
    ref = _write(tmp_cfg, x, GramOracleCodec(n_lanes=2, capacity_chunks=8))
    seen = []
    keep = FilteredGramOracleCodec.gram

    def spy(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, *args, lane=None):
        seen.append((lane, list(keys), list(row0), list(lens), list(n_rows), n_channels, np.dtype(dtype), flags) + tuple(
            a.tolist() if isinstance(a, np.ndarray) else a for a in args))
        return keep(self, cache_id, keys, row0, cdata, offs, lens, n_rows, n_channels, dtype, flags, *args, lane=lane)
    r.codec.gram = spy.__get__(r.codec)
    for kw in (dict(), dict(start=7, stop=-9, window=1700), dict(channels=[2, 0], window=2500, ddof=0), dict(taps=None, reference=None)):
        a, b = r.cov(**kw), ref.cov(**kw)
        for k in ('count', 'sum', 'gram', 'mean', 'cov'):
            assert a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype
        assert a.gram.dtype == np.int64 and 'taps' not in a and 'reference' not in a
    assert sorted(c[:5] for c in r.codec.gram_calls) == sorted(c[:5] for c in ref.codec.gram_calls) and r.codec.gram_calls
    assert not r.codec.filtered_gram_calls
    # the arguments: (range_begin, range_end, window_rows, group_begin, group_end, cols) after the chunk table, for the chunks of the
    # groups' own rows
    assert [(c[1], c[8:]) for c in seen if c[8:11] == (0, 5200, 5200)] == [([0, 1, 2, 3, 4, 5], (0, 5200, 5200, 0, 1, [0, 1, 2, 3]))] * 2
    for c in seen:
        rb, re_, w, g0, g1 = c[8:13]
        lo, hi = call_rows(rb, re_, w, g0, g1)
        assert c[1] == list(range(lo // 1000, (hi - 1) // 1000 + 1)) and len(c) == 14
    # ... and the calls (lane, keys, row0, lens, rows, n_channels, dtype, flags, the op's arguments) are those that the commit before
    # taps= / reference= made
    digest = hashlib.sha256(repr(sorted((c[:6] + (str(c[6]),) + c[7:] for c in seen), key=repr)).encode()).hexdigest()
    assert digest == 'dfc160fcb7c93f7a112b742bbd9df70f087caa978eee964ed7902fab86fb56e5', sorted(seen, key=repr)
    with pytest.raises(NotImplementedError, match='filtered'):
        ref.cov(taps=HP)
    r.close()
    ref.close()


def test_parts_cover_their_support_and_are_adjacent(tmp_cfg, monkeypatch):
    """(the oracle codec asserts adjacency and cover in every call; here: what was called, with what)"""
    x = _recording(rows=6400, nc=5, seed=6)
    codec = FilteredGramOracleCodec(n_lanes=3, capacity_chunks=8)
    r = _write(tmp_cfg, x, codec)
    monkeypatch.setattr(api, 'GRAM_CALL_BYTES', 1)                      # a cut after every group
    r.cov(1234, 5678, window=700, taps=HP, reference='median')
    groups = sorted((c[6], c[7]) for c in codec.filtered_gram_calls)
    assert groups[0][0] == 0 and groups[-1][1] == 7 and all(a[1] == b[0] for a, b in zip(groups[:-1], groups[1:]))
    for lane, keys, lens, rb, re_, w, g0, g1 in codec.filtered_gram_calls:
        assert (rb, re_, w) == (1234, 5678, 700)
        lo, hi = support(*call_rows(rb, re_, w, g0, g1), len(HP), 0, 6400)
        assert keys == list(range(lo // 1000, (hi - 1) // 1000 + 1))    # exactly the chunks of the support
    # rows of chunk 2 alone: the 10 rows either side that 21 taps read do not leave it, the 20 of 41 taps do
    codec.filtered_gram_calls.clear()
    r.cov(2010, 2990, taps=HP)
    assert [c[1] for c in codec.filtered_gram_calls] == [[2]]
    codec.filtered_gram_calls.clear()
    r.cov(2010, 2990, taps=api.highpass_taps(300, 30000, 41))
    assert [c[1] for c in codec.filtered_gram_calls] == [[1, 2, 3]]
    codec.filtered_gram_calls.clear()
    monkeypatch.setattr(api, 'GRAM_CALL_BYTES', 1 << 30)
    r.cov(window=700, taps=HP)                                          # 10 groups over three lanes
    assert {c[0] for c in codec.filtered_gram_calls} == {0, 1, 2}
    r.close()


def _flat(r):
    res = [r.cov(7, -9, window=w, taps=HP, reference='median') for w in (None, 2500, 300)]
    res.append(r.cov(7, -9, window=2500, taps=[0.5, 0.5]))
    return b''.join(a[k].tobytes() for a in res for k in ('count', 'sum', 'gram', 'mean', 'cov'))


def test_same_bits_from_any_lanes_and_call_budgets(tmp_cfg, monkeypatch):
    x = _recording(rows=6400, nc=5, seed=7)
    base = None
    for lanes in (1, 2, 3):
        codec = FilteredGramOracleCodec(n_lanes=lanes, capacity_chunks=8)
        r = _write(tmp_cfg, x, codec)
        flat = _flat(r)
        base = base or flat
        assert flat == base
        assert {c[0] for c in codec.filtered_gram_calls} == set(range(lanes))
        if lanes == 2:
            n_calls = len(codec.filtered_gram_calls)
            monkeypatch.setattr(api, 'GRAM_CALL_BYTES', 1)              # a small call budget: a call per group
            assert _flat(r) == base
            assert len(codec.filtered_gram_calls) - n_calls > n_calls
            monkeypatch.setattr(api, 'GRAM_CALL_BYTES', 1 << 30)
            monkeypatch.setattr(api, 'GRAM_SLAB_BYTES', 1)              # a small result budget: one group a call
            n_calls = len(codec.filtered_gram_calls)
            assert _flat(r) == base
            assert all(c[7] - c[6] == 1 for c in codec.filtered_gram_calls[n_calls:])
            monkeypatch.setattr(api, 'GRAM_SLAB_BYTES', 1 << 30)
        r.close()


def test_windows_stitch_across_call_cuts(tmp_cfg, monkeypatch):
    """A window of more than one group (the group length cut down to 512 rows), every group a call of its own."""
    x = _recording(rows=5000, nc=3, seed=8)
    r = _write(tmp_cfg, x, FilteredGramOracleCodec(n_lanes=2, capacity_chunks=8))
    whole = [r.cov(a, b, window=w, taps=HP, reference='median') for a, b, w in ((0, 5000, None), (999, 3001, 1000), (1, 4999, 1999))]
    monkeypatch.setattr(hip, 'GRAM_GROUP_ROWS', 512)
    monkeypatch.setattr(api, 'GRAM_CALL_BYTES', 1)
    z = _z(x, [0, 1, 2], HP, 'median')
    for (a, b, w), one in zip(((0, 5000, None), (999, 3001, 1000), (1, 4999, 1999)), whole):
        n_calls = len(r.codec.filtered_gram_calls)
        got = r.cov(a, b, window=w, taps=HP, reference='median')
        assert len(r.codec.filtered_gram_calls) - n_calls == hip.gram_groups(a, b, w or 5000) > len(got.count)
        assert got.count.tolist() == one.count.tolist()
        assert np.allclose(got.gram, one.gram, rtol=1e-12, atol=0) and np.allclose(got.sum, one.sum, rtol=1e-9, atol=1e-6)
        for k in range(len(got.count)):                                 # the groups of a window added in order, from the oracle's partials
            lo = a + k * (w or 5000)
            zz = z[lo:min(lo + (w or 5000), b)].astype(np.float64)
            want = np.zeros((3, 3))
            for g in range(0, len(zz), 512):
                want = want + zz[g:g + 512].T @ zz[g:g + 512]
            assert np.allclose(got.gram[k], want, rtol=1e-12, atol=0)
    r.close()


class _WithDetect(FilteredGramOracleCodec, DetectOracleCodec):
    """Both ops, so that one Reader gives detect's message and cov's."""


def test_argument_errors_carry_detects_messages(tmp_cfg):
    x = _recording(rows=2000, nc=4, seed=9)
    r = _write(tmp_cfg, x, _WithDetect(n_lanes=1, capacity_chunks=8))

    def message(call):
        with pytest.raises(ValueError) as e:
            call()
        return str(e.value)
    for bad_kw in (dict(reference='mean'), dict(reference=1), dict(taps=[]), dict(taps=[1.0, np.nan]), dict(taps=np.ones(8193)),
                   dict(taps=[[1.0]]), dict(taps='a')):
        assert message(lambda: r.cov(**bad_kw)) == message(lambda: r.detect(5.0, **bad_kw))
    wide = _write(tmp_cfg, np.zeros((10, 1025), np.int16), _WithDetect(n_lanes=1, capacity_chunks=8))
    want = message(lambda: wide.detect(5.0, reference='median'))
    assert '1024' in want and message(lambda: wide.cov(reference='median')) == want
    assert wide.cov(reference='median', channels=slice(0, 1024)).gram.shape == (1, 1024, 1024)
    assert wide.cov(taps=[1.0]).gram.shape == (1, 1025, 1025)          # without a reference: mts_gram's limit
    wide.close()
    # the other arguments are checked as before
    for call in (lambda: r.cov(window=0, taps=HP), lambda: r.cov(ddof=-1, taps=HP), lambda: r.cov(ddof=1.5, reference='median'),
                 lambda: r.cov(channels=slice(None, None, -1), taps=HP)):
        message(call)
    with pytest.raises(IndexError):
        r.cov(channels=4, taps=HP)
    assert not r.codec.filtered_gram_calls
    r.close()


def test_cache_use_no_insertion_miss_retry_and_damage(tmp_cfg):
    x = _recording(rows=5200, nc=4, seed=10)
    codec = FilteredGramOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, x, codec)
    kw = dict(window=1700, taps=HP, reference='median')
    cold = r.cov(**kw)
    assert all(not c for c in codec.caches.values())                # a scan inserts nothing
    assert all(all(n > 0 for n in c[2]) for c in codec.filtered_gram_calls)
    r[1005:1010]
    r[2005:2010]                                                    # chunks 1 and 2 resident, on lanes 1 and 0
    before = {cid: sorted(c) for cid, c in codec.caches.items()}
    n_calls = len(codec.filtered_gram_calls)
    assert r.cov(**kw).gram.tobytes() == cold.gram.tobytes()
    assert {cid: sorted(c) for cid, c in codec.caches.items()} == before
    assert any(0 in c[2] for c in codec.filtered_gram_calls[n_calls:])   # some resident chunk went without bytes
    codec.miss_next_filtered_gram = True                            # an entry dropped between the query and the call: sent whole once more
    assert r.cov(**kw).gram.tobytes() == cold.gram.tobytes()
    r.close()
    # a damaged chunk in the support: the IOError of Reader[...]
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    o = r.chunk_offsets
    data[o[3] + 20:o[3] + 40] = b'\x00' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=FilteredGramOracleCodec(n_lanes=2, capacity_chunks=8),
                               check_after_decompress=False)
    for call in (lambda: r.cov(taps=HP), lambda: r.cov(window=500, taps=HP), lambda: r.cov(window=1700, reference='median'),
                 lambda: r.cov(2995, 3000, taps=HP), lambda: r.cov(3995, 4005, taps=HP)):      # (2995 .. 3000: chunk 3 in the halo only)
        with pytest.raises(IOError, match='#3'):
            call()
    check_cov_result(r.cov(0, 2980, taps=HP), _z(x, [0, 1, 2, 3], HP, None), 0, 2980, None)
    r.close()


def test_exports_are_listed_and_declared():
    names = {'mts_filtered_gram', 'mts_dev_filtered_gram'}
    assert names <= set(hip.EXPORTS)
    assert callable(api.HipCodec.filtered_gram) and callable(hip.filtered_gram) and callable(hip.dev_filtered_gram)
    header = (ROOT / 'include' / 'mtscomp_hip.h').read_text()
    assert names <= set(re.findall(r'\b(mts_[a-z0-9_]+)\s*\(', header))
    L = hip.lib()
    assert all(hasattr(L, n) for n in names)
    import inspect
    assert list(inspect.signature(api.Reader.cov).parameters)[1:] == ['start', 'stop', 'channels', 'window', 'ddof', 'taps', 'reference']
