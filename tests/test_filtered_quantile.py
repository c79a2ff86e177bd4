"""Reader.quantile / median / mad with taps= / reference=, host side, on the oracle codec of tests/filtered_select_oracle.py: the results
against np.median / scipy / the sorted z of tests/detect_oracle.py, the untouched unfiltered path, the halo feed (every part's chunks
adjacent and covering its support), bit-identity across lanes and call budgets, windows stitched across call cuts, detect's argument
errors, damaged chunks, cache use and the round cap.  The kernel: tests/test_gpu_filtered_quantile.py."""
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.detect_oracle import DetectOracleCodec
from tests.filtered_select_oracle import FilteredSelectOracleCodec, support, z_rows
from tests.select_oracle import SelectOracleCodec, check_quantile, np_mad, np_median, same_values, scipy_mad

ROOT = Path(__file__).resolve().parent.parent
METHODS = ('linear', 'lower', 'higher', 'nearest', 'midpoint')
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


def _z(x, cols, a, b, taps, reference):
    """The oracle's z of file rows [a, b) over the columns `cols` of the whole recording x."""
    return z_rows(x[:, cols], 0, 0, x.shape[0], a, b, [1.0] if taps is None else taps, 1 if reference else 0)


def _cols(channels, nc):
    if isinstance(channels, (int, np.integer)):
        return [int(channels) % nc]
    if isinstance(channels, slice):
        return list(range(*channels.indices(nc)))
    return [int(c) % nc for c in channels]


def _check(r, x, start, stop, window, channels, taps, reference, q=(0.0, 0.25, 0.5, 0.999, 1.0), methods=('linear',)):
    """quantile, median and mad of the filtered rows against the oracle's z."""
    cols = _cols(channels, x.shape[1])
    i0, i1 = r._row_range(start, stop)
    z = np.zeros((x.shape[0], len(cols)), np.float32)
    z[i0:i1] = _z(x, cols, i0, i1, taps, reference)                    # (rows outside [i0, i1) are never looked at)
    for method in methods:
        got = r.quantile(list(q), start, stop, channels=channels, window=window, method=method, taps=taps, reference=reference)
        assert got.lower.dtype == np.float32 and got.reference == reference
        assert got.taps.dtype == np.float64 and got.taps.tolist() == ([1.0] if taps is None else list(taps))
        check_quantile(got, z, i0, i1, window, q, method)
    med = r.median(start, stop, channels=channels, window=window, taps=taps, reference=reference)
    got = r.mad(start, stop, channels=channels, window=window, taps=taps, reference=reference)
    assert same_values(med, np_median(z, i0, i1, window)) and same_values(got.center, med)
    assert same_values(got.mad, np_mad(z, i0, i1, window))
    zero = r.mad(start, stop, channels=channels, window=window, center=0.0, taps=taps, reference=reference)
    assert same_values(zero.mad, np_mad(z, i0, i1, window, center=0.0)) and zero.reference == reference


def test_filtered_results_equal_the_sorted_z(tmp_cfg):
    x = _recording(rows=4500, nc=6, seed=1)
    r = _write(tmp_cfg, x, FilteredSelectOracleCodec(n_lanes=2, capacity_chunks=8))
    for taps, reference in ((HP, 'median'), (None, 'median'), ([0.5, 0.5], None), (HP, None)):
        for window in (None, 7, 1000, 3001):
            start, stop = (995, 1030) if window == 7 else (10, -3)      # (a cell costs a histogram: few rows for the small window)
            for channels in (slice(None), [5, 0, 2, 2, 1]):
                _check(r, x, start, stop, window, channels, taps, reference, methods=METHODS if window == 1000 else ('linear',))
    # center / absolute order float64(z) - c in 64-bit keys
    cen = np.random.RandomState(2).randn(5, 6) * 50
    z = _z(x, list(range(6)), 0, 4500, HP, 'median')
    for absolute in (False, True):
        got = r.quantile([0, 0.5, 1], window=1000, center=cen, absolute=absolute, taps=HP, reference='median')
        assert got.lower.dtype == np.float64
        check_quantile(got, z, 0, 4500, 1000, [0, 0.5, 1], 'linear', mode=2 if absolute else 1, center=cen)
    # an int channel drops the C axis; no rows, no channels
    one = r.mad(channels=3, window=1500, center=0.0, taps=HP)
    assert one.mad.shape == (3,) and same_values(one.mad[:, None], np_mad(_z(x, [3], 0, 4500, HP, None), 0, 4500, 1500, center=0.0))
    assert r.median(100, 100, taps=HP).shape == (0, 6)
    n_calls = len(r.codec.filtered_calls)
    e = r.quantile([0.1, 0.9], channels=[], window=1000, taps=HP)
    assert e.quantile.shape == (5, 2, 0) and e.rounds == 0 and len(r.codec.filtered_calls) == n_calls
    assert not r.codec.rank_calls                                      # the filtered path makes no rank_hist call
    r.close()


def test_mad_equals_scipy_and_special_floats(tmp_cfg):
    pytest.importorskip('scipy')
    rs = np.random.RandomState(4)
    x = (rs.randn(2400, 7) * 10).astype(np.float32)
    x[100, 1] = np.nan
    x[300, 2], x[450, 3] = np.inf, -np.inf
    x[:, 5] = 0
    x[::2, 5] = -0.0
    x[:, 6] = np.float32(3.25)
    x[7, 4] = np.finfo(np.float32).tiny / 4
    r = _write(tmp_cfg, x, FilteredSelectOracleCodec(n_lanes=2, capacity_chunks=8), do_time_diff=False)
    for reference in (None, 'median'):
        z = _z(x, list(range(7)), 0, 2400, None, reference)
        for window in (None, 700):
            got = r.mad(window=window, reference=reference, taps=[1.0])
            assert same_values(got.mad, scipy_mad(z, 0, 2400, window))
            assert same_values(r.median(window=window, reference=reference, taps=[1.0]), np_median(z, 0, 2400, window))
            check_quantile(r.quantile([0, 0.5, 1], window=window, reference=reference, taps=[1.0]), z, 0, 2400, window, [0, 0.5, 1], 'linear')
    # with the median reference a NaN in a row makes every column's window NaN; without it only its own column's
    assert np.isnan(r.median(0, 700, reference='median')).all()
    plain = r.median(0, 700, taps=[1.0])
    assert np.isnan(plain[0, 1]) and np.isfinite(plain[0, [0, 4, 5, 6]]).all()
    zero = r.quantile(0.5, channels=5, method='lower', taps=[1.0])      # -0 and +0 are one key and come back as +0
    assert zero.lower[0] == 0 and not np.signbit(zero.lower[0])
    r.close()


def test_unfiltered_calls_are_what_they_were(tmp_cfg, monkeypatch):
    x = _recording(rows=5200, nc=4, seed=5)
    r = _write(tmp_cfg, x, FilteredSelectOracleCodec(n_lanes=2, capacity_chunks=8))
    ref = _write(tmp_cfg, x, SelectOracleCodec(n_lanes=2, capacity_chunks=8))         # (a codec without the new entry serves the old path)
    for run in (lambda v: v.quantile([0.1, 0.5], 7, -9, window=1700), lambda v: v.mad(window=2500), lambda v: v.median(3, 4000, channels=[2, 0])):
        a, b = run(r), run(ref)
        for k in ('quantile', 'lower', 'upper', 'mad', 'center', 'count'):
            if isinstance(a, dict) and k in a:
                assert a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype
        if not isinstance(a, dict):
            assert a.tobytes() == b.tobytes()
        assert isinstance(a, np.ndarray) or ('taps' not in a and 'reference' not in a)
    assert sorted(r.codec.rank_calls) == sorted(ref.codec.rank_calls) and r.codec.rank_calls         # (lanes run side by side: any order)
    # ... and the 24 calls (lane, keys, lens, row_begin, row_end, mode) are those that the commit before taps= / reference= made
    digest = hashlib.sha256(repr(sorted(r.codec.rank_calls)).encode()).hexdigest()
    assert digest == '33fa68966fe3e0864d674aaf84c7d94a23bea9e588c575aab877da2febd975bf', sorted(r.codec.rank_calls)
    assert not r.codec.filtered_calls
    with pytest.raises(NotImplementedError, match='filtered'):
        ref.median(taps=HP)
    r.close()
    ref.close()


def test_parts_cover_their_support_and_are_adjacent(tmp_cfg, monkeypatch):
    """(the oracle codec asserts adjacency and cover in every call; here: what was called, with what)"""
    x = _recording(rows=6400, nc=5, seed=6)
    codec = FilteredSelectOracleCodec(n_lanes=3, capacity_chunks=8)
    r = _write(tmp_cfg, x, codec)
    monkeypatch.setattr(api, 'QUANTILE_CALL_BYTES', 1)                  # a cut at every chunk boundary
    got = r.quantile(0.5, 1234, 5678, window=1500, taps=HP, reference='median')
    assert got.rounds >= 1
    first = [c for c in codec.filtered_calls if c[-1] == 0][:len(codec.filtered_calls) // got.rounds]
    counted = sorted((c[5], c[6]) for c in first)
    assert counted[0][0] == 1234 and counted[-1][1] == 5678 and all(a[1] == b[0] for a, b in zip(counted[:-1], counted[1:]))
    for lane, keys, lens, rb, re_, cb, ce, mode in codec.filtered_calls:
        lo, hi = support(cb, ce, len(HP), 0, 6400)
        assert keys == list(range(lo // 1000, (hi - 1) // 1000 + 1))    # exactly the chunks of the support
        assert (rb - 1234) % 1500 == 0 and rb <= cb < ce <= re_ and (re_ == 5678 or (re_ - 1234) % 1500 == 0)
        assert cb - rb < 1500 and re_ - ce < 1500                      # the grid is the windows that the part meets, no more
    assert {c[0] for c in codec.filtered_calls} == {0, 1, 2}
    r.close()


def test_same_bits_from_any_lanes_calls_and_runs(tmp_cfg, monkeypatch):
    x = _recording(rows=6400, nc=5, seed=7)
    base = None
    for lanes in (1, 2, 3):
        codec = FilteredSelectOracleCodec(n_lanes=lanes, capacity_chunks=8)
        r = _write(tmp_cfg, x, codec)

        def results():
            res = [r.quantile([0.2, 0.5], 7, -9, window=w, taps=HP, reference='median') for w in (None, 2500)]
            res += [r.mad(7, -9, window=2500, taps=HP, reference='median'), r.mad(7, -9, window=2500, center=0.0, taps=HP)]
            return b''.join(a[k].tobytes() for a in res for k in ('quantile', 'lower', 'upper', 'mad', 'center', 'count') if k in a)
        flat = results()
        base = base or flat
        assert flat == base
        assert {c[0] for c in codec.filtered_calls} == set(range(lanes))
        if lanes == 2:
            n_calls = len(codec.filtered_calls)
            monkeypatch.setattr(api, 'QUANTILE_CALL_BYTES', 1)         # a small call budget: every window of 2500 rows is split over calls
            assert results() == base
            assert len(codec.filtered_calls) - n_calls > 2 * n_calls
            monkeypatch.setattr(api, 'QUANTILE_CALL_BYTES', 1 << 30)
            monkeypatch.setattr(api, 'QUANTILE_SLAB_BYTES', 1)         # one window per run
            n_calls = len(codec.filtered_calls)
            assert results() == base
            assert {(c[3], c[4]) for c in codec.filtered_calls[n_calls:]} >= {(7, 2507), (2507, 5007), (5007, 6391)}
            monkeypatch.setattr(api, 'QUANTILE_SLAB_BYTES', 1 << 30)
        r.close()


def test_windows_stitch_across_call_cuts(tmp_cfg, monkeypatch):
    x = _recording(rows=5000, nc=3, seed=8)
    r = _write(tmp_cfg, x, FilteredSelectOracleCodec(n_lanes=2, capacity_chunks=8))
    monkeypatch.setattr(api, 'QUANTILE_CALL_BYTES', 1)
    z = _z(x, [0, 1, 2], 0, 5000, HP, 'median')
    for a, b, window in ((0, 5000, None), (999, 3001, 1000), (1000, 4000, 1000), (1, 4999, 1999)):
        got = r.quantile([0.0, 0.5, 1.0], a, b, window=window, taps=HP, reference='median')
        check_quantile(got, z, a, b, window, [0.0, 0.5, 1.0], 'linear')
    r.close()


class _WithDetect(FilteredSelectOracleCodec, DetectOracleCodec):
    """Both ops, so that one Reader gives detect's message and quantile's."""


def test_argument_errors_carry_detects_messages(tmp_cfg):
    x = _recording(rows=2000, nc=4, seed=9)
    r = _write(tmp_cfg, x, _WithDetect(n_lanes=1, capacity_chunks=8))

    def message(call):
        with pytest.raises(ValueError) as e:
            call()
        return str(e.value)
    for bad_kw in (dict(reference='mean'), dict(reference=1), dict(taps=[]), dict(taps=[1.0, np.nan]), dict(taps=np.ones(8193)),
                   dict(taps=[[1.0]]), dict(taps='a')):
        want = message(lambda: r.detect(5.0, **bad_kw))
        for call in (lambda: r.quantile(0.5, **bad_kw), lambda: r.median(**bad_kw), lambda: r.mad(**bad_kw), lambda: r.mad(center=0.0, **bad_kw)):
            assert message(call) == want
    wide = _write(tmp_cfg, np.zeros((10, 1025), np.int16), _WithDetect(n_lanes=1, capacity_chunks=8))
    want = message(lambda: wide.detect(5.0, reference='median'))
    assert '1024' in want and message(lambda: wide.median(reference='median')) == want
    assert wide.median(reference='median', channels=slice(0, 1024)).shape == (1, 1024)
    wide.close()
    # the other arguments are checked as before
    for call in (lambda: r.quantile(1.5, taps=HP), lambda: r.quantile(0.5, window=0, taps=HP), lambda: r.quantile(0.5, method='x', taps=HP),
                 lambda: r.mad(center='mean', taps=HP), lambda: r.quantile(0.5, center=np.zeros((2, 3)), taps=HP)):
        message(call)
    with pytest.raises(IndexError):
        r.median(channels=4, taps=HP)
    assert not r.codec.filtered_calls
    r.close()


def test_cache_use_no_insertion_miss_retry_and_damage(tmp_cfg):
    x = _recording(rows=5200, nc=4, seed=10)
    codec = FilteredSelectOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, x, codec)
    kw = dict(window=1700, taps=HP, reference='median')
    cold = r.median(**kw)
    assert all(not c for c in codec.caches.values())                # a scan inserts nothing
    assert all(all(n > 0 for n in c[2]) for c in codec.filtered_calls)
    r[1005:1010]
    r[2005:2010]                                                    # chunks 1 and 2 resident, on lanes 1 and 0
    before = {cid: sorted(c) for cid, c in codec.caches.items()}
    n_calls = len(codec.filtered_calls)
    assert r.median(**kw).tobytes() == cold.tobytes()
    assert {cid: sorted(c) for cid, c in codec.caches.items()} == before
    assert any(0 in c[2] for c in codec.filtered_calls[n_calls:])   # some resident chunk went without bytes
    codec.miss_next_filtered_rank_hist = True                       # an entry dropped between the query and the call: sent whole once more
    assert r.median(**kw).tobytes() == cold.tobytes()
    r.close()
    # a damaged chunk in the support: the IOError of Reader[...]
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    o = r.chunk_offsets
    data[o[3] + 20:o[3] + 40] = b'\x00' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=FilteredSelectOracleCodec(n_lanes=2, capacity_chunks=8),
                               check_after_decompress=False)
    for call in (lambda: r.median(taps=HP), lambda: r.quantile(0.9, window=500, taps=HP), lambda: r.mad(window=1700, reference='median'),
                 lambda: r.median(2995, 3000, taps=HP), lambda: r.median(3995, 4005, taps=HP)):      # (the last two: chunk 3 in the halo only)
        with pytest.raises(IOError, match='#3'):
            call()
    assert same_values(r.median(0, 2980, taps=HP), np_median(_z(x, [0, 1, 2, 3], 0, 2980, HP, None), 0, 2980, None))
    r.close()


def test_round_cap(tmp_cfg):
    """At most ceil(key_bits / 8) rounds per scan of two ranks: 4 in mode 0 (float32 keys), 8 in modes 1 and 2."""
    x = _recording(rows=2048, nc=3, seed=11)
    x[:, 0] = (np.arange(2048) * 31).astype(np.int16)                   # spread over the type
    codec = FilteredSelectOracleCodec(n_lanes=1, capacity_chunks=8)
    r = _write(tmp_cfg, x, codec)

    def rounds_of(run):
        n = len(codec.filtered_calls)
        got = run()
        assert got.rounds == len(codec.filtered_calls) - n          # (one lane, one call per round here)
        return got.rounds
    for kw in (dict(taps=HP, reference='median'), dict(taps=[1.0]), dict(reference='median')):
        assert 1 <= rounds_of(lambda: r.quantile(0.5, method='midpoint', **kw)) <= 4
        assert 1 <= rounds_of(lambda: r.quantile(0.5, center=0.25, **kw)) <= 8
        assert 1 <= rounds_of(lambda: r.quantile(0.5, center=0.25, absolute=True, **kw)) <= 8
        assert rounds_of(lambda: r.quantile([0.1, 0.5, 0.9], **kw)) <= 3 * 4
        assert rounds_of(lambda: r.mad(**kw)) <= 4 + 8
    r.close()
    r = _write(tmp_cfg, np.full((500, 2), 7, np.int16), FilteredSelectOracleCodec(n_lanes=1, capacity_chunks=8))
    got = r.quantile(0.5, method='midpoint', taps=[1.0])
    assert (got.quantile == 7).all() and got.rounds == 1            # kmin == kmax: resolved by the first round
    r.close()


def test_exports_are_listed_and_declared():
    names = {'mts_filtered_rank_hist', 'mts_dev_filtered_rank_hist'}
    assert names <= set(hip.EXPORTS)
    assert callable(api.HipCodec.filtered_rank_hist) and callable(hip.filtered_rank_hist) and callable(hip.dev_filtered_rank_hist)
    header = (ROOT / 'include' / 'mtscomp_hip.h').read_text()
    assert names <= set(re.findall(r'\b(mts_[a-z0-9_]+)\s*\(', header))
    common = (ROOT / 'mtscomp_amd' / 'csrc' / 'common.h').read_text()
    assert re.search(r'ZSEL_BLOCK_ROWS = %d;' % hip.ZRANK_BLOCK_ROWS, common)
    L = hip.lib()
    assert all(hasattr(L, n) for n in names)
