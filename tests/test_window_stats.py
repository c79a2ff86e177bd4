"""Reader.window_stats, host side: argument handling, result dtypes, lane combination, use of the decoded-chunk cache and errors,
driven through a numpy restatement of mts_window_stats (tests/stats_oracle.py) and compared with numpy over the decoded array.
The device kernels themselves: tests/test_gpu_window_stats.py."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api
from tests.codec_oracle import OracleCodec
from tests.stats_oracle import StatsOracleCodec, assert_stats_equal, numpy_window_stats


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _write(tmp, arr, codec, sample_rate=1000.):
    raw = tmp / 'data.bin'
    arr.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'data.cbin', tmp / 'data.ch', sample_rate=sample_rate, n_channels=arr.shape[1], dtype=arr.dtype,
                         codec=codec, check_after_compress=False)
    return mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', codec=codec, check_after_decompress=False)


def _recording(dtype, rows=4500, nc=6, seed=0):
    rs = np.random.RandomState(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        return (rs.randn(rows, nc) * 100).astype(dtype)
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max, size=(rows, nc), dtype=np.int64 if dtype != np.uint64 else np.uint64).astype(dtype) \
        if dtype.itemsize < 8 else rs.randint(-2 ** 62 if dtype.kind == 'i' else 0, 2 ** 62, size=(rows, nc), dtype=np.int64).astype(dtype)


def _decoded(tmp):
    """The recording as a Reader of its own decodes it (for floats diff + cumsum is not the identity: not the input itself)."""
    r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', codec=OracleCodec(), check_after_decompress=False)
    out = r[:]
    r.close()
    return out


def _check(r, arr, window, start=0, stop=None, channels=slice(None), decoded=None):
    """r.window_stats against numpy over the decoded array."""
    got = r.window_stats(window, start=start, stop=stop, channels=channels)
    arr = r[:] if decoded is None else decoded
    i0 = r._validate_index(start, 0)
    i1 = max(i0, r._validate_index(stop, r.n_samples))
    w = max(i1 - i0, 1) if window is None else window
    if isinstance(channels, (int, np.integer)):
        cols, squeeze = [channels % arr.shape[1]], True
    elif isinstance(channels, slice):
        cols, squeeze = list(range(*channels.indices(arr.shape[1]))), False
    else:
        cols, squeeze = [c % arr.shape[1] for c in channels], False
    want = numpy_window_stats(arr, w, i0, i1, cols)
    assert_stats_equal(got, want, arr.dtype, squeeze=squeeze)
    assert got.start == i0 and got.stop == i1 and got.window == w and list(got.channels) == cols
    return got


@pytest.mark.parametrize('dtype', ['int16', 'uint8', 'int8', 'uint16', 'int32', 'uint32', 'int64', 'float32', 'float64'])
def test_window_stats_every_dtype(tmp_cfg, dtype):
    arr = _recording(dtype)
    codec = StatsOracleCodec(n_lanes=1, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    assert r.n_chunks == 5
    for window in (1, 7, 1000, 3001, 10 ** 6, None):
        _check(r, arr, window)
    r.close()


def test_window_stats_arguments(tmp_cfg):
    arr = _recording('int16', rows=3500)
    codec = StatsOracleCodec(n_lanes=1, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    for start, stop in [(None, None), (-1200, None), (100, -100), (250, 2750), (-10 ** 6, 10 ** 6), (3499, 3500), (0, 1)]:
        for window in (1, 333, None):
            _check(r, arr, window, start, stop)
    for channels in (0, -1, 5, slice(1, None, 2), slice(None, None, 3), slice(4, 2), [3, 1, 1, -2, 0], np.array([5, 5]), []):
        _check(r, arr, 500, 100, 3000, channels)
    # empty ranges: zero windows, shapes (0, n_cols)
    for start, stop in [(2000, 1000), (3500, None), (100, 100)]:
        s = r.window_stats(10, start, stop)
        assert s.count.shape == (0,) and s.min.shape == (0, 6) and s.mean.shape == (0, 6) and s.min.dtype == np.int16
    s = r.window_stats(10, 5, 5, channels=2)
    assert s.min.shape == (0,)
    # a window longer than the range: one window
    s = r.window_stats(10 ** 9, 10, 20)
    assert s.count.tolist() == [10]
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            r.window_stats(bad)
    with pytest.raises(ValueError):
        r.window_stats(10, channels=slice(None, None, -1))
    for bad in (6, -7, [0, 6], [-7], np.array([[0, 1]]), [0.5]):
        with pytest.raises(IndexError):
            r.window_stats(10, channels=bad)
    r.close()


@pytest.mark.parametrize('n_lanes', [2, 3])
def test_window_stats_lanes_equal_one_lane(tmp_cfg, n_lanes):
    arr = _recording('float32', rows=7000, nc=5, seed=3)
    arr[1234, 2] = np.nan
    one = _write(tmp_cfg, arr, StatsOracleCodec(n_lanes=1, capacity_chunks=8))
    codec = StatsOracleCodec(n_lanes=n_lanes, capacity_chunks=8)
    many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    for window in (1000, 777, None):
        a, b = one.window_stats(window, 10, 6990), _check(many, arr, window, 10, 6990)
        for key in ('count', 'min', 'max', 'sum', 'sumsq', 'mean', 'rms'):
            assert np.allclose(a[key], b[key], rtol=1e-13, equal_nan=True)
    lanes_used = {lane for lane, _, _ in codec.stats_calls}
    assert lanes_used == set(range(n_lanes))
    for lane, keys, _ in codec.stats_calls:                      # chunk k on lane k mod lanes, nowhere else
        assert all(k % n_lanes == lane for k in keys)
    ints = _recording('int16', rows=7000, nc=5, seed=4)
    (tmp_cfg / 'i').mkdir()
    r1 = _write(tmp_cfg / 'i', ints, StatsOracleCodec(n_lanes=1, capacity_chunks=8))
    rn = mtscomp_amd.decompress(tmp_cfg / 'i' / 'data.cbin', tmp_cfg / 'i' / 'data.ch', codec=StatsOracleCodec(n_lanes=n_lanes),
                                check_after_decompress=False)
    a, b = r1.window_stats(999), rn.window_stats(999)
    for key in ('count', 'min', 'max', 'sum', 'sumsq', 'mean', 'rms'):
        assert np.array_equal(a[key], b[key]), key


def test_window_stats_long_range_is_split(tmp_cfg, monkeypatch):
    arr = _recording('int16', rows=9000, nc=4, seed=5)
    codec = StatsOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    monkeypatch.setattr(api, 'WINDOW_STATS_CALL_BYTES', 1)       # one chunk per call: windows across calls are combined
    for window in (1300, 2500, None):
        codec.stats_calls.clear()
        _check(r, arr, window, 500, 8700)
        assert len(codec.stats_calls) == 9
    r.close()


def test_window_stats_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    arr = _recording('int16', rows=6000, nc=4, seed=6)
    codec = StatsOracleCodec(n_lanes=1, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    dec = _decoded(tmp_cfg)
    cache = r._cache_for(0)
    assert not codec.caches[cache]
    _check(r, arr, 1000, decoded=dec)
    assert not codec.caches[cache]                               # a scan inserts nothing
    r[2100:2200]                                                 # chunk 2 (and what is read ahead) becomes resident
    resident = sorted(codec.caches[cache])
    assert 2 in resident
    codec.stats_calls.clear()
    _check(r, arr, 1000, decoded=dec)
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens), = codec.stats_calls
    assert keys == list(range(6)) and [k for k, n in zip(keys, lens) if n == 0] == resident
    # an entry dropped between the query and the call: sent again with its bytes
    real = codec.window_stats

    def drop_then_call(cid, *a, **kw):
        codec.caches[cid].clear()
        codec.window_stats = real
        return real(cid, *a, **kw)
    codec.window_stats = drop_then_call
    codec.stats_calls.clear()
    _check(r, arr, 1000, decoded=dec)
    assert [sum(1 for n in lens if n == 0) for _, _, lens in codec.stats_calls] == [len(resident), 0]
    r.close()


def test_window_stats_damaged_chunk_raises_ioerror(tmp_cfg):
    arr = _recording('int16', rows=5000, nc=4, seed=7)
    codec = StatsOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    r.close()
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    ch = r.chunk_offsets
    data[ch[3] + 20:ch[3] + 40] = b'\xff' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    with pytest.raises(IOError, match='#3'):
        r[3100:3200]
    with pytest.raises(IOError, match='#3'):
        r.window_stats(100)
    _check(r, arr, 100, 0, 3000, decoded=arr)                    # the range without it is fine (integers: decoded == input)
    r.close()


def test_window_stats_needs_a_device_codec(tmp_cfg):
    arr = _recording('int16', rows=2000, nc=3, seed=8)
    r = _write(tmp_cfg, arr, OracleCodec())
    with pytest.raises(NotImplementedError):
        r.window_stats(100)
    r.close()
