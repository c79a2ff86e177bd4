"""Reader.welch, host side: the contract against scipy.signal.welch, the summation tree, lanes, calls, cache use, argument handling
and errors, driven through a numpy restatement of mts_welch (tests/welch_oracle.py).  The kernel: tests/test_gpu_welch.py."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.codec_oracle import OracleCodec
from tests.welch_oracle import WelchOracleCodec, assert_welch_close, psd_scale, welch_bound_bins, welch_f64


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _write(tmp, arr, codec, sample_rate=1000., chunk_duration=1.):
    raw = tmp / 'data.bin'
    arr.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'data.cbin', tmp / 'data.ch', sample_rate=sample_rate, n_channels=arr.shape[1], dtype=arr.dtype,
                         chunk_duration=chunk_duration, codec=codec, check_after_compress=False)
    return mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', codec=codec, check_after_decompress=False)


def _recording(rows=9000, nc=5, seed=0, dtype=np.int16):
    rs = np.random.RandomState(seed)
    t = np.arange(rows)[:, None]
    x = 3000 * np.sin(t * (0.05 + 0.03 * np.arange(nc))) + rs.randn(rows, nc) * 200 + 1500
    return x.astype(dtype)


def _cols(channels, nc):
    if isinstance(channels, int):
        return [channels % nc]
    if isinstance(channels, slice):
        return list(range(*channels.indices(nc)))
    return [int(c) % nc for c in channels]


def _check_scipy(r, x, nperseg, start, stop, channels, noverlap, window, detrend, scaling, dtype):
    signal = pytest.importorskip('scipy.signal')
    f, got = r.welch(nperseg, start, stop, channels=channels, noverlap=noverlap, window=window, detrend=detrend, scaling=scaling, dtype=dtype)
    i0 = r._validate_index(start, 0)
    i1 = max(i0, r._validate_index(stop, r.n_samples))
    cols = _cols(channels, r.n_channels)
    seg = x[i0:i1][:, cols].astype(np.float64)
    fw, want = signal.welch(seg, fs=r.sample_rate, nperseg=nperseg, noverlap=noverlap, window=window, detrend=detrend, scaling=scaling, axis=0)
    assert np.array_equal(f, fw) and f.dtype == np.float64
    assert got.dtype == np.float64
    step = nperseg - (nperseg // 2 if noverlap is None else noverlap)
    taper = api.welch_window(window, nperseg)
    tot, _, n_seg, first = welch_f64(x[:, cols], i0, i1, nperseg, step, taper, bool(detrend), dtype)
    k = psd_scale(nperseg, taper, scaling, r.sample_rate, n_seg)
    bound = k[:, None] * welch_bound_bins(tot, first, n_seg)
    got2 = got.reshape(want.shape)
    assert_welch_close(got2, want, bound * 1.01 + 1e-12 * np.abs(want))   # (scipy's own float64 rounding: below 1e-12 relative)
    return got


@pytest.mark.parametrize('nperseg', [16, 256, 1024, 4096])
def test_matches_scipy_for_every_overlap(tmp_cfg, nperseg):
    arr = _recording(rows=9000, seed=nperseg)
    r = _write(tmp_cfg, arr, WelchOracleCodec(n_lanes=1, capacity_chunks=8))
    x = r[:]
    for noverlap in (0, nperseg // 4, None, nperseg - 1):
        if nperseg == 4096 and noverlap == nperseg - 1:
            stop = 4096 + 300                              # (a few hundred segments are enough)
        else:
            stop = None
        for dtype in (np.float32, np.float64):
            _check_scipy(r, x, nperseg, 0, stop, slice(None), noverlap, 'hann', 'constant', 'density', dtype)
    r.close()


def test_windows_detrends_scalings_and_ranges(tmp_cfg):
    arr = _recording(rows=7000, nc=6, seed=1)
    r = _write(tmp_cfg, arr, WelchOracleCodec(n_lanes=1, capacity_chunks=8))
    x = r[:]
    arr_window = np.random.RandomState(2).rand(256) + 0.5
    for window in ('hann', 'hamming', 'boxcar', arr_window):
        for detrend in ('constant', False):
            for scaling in ('density', 'spectrum'):
                _check_scipy(r, x, 256, 100, 6900, slice(None), None, window, detrend, scaling, np.float32)
    for start, stop, channels in [(0, None, 2), (-3000, -1, -1), (123, 4567, slice(1, None, 2)), (None, 2000, [4, 0, 0, -2]),
                                  (6000, 7000, slice(None, None, 3)), (0, 256, [3])]:
        _check_scipy(r, x, 256, start, stop, channels, 64, 'hann', 'constant', 'density', np.float64)
    r.close()


def test_window_restatement_matches_scipy():
    signal = pytest.importorskip('scipy.signal')
    for n in (16, 256, 4096):
        for name in ('hann', 'hamming', 'boxcar'):
            assert np.allclose(api.welch_window(name, n), signal.get_window(name, n), rtol=0, atol=1e-15)


def test_float64_restatement_matches_scipy():
    signal = pytest.importorskip('scipy.signal')
    x = _recording(rows=5000, nc=3, seed=3).astype(np.float64)
    for nperseg, step, detrend in [(256, 128, True), (64, 64, False), (1024, 1000, True)]:
        taper = api.welch_window('hann', nperseg)
        tot, energy, n_seg, _ = welch_f64(x, 0, 5000, nperseg, step, taper, detrend)
        _, want = signal.welch(x, fs=1.0, nperseg=nperseg, noverlap=nperseg - step, detrend='constant' if detrend else False,
                               scaling='spectrum', axis=0)
        got = tot * psd_scale(nperseg, taper, 'spectrum', 1.0, n_seg)[:, None]
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        assert np.all(energy > 0)


@pytest.mark.parametrize('n_lanes', [2, 3])
def test_lanes_calls_and_columns_give_identical_bits(tmp_cfg, monkeypatch, n_lanes):
    monkeypatch.setattr(hip, 'WELCH_GROUP_ROWS', 1 << 11)      # (several groups in a short recording: the test needs lanes to split them)
    arr = _recording(rows=12000, seed=4, dtype=np.float32)
    one = _write(tmp_cfg, arr, WelchOracleCodec(n_lanes=1, capacity_chunks=8))
    codec = WelchOracleCodec(n_lanes=n_lanes, capacity_chunks=8)
    many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    for nperseg, noverlap in [(16, 8), (256, 0), (256, None), (1024, 1023)]:
        _, a = one.welch(nperseg, 10, 11990, noverlap=noverlap)
        _, b = many.welch(nperseg, 10, 11990, noverlap=noverlap)
        assert a.tobytes() == b.tobytes()
        for c in (0, 3):
            _, s = many.welch(nperseg, 10, 11990, channels=[c], noverlap=noverlap)
            assert s.tobytes() == np.ascontiguousarray(a[:, [c]]).tobytes()
    assert {lane for lane, *_ in codec.welch_calls} == set(range(n_lanes))
    G = hip.welch_group_segments(128)
    for lane, keys, _, s0, s1 in codec.welch_calls:
        assert keys == list(range(keys[0], keys[-1] + 1))
    monkeypatch.setattr(api, 'WELCH_CALL_BYTES', 1)
    codec.welch_calls.clear()
    _, c = many.welch(256, 10, 11990)
    _, a = one.welch(256, 10, 11990)
    assert c.tobytes() == a.tobytes()
    assert len(codec.welch_calls) == 3                           # one call per group: 92 segments, G = 32
    for _, _, _, s0, _ in codec.welch_calls:
        assert s0 % G == 0
    one.close()
    many.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    arr = _recording(rows=6000, nc=4, seed=7)
    codec = WelchOracleCodec(n_lanes=1, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    cache = r._cache_for(0)
    _, cold = r.welch(512)
    assert not codec.caches[cache]                               # a scan inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    codec.welch_calls.clear()
    _, warm = r.welch(512)
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens, _, _), = codec.welch_calls
    assert [k for k, n in zip(keys, lens) if n == 0] == resident
    assert warm.tobytes() == cold.tobytes()
    r.close()


def test_damaged_chunk_raises(tmp_cfg):
    arr = _recording(rows=5000, nc=4, seed=8)
    codec = WelchOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    r.close()
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    ch = r.chunk_offsets
    data[ch[3] + 20:ch[3] + 40] = b'\xff' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    with pytest.raises(IOError, match='#3'):
        r.welch(256, 0, 3000 + 256)                              # the last segment reads chunk 3 (rows 3000..)
    r.welch(256, 0, 3000)
    r.close()


def test_argument_errors(tmp_cfg):
    arr = _recording(rows=3000, nc=3, seed=9)
    r = _write(tmp_cfg, arr, WelchOracleCodec(n_lanes=1, capacity_chunks=8))
    for bad in (8, 15, 100, 32768, 256.0, True, -16):
        with pytest.raises(ValueError):
            r.welch(bad)
    for bad in (-1, 256, 300, 1.5, True):
        with pytest.raises(ValueError):
            r.welch(256, noverlap=bad)
    for bad in ('blackman', np.ones(255), np.ones((256, 1)), np.r_[np.ones(255), np.nan]):
        with pytest.raises(ValueError):
            r.welch(256, window=bad)
    for bad in ('linear', True, None, 'mean'):
        with pytest.raises(ValueError):
            r.welch(256, detrend=bad)
    with pytest.raises(ValueError):
        r.welch(256, scaling='psd')
    for bad in (np.int16, np.float16, 'complex64', 'nonsense'):
        with pytest.raises(ValueError):
            r.welch(256, dtype=bad)
    with pytest.raises(ValueError):
        r.welch(256, 100, 355)                                   # 255 rows: fewer than nperseg
    with pytest.raises(ValueError):
        r.welch(4096)
    with pytest.raises(IndexError):
        r.welch(256, channels=3)
    f, p = r.welch(256, 100, 356)                                # exactly one segment
    assert p.shape == (129, 3) and f.shape == (129,)
    f, p = r.welch(256, channels=[])
    assert p.shape == (129, 0)
    r.close()


def test_needs_a_device_codec(tmp_cfg):
    r = _write(tmp_cfg, _recording(rows=2000, nc=3), OracleCodec())
    with pytest.raises(NotImplementedError):
        r.welch(256)
    r.close()


def test_exact_cases_on_the_stand_in(tmp_cfg):
    nperseg, nc = 64, 3
    rows = nperseg * 20
    x = np.zeros((rows, nc), np.int16)
    x[::nperseg, 0] = 7                                          # an impulse at each segment's first row
    x[:, 1] = np.repeat(np.arange(20, dtype=np.int16) * 3 - 20, nperseg)   # piecewise constant
    x[:, 2] = -5
    r = _write(tmp_cfg, x, WelchOracleCodec(n_lanes=1, capacity_chunks=8))
    _, p = r.welch(nperseg, noverlap=0, window='boxcar', detrend=False, scaling='spectrum', dtype=np.float64)
    # spectrum scaling with a boxcar: 1 / nperseg^2; interior bins doubled; / n_seg
    k = np.full(nperseg // 2 + 1, 2.0 / nperseg ** 2 / 20)
    k[0] = k[-1] = 1.0 / nperseg ** 2 / 20
    assert np.array_equal(p[:, 0], k * 20 * 49.0)
    v = np.arange(20) * 3 - 20
    assert np.array_equal(p[:, 1], np.r_[k[0] * float((nperseg * v.astype(np.float64)) ** 2 @ np.ones(20)), np.zeros(nperseg // 2)])
    _, p = r.welch(nperseg, noverlap=0, window='hann', detrend='constant')
    assert not p[:, 1:].any()
    r.close()
