"""Reader.cov, host side: argument handling, windows on every item type against tests/gram_oracle.py, bit-identity across lanes and
calls, cache use, errors, and the covariance formula against exact rationals and np.cov.  The kernel: tests/test_gpu_gram.py."""
import json

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.codec_oracle import OracleCodec
from tests.gram_oracle import (GramOracleCodec, U, assert_cov_exact_bound, cov_bound, exact_gram, gamma, window_grams)
from tests.test_golden import CASES, golden_cbin

DTYPES = ['uint8', 'int8', 'uint16', 'int16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


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


def _recording(rows=5500, nc=5, seed=0, dtype='int16'):
    rs = np.random.RandomState(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        return (rs.randn(rows, nc) * 300 + rs.randn(nc) * 1000).astype(dtype)
    info = np.iinfo(dtype)
    return rs.randint(max(info.min, -(1 << 40)), min(info.max, 1 << 40), size=(rows, nc), dtype=np.int64).astype(dtype)


def _cols(channels, nc):
    if isinstance(channels, (int, np.integer)):
        return [int(channels) % nc]
    if isinstance(channels, slice):
        return list(range(*channels.indices(nc)))
    return [int(c) % nc for c in channels]


def _check(r, x, start=0, stop=None, channels=slice(None), window=None, ddof=1):
    got = r.cov(start, stop, channels=channels, window=window, ddof=ddof)
    x = r[:]                                                     # (what the chunks decode to: float data with a time diff is not the input)
    i0 = r._validate_index(start, 0)
    i1 = max(i0, r._validate_index(stop, r.n_samples))
    cols = _cols(channels, r.n_channels)
    xs = x[:, cols]
    G, S = window_grams(xs, i0, i1, window)
    g_dt, s_dt = hip.gram_dtypes(x.dtype)
    assert got.gram.dtype == g_dt and got.sum.dtype == s_dt and got.count.dtype == np.int64
    assert got.gram.tobytes() == G.tobytes() and got.sum.tobytes() == S.tobytes()
    w = window or max(i1 - i0, 1)
    n_win = -(-(i1 - i0) // w)
    assert got.count.tolist() == [min(w, i1 - i0 - k * w) for k in range(n_win)]
    assert got.cov.shape == (n_win, len(cols), len(cols)) and got.mean.shape == (n_win, len(cols))
    assert (got.start, got.stop, got.window) == (i0, i1, w) and got.channels.tolist() == cols
    if hip.gram_exact(x.dtype):                                  # the exact types: numpy int64, bit for bit
        for k in range(n_win):
            a = xs[i0 + k * w:min(i1, i0 + (k + 1) * w)].astype(np.int64)
            assert np.array_equal(got.gram[k], a.T @ a)
    if x.dtype.kind in 'iu':
        for k in range(n_win):
            assert np.array_equal(got.sum[k], xs[i0 + k * w:min(i1, i0 + (k + 1) * w)].astype(np.int64).sum(0))
    with np.errstate(invalid='ignore', divide='ignore'):
        sf = got.sum.astype(np.float64)
        mean = sf / got.count[:, None]
        want = (got.gram.astype(np.float64) - sf[:, :, None] * mean[:, None, :]) / (got.count - ddof)[:, None, None]
    want[got.count - ddof <= 0] = np.nan
    assert got.cov.tobytes() == want.tobytes() and got.mean.tobytes() == mean.tobytes()
    return got


def test_arguments(tmp_cfg):
    x = _recording(rows=3000, nc=4, seed=1)
    r = _write(tmp_cfg, x, GramOracleCodec(n_lanes=1, capacity_chunks=8))
    for bad in (0, -1, 1.5, True, '7'):
        with pytest.raises(ValueError):
            r.cov(window=bad)
    for bad in (-1, 1.5, True, None, '1'):
        with pytest.raises(ValueError):
            r.cov(ddof=bad)
    with pytest.raises(ValueError):
        r.cov(channels=slice(None, None, -1))
    for bad in (4, -5, [0, 4], [[0, 1]], [0.5]):
        with pytest.raises(IndexError):
            r.cov(channels=bad)
    got = _check(r, x, channels=2)                              # an int: C = 1, nothing squeezed
    assert got.gram.shape == (1, 1, 1) and got.sum.shape == (1, 1)
    for start, stop in [(None, None), (-1000, -1), (100, 50), (2999, None), (0, 10 ** 9), (-10 ** 9, 5), (123, 2456)]:
        for window in (None, 1, 7, 1000):
            for ddof in (0, 1, 3):
                got = _check(r, x, start, stop, window=window, ddof=ddof)
                n = r[start:stop].shape[0]
                assert got.count.sum() == n
    got = r.cov(channels=[])
    assert got.gram.shape == (1, 0, 0) and got.count.tolist() == [3000]
    got = r.cov(100, 100)
    assert got.gram.shape == (0, 4, 4) and got.cov.shape == (0, 4, 4)
    _check(r, x, channels=[3, 0, 0, -1, 2])
    _check(r, x, channels=slice(1, None, 2), window=999)
    r.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_windows_every_dtype(tmp_cfg, dtype):
    x = _recording(rows=4500, nc=6, seed=2, dtype=dtype)
    r = _write(tmp_cfg, x, GramOracleCodec(n_lanes=2, capacity_chunks=8))
    for window in (None, 1, 7, 1000, 3001, 4505):
        for channels in (slice(None), slice(1, None, 3), [5, 0, 2, 2, 1]):
            _check(r, x, 10, -3, channels=channels, window=window)
    r.close()


def test_exact_types_wrap_like_numpy(tmp_cfg, monkeypatch):
    monkeypatch.setattr(hip, 'GRAM_GROUP_ROWS', 1 << 10)        # (many groups per window in a short recording)
    rows = 6000
    x = np.empty((rows, 4), np.int16)
    x[:, 0] = -32768
    x[:, 1] = np.where(np.arange(rows) % 2, 32767, -32768)
    x[:, 2] = 32767
    x[:, 3] = np.arange(rows) % 7 - 3
    r = _write(tmp_cfg, x, GramOracleCodec(n_lanes=3, capacity_chunks=8))
    got = _check(r, x)
    a = x.astype(np.int64)
    assert np.array_equal(got.gram[0], a.T @ a)
    r.close()
    u = np.full((rows, 2), 65535, np.uint16)
    r = _write(tmp_cfg, u, GramOracleCodec(n_lanes=2, capacity_chunks=8))
    got = _check(r, u, window=2500)
    assert got.gram[0, 0, 0] == 2500 * 65535 ** 2
    r.close()


@pytest.mark.parametrize('n_lanes', [1, 2, 3])
def test_lanes_and_calls_give_identical_bits(tmp_cfg, monkeypatch, n_lanes):
    monkeypatch.setattr(hip, 'GRAM_GROUP_ROWS', 1 << 11)        # (several groups per window: lanes and calls split them)
    x = _recording(rows=12000, nc=5, seed=4, dtype='float32')
    one = _write(tmp_cfg, x, GramOracleCodec(n_lanes=1, capacity_chunks=8))
    codec = GramOracleCodec(n_lanes=n_lanes, capacity_chunks=8)
    many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    for window in (None, 5000, 1500, 7):
        a, b = one.cov(10, 11990, window=window), many.cov(10, 11990, window=window)
        for key in ('gram', 'sum', 'cov', 'mean', 'count'):
            assert a[key].tobytes() == b[key].tobytes(), key
        _check(many, x, 10, 11990, window=window)
    if n_lanes > 1:
        assert {lane for lane, *_ in codec.gram_calls} == set(range(n_lanes))
    for lane, keys, _, g0, g1 in codec.gram_calls:
        assert keys == list(range(keys[0], keys[-1] + 1)) and g1 > g0
    monkeypatch.setattr(api, 'GRAM_CALL_BYTES', 1)             # one call per group: calls cut inside windows
    codec.gram_calls.clear()
    c = many.cov(10, 11990)
    a = one.cov(10, 11990)
    for key in ('gram', 'sum', 'cov'):
        assert c[key].tobytes() == a[key].tobytes(), key
    assert len(codec.gram_calls) == hip.gram_groups(10, 11990, 11980) == 6
    assert all(g1 == g0 + 1 for *_, g0, g1 in codec.gram_calls)
    monkeypatch.setattr(api, 'GRAM_SLAB_BYTES', 1)             # results: one group per call too
    codec.gram_calls.clear()
    assert many.cov(window=3).gram.tobytes() == one.cov(window=3).gram.tobytes()
    assert all(g1 == g0 + 1 for *_, g0, g1 in codec.gram_calls)
    one.close()
    many.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    x = _recording(rows=6000, nc=4, seed=7)
    codec = GramOracleCodec(n_lanes=1, capacity_chunks=8)
    r = _write(tmp_cfg, x, codec)
    cache = r._cache_for(0)
    cold = r.cov()
    assert not codec.caches[cache]                               # a scan inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    assert resident
    codec.gram_calls.clear()
    warm = r.cov()
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens, _, _), = codec.gram_calls
    assert [k for k, n in zip(keys, lens) if n == 0] == resident
    for key in ('gram', 'sum', 'cov'):
        assert warm[key].tobytes() == cold[key].tobytes()
    r.close()


def test_damaged_chunk_raises(tmp_cfg):
    x = _recording(rows=5000, nc=4, seed=8)
    codec = GramOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, x, codec)
    r.close()
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    ch = r.chunk_offsets
    data[ch[3] + 20:ch[3] + 40] = b'\xff' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    with pytest.raises(IOError, match='#3'):
        r.cov(0, 3001)                                           # row 3000 is in chunk 3
    r.cov(0, 3000)
    r.close()


def test_needs_a_device_codec(tmp_cfg):
    r = _write(tmp_cfg, _recording(rows=2000, nc=3), OracleCodec())
    with pytest.raises(NotImplementedError):
        r.cov()
    r.close()


def test_cov_formula_against_exact_rationals(tmp_cfg):
    rs = np.random.RandomState(9)
    worst = 0.0
    for n, nc, offset in [(2, 3, 32000), (3, 4, -32000), (17, 4, 30000), (400, 5, 0), (2500, 3, -31000)]:
        x = np.clip(rs.randint(-300, 300, size=(n, nc)) + offset * rs.choice([-1, 0, 1], nc), -32768, 32767).astype(np.int16)
        x[:, 0] = -32768                                         # an all -32768 column
        r = _write(tmp_cfg, x, GramOracleCodec(n_lanes=1, capacity_chunks=8), chunk_duration=0.5)
        for ddof in (0, 1, 2):
            got = r.cov(ddof=ddof)
            if n - ddof <= 0:
                continue
            worst = max(worst, assert_cov_exact_bound(got.cov[0], got.gram[0], got.sum[0], n, ddof))
        r.close()
    print('cov against Fraction: worst error / bound %.3g' % worst)


def test_nan_where_count_minus_ddof_not_positive(tmp_cfg):
    case = CASES['np385_1sample']
    hdr = json.loads(case['ch_text'])
    p = tmp_cfg / 'one.cbin'
    p.write_bytes(golden_cbin(case))
    r = mtscomp_amd.Reader(codec=GramOracleCodec(n_lanes=1, capacity_chunks=8), check_after_decompress=False)
    r.open(p, cmeta=hdr)
    x = r[:]
    with np.errstate(all='raise'):                               # no warning
        got = r.cov(channels=slice(0, 20))
    assert got.count.tolist() == [1] and np.isnan(got.cov).all()
    assert np.array_equal(got.gram[0], x[:, :20].astype(np.int64).T @ x[:, :20].astype(np.int64))
    got = r.cov(channels=slice(0, 20), ddof=0)
    assert not np.isnan(got.cov).any() and (got.cov == 0).all()
    got = r.cov(0, 0)
    assert got.cov.shape == (0, 385, 385)
    r.close()


def test_cov_against_np_cov(tmp_cfg):
    rs = np.random.RandomState(10)
    worst = 0.0
    for n, offset in [(10, 30000), (1000, 0), (3000, -20000), (30000, 12345)]:
        nc = 4
        x = np.clip(rs.randint(-2000, 2000, size=(n, nc)) + offset * np.array([1, -1, 0, 1]) // (1 + np.arange(nc)), -32768, 32767).astype(np.int16)
        r = _write(tmp_cfg, x, GramOracleCodec(n_lanes=2, capacity_chunks=8), chunk_duration=float(max(n // 3000, 1)))
        got = r.cov()
        want = np.cov(x, rowvar=False, ddof=1)
        m = x.astype(np.float64).mean(0)
        dev = np.abs(x.astype(np.float64) - m)
        allow = cov_bound(got.gram[0], got.sum[0], n, 1) + gamma(n + 2) * (dev.T @ dev) / (n - 1)
        err = np.abs(got.cov[0] - want)
        assert (err <= allow).all(), (err / allow).max()
        worst = max(worst, float((err / allow).max()))
        r.close()
    print('cov against np.cov: worst error / allowance %.3g' % worst)
    assert U == 2.0 ** -53
    assert np.array_equal(exact_gram(np.full((3, 2), -32768, np.int16)), np.full((2, 2), 3 * 2 ** 30))
