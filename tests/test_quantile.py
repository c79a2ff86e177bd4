"""Reader.quantile / median / mad, host side: argument handling, every item type over windows, channel sets and methods against
tests/select_oracle.py, the contract with np.median, np.quantile and scipy's median_abs_deviation, special floats in the three key
modes, bit-identity across lanes and calls, cache use, errors, and the round cap.  The kernel: tests/test_gpu_quantile.py."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.codec_oracle import OracleCodec
from tests.select_oracle import (S, SelectOracleCodec, brute_round, check_all, check_quantile, empty_outputs, keys_of, np_mad, np_median,
                                 position, round_add, same_values, scipy_mad)

DTYPES = ['uint8', 'int8', 'uint16', 'int16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']
METHODS = ('linear', 'lower', 'higher', 'nearest', 'midpoint')


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _write(tmp, arr, codec, sample_rate=1000., chunk_duration=1., **kw):
    raw = tmp / 'data.bin'
    arr.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'data.cbin', tmp / 'data.ch', sample_rate=sample_rate, n_channels=arr.shape[1], dtype=arr.dtype,
                         chunk_duration=chunk_duration, codec=codec, check_after_compress=False, **kw)
    return mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', codec=codec, check_after_decompress=False)


def _recording(rows=4500, nc=6, seed=0, dtype='int16', spread=None):
    rs = np.random.RandomState(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        return (rs.randn(rows, nc) * 300 + rs.randn(nc) * 1000).astype(dtype)
    info = np.iinfo(dtype)
    lo, hi = (max(info.min, -(1 << 62)), min(info.max, 1 << 62)) if spread is None else (max(info.min, -spread), min(info.max, spread))
    return rs.randint(lo, hi, size=(rows, nc), dtype=np.int64).astype(dtype)


def _cols(channels, nc):
    if isinstance(channels, (int, np.integer)):
        return [int(channels) % nc]
    if isinstance(channels, slice):
        return list(range(*channels.indices(nc)))
    return [int(c) % nc for c in channels]


def test_arguments(tmp_cfg):
    x = _recording(rows=3000, nc=4, seed=1)
    r = _write(tmp_cfg, x, SelectOracleCodec(n_lanes=1, capacity_chunks=8))
    for bad in (0, -1, 1.5, True, '7'):
        with pytest.raises(ValueError):
            r.median(window=bad)
        with pytest.raises(ValueError):
            r.quantile(0.5, window=bad)
    for bad in (-0.1, 1.0001, float('nan'), [0.5, 2], [[0.5]], 'a', None, True):
        with pytest.raises(ValueError):
            r.quantile(bad)
    for bad in ('Linear', 'median_unbiased', None):
        with pytest.raises(ValueError):
            r.quantile(0.5, method=bad)
    with pytest.raises(ValueError):
        r.quantile(0.5, channels=slice(None, None, -1))
    for bad in (4, -5, [0, 4], [[0, 1]], [0.5]):
        with pytest.raises(IndexError):
            r.mad(channels=bad)
    with pytest.raises(ValueError):
        r.mad(center='mean')
    with pytest.raises(ValueError):
        r.quantile(0.5, center=np.zeros((2, 3)))
    # shapes: a scalar q drops the n_q axis, an int channel the C axis
    a = r.quantile(0.5, window=1000)
    assert a.quantile.shape == a.lower.shape == (3, 4) and a.index.shape == a.frac.shape == (3,) and a.q.shape == (1,)
    b = r.quantile([0.5, 1], window=1000, channels=2)
    assert b.quantile.shape == b.upper.shape == (3, 2) and b.index.shape == (3, 2) and b.channels.tolist() == [2]
    c = r.quantile(0.5, channels=-1)
    assert c.quantile.shape == (1,) and c.lower.dtype == x.dtype and (c.start, c.stop, c.window, c.method) == (0, 3000, 3000, 'linear')
    assert r.median(channels=1).shape == (1,) and r.mad(channels=1, window=1000).mad.shape == (3,)
    for start, stop in [(None, None), (-1000, -1), (2999, None), (0, 10 ** 9), (-10 ** 9, 5), (123, 2456)]:
        for window in (None, 7, 1000):
            check_all(r, x, start, stop, window, slice(None), [0, 1, 2, 3], q=(0.0, 0.4, 1.0))
    # no rows: zero windows; no channels: C = 0 arrays and no chunk touched
    e = r.quantile([0.1, 0.9], 100, 50)
    assert e.quantile.shape == (0, 2, 4) and e.count.shape == (0,) and e.lower.dtype == x.dtype
    assert r.median(100, 100).shape == (0, 4) and r.mad(100, 100).mad.shape == (0, 4)
    n_calls = len(r.codec.rank_calls)
    e = r.quantile([0.1, 0.9], channels=[], window=1000)
    assert e.quantile.shape == (3, 2, 0) and e.count.tolist() == [1000] * 3 and r.mad(channels=[]).mad.shape == (1, 0)
    assert len(r.codec.rank_calls) == n_calls
    r.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_windows_channels_methods_every_dtype(tmp_cfg, dtype):
    x = _recording(rows=4500, nc=6, seed=2, dtype=dtype)
    r = _write(tmp_cfg, x, SelectOracleCodec(n_lanes=2, capacity_chunks=8))
    x = r[:]                                                    # (what the chunks decode to: float data with a time diff is not the input)
    q = (0.0, 0.1, 1 / 3, 0.5, 0.999, 1.0)
    for window in (None, 1, 7, 1000, 3001, 4505):
        start, stop = (900, 1130) if window in (1, 7) else (10, -3)       # (a cell costs a histogram: few rows for the small windows)
        for channels in (slice(None), slice(1, None, 3), [5, 0, 2, 2, 1], 4):
            check_all(r, x, start, stop, window, channels, _cols(channels, 6), q=q, methods=METHODS)
        assert r.quantile(list(q), start, stop, channels=[], window=window).quantile.shape[1:] == (len(q), 0)
    r.close()


def _spacing(v):
    return np.spacing(np.abs(v))


@pytest.mark.parametrize('dtype', DTYPES)
def test_against_numpy_and_scipy(tmp_cfg, dtype):
    """median == np.median by value (mad against scipy: test_mad_equals_scipy); 'linear' within 4 spacing(max(|lo|, |hi|)) + |hi - lo| 4 spacing(n - 1) of
    np.quantile (the second term: numpy rounds its floating position q (n - 1), this interface computes it exactly); the discrete
    methods equal to np.quantile's wherever numpy's floating position picks the same index ('midpoint' within one rounding: numpy forms
    lo + (hi - lo) * 0.5), and to the sorted array everywhere."""
    x = _recording(rows=2100, nc=3, seed=3, dtype=dtype, spread=None if dtype not in ('int64', 'uint64') else 1 << 52)
    r = _write(tmp_cfg, x, SelectOracleCodec(n_lanes=2, capacity_chunks=8))
    x = r[:]
    xf = x.astype(np.float64)
    for n in (1, 2, 7, 1000, 1001):
        a, b = 50, 50 + n
        assert same_values(r.median(a, b), np.median(xf[a:b], axis=0)[None])
        assert same_values(r.mad(a, b).mad, np_mad(x, a, b, None))
        qs = [0, .1, .25, 1 / 3, .5, .9, .999, 1]
        got = r.quantile(qs, a, b)
        want = np.quantile(xf[a:b], qs, axis=0)
        lo, hi = got.lower[0].astype(np.float64), got.upper[0].astype(np.float64)
        bound = 4 * _spacing(np.maximum(np.abs(lo), np.abs(hi))) + np.abs(hi - lo) * 4 * np.spacing(float(n - 1))
        assert (np.abs(got.quantile[0] - want) <= bound).all(), (n, float(np.max(np.abs(got.quantile[0] - want) / bound)))
    for n in (1, 2, 5, 9, 17, 1000, 1025):
        a, b = 20, 20 + n
        for qv in [k / 8 for k in range(9)] + [0.1, 0.3]:
            j, g, _ = position(qv, n)
            fj, fg = divmod(qv * (n - 1), 1)
            same_index = int(fj) == j and (fg > 0) == (g > 0) and (fg < 0.5) == (g < 0.5) and (fg > 0.5) == (g > 0.5)
            for method in ('lower', 'higher', 'nearest', 'midpoint'):
                got = r.quantile(qv, a, b, method=method)
                check_quantile(r.quantile([qv], a, b, method=method), x, a, b, None, [qv], method)
                if not same_index:
                    continue
                want = np.quantile(xf[a:b], qv, axis=0, method=method)
                if method == 'midpoint':
                    lo, hi = got.lower[0].astype(np.float64), got.upper[0].astype(np.float64)
                    assert (np.abs(got.quantile[0] - want) <= 2 * _spacing(np.maximum(np.abs(lo), np.abs(hi)))).all(), (n, qv)
                else:
                    assert same_values(got.quantile[0], want), (n, qv, method)
    r.close()


def test_eight_byte_integers_are_ordered_exactly(tmp_cfg):
    big = np.array([2 ** 62 + 1, 2 ** 62, 2 ** 62 + 2, 2 ** 62 + 3, -2 ** 62 - 1], np.int64)        # float64 cannot tell the first four apart
    x = np.stack([big, big[::-1]], axis=1)
    r = _write(tmp_cfg, x, SelectOracleCodec(n_lanes=1, capacity_chunks=8))
    got = r.quantile([0, 0.25, 0.5, 0.75, 1], method='lower')
    assert got.lower[0, :, 0].tolist() == sorted(big.tolist()) and got.lower[0, :, 1].tolist() == sorted(big.tolist())
    r.close()
    u = np.array([[2 ** 64 - 1], [2 ** 63], [2 ** 63 + 1], [0], [2 ** 64 - 2]], np.uint64)
    r = _write(tmp_cfg, u, SelectOracleCodec(n_lanes=1, capacity_chunks=8))
    assert r.quantile([0, 0.25, 0.5, 0.75, 1], method='nearest').lower[0, :, 0].tolist() == [0, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 2, 2 ** 64 - 1]
    r.close()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_special_floats_in_the_three_key_modes(tmp_cfg, dtype):
    rs = np.random.RandomState(4)
    x = (rs.randn(2400, 7) * 10).astype(dtype)
    x[100, 1] = np.nan
    x[101, 1] = -np.nan
    x[300, 2] = np.inf
    x[450, 3] = -np.inf
    x[500, 4], x[501, 4] = np.inf, -np.inf
    x[:, 5] = 0
    x[::2, 5] = -0.0
    x[450, 5] = 1.0
    x[:, 6] = np.where(rs.rand(2400) < 0.5, -0.0, 0.0)
    x[7, 6], x[8, 6] = np.finfo(dtype).tiny / 4, -np.finfo(dtype).max
    r = _write(tmp_cfg, x, SelectOracleCodec(n_lanes=2, capacity_chunks=8), do_time_diff=False)
    assert np.array_equal(r[:], x, equal_nan=True)
    for window in (None, 700, 1):
        start, stop = (95, 105) if window == 1 else (0, 2400)
        check_all(r, x, start, stop, window, slice(None), list(range(7)), methods=METHODS)
    q = [0, 0.5, 0.9999, 1]
    cen = rs.randn(4, 7) * 5
    cen[2, 0], cen[3, 2], cen[1, 3] = np.nan, np.inf, -np.inf
    for absolute in (False, True):
        for method in METHODS:
            got = r.quantile(q, window=700, center=cen, absolute=absolute, method=method)
            check_quantile(got, x, 0, 2400, 700, q, method, mode=2 if absolute else 1, center=cen)
    got = r.quantile(q, window=700, absolute=True)                 # center None is 0
    check_quantile(got, x, 0, 2400, 700, q, 'linear', mode=2, center=np.zeros(7))
    assert same_values(r.mad(window=700, center=np.zeros(7)).mad, np_mad(x, 0, 2400, 700, center=np.zeros(7)))
    # a window that holds a NaN: a NaN result, while lower / upper are the order statistics (the NaNs sort last)
    lone = r.quantile([0.5, 1.0], channels=1)
    assert np.isnan(lone.quantile).all() and np.isfinite(lone.lower[0, 0]) and np.isnan(lone.upper[0, 1])
    assert np.isnan(r.median(channels=1)).all() and np.isnan(r.mad(channels=1).mad).all()
    # the zeros are one key: +0 comes back whichever was met first
    z = r.quantile(0.5, channels=6, method='lower')
    assert z.lower[0] == 0 and not np.signbit(z.lower[0])
    r.close()


def test_keys_order_like_numpy_sorts():
    rs = np.random.RandomState(5)
    for dtype in DTYPES:
        x = _recording(rows=400, nc=1, seed=6, dtype=dtype)[:, 0]
        if np.dtype(dtype).kind == 'f':
            x[:8] = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, np.finfo(dtype).tiny / 2, -np.finfo(dtype).tiny / 2]
        else:
            x[:2] = [np.iinfo(dtype).min, np.iinfo(dtype).max]
        k = hip.rank_keys(x)
        assert k.dtype == np.uint64 and np.array_equal(k, keys_of(x)) and int(k.max()) < 1 << hip.rank_key_bits(dtype)
        assert same_values(hip.rank_values(np.sort(k), dtype), np.sort(x))
        for mode in (1, 2):
            c = float(rs.randn() * 50)
            k = hip.rank_keys(x, mode, c)
            assert np.array_equal(k, keys_of(x, mode, c))
            d = x.astype(np.float64) - c
            assert same_values(hip.rank_values(np.sort(k), dtype, mode), np.sort(np.abs(d) if mode == 2 else d))
    assert hip.rank_keys(np.array([-0.0], np.float32))[0] == hip.rank_keys(np.array([0.0], np.float32))[0] == 1 << 31
    assert hip.rank_keys(np.array([np.nan, -np.nan]))[0] == hip.rank_keys(np.array([np.nan, -np.nan]))[1] == hip.rank_key_nan(np.float64)
    assert hip.rank_keys(np.array([np.inf]))[0] < hip.rank_key_nan(np.float64)


def test_a_round_agrees_with_a_brute_force_count():
    rs = np.random.RandomState(7)
    for dtype, mode in (('int16', 0), ('uint8', 0), ('float32', 0), ('int64', 0), ('int16', 2), ('float64', 1)):
        x = _recording(rows=300, nc=2, seed=8, dtype=dtype, spread=3000)
        kb = hip.rank_key_bits(dtype, mode)
        cen = rs.randn(1, 2) * 100 if mode else None
        ks = hip.rank_keys(x, mode, cen)
        pref = np.zeros((1, S, 2), np.uint64)
        shift = np.zeros((1, S, 2), np.int64)
        shift[0, 0] = kb - 8
        shift[0, 1] = max(kb - 16, 0)
        if kb > 8:
            pref[0, 1] = ks[17] >> np.uint64(kb - 8)               # the top digit of some item
        else:
            shift[0, 1] = -1
        out = empty_outputs(1, 2)
        count = round_add(out, x[:130], 40, 60, 340, 280, mode, cen, pref, shift)       # two chunks of file rows 40 .. 339, the range cuts both
        count += round_add(out, x[130:], 170, 60, 340, 280, mode, cen, pref, shift)
        assert count.tolist() == [280]
        for j in range(2):
            h, kmin, kmax = brute_round(x[20:, j], mode, None if cen is None else cen[0, j], [int(p) for p in pref[0, :, j]],
                                        [int(s) for s in shift[0, :, j]])
            assert out[0][0, :, :, j].tolist() == h and out[1][0, :, j].tolist() == kmin and out[2][0, :, j].tolist() == kmax


def test_same_bytes_from_any_lanes_and_calls(tmp_cfg, monkeypatch):
    x = _recording(rows=6400, nc=5, seed=9, dtype='float32')
    base = None
    for lanes in (1, 2, 3):
        codec = SelectOracleCodec(n_lanes=lanes, capacity_chunks=8)
        r = _write(tmp_cfg, x, codec)
        res = [r.quantile([0.2, 0.5], 7, -9, window=w) for w in (None, 2500)] + [r.mad(7, -9, window=2500)]
        flat = b''.join(a[k].tobytes() for a in res for k in ('quantile', 'lower', 'upper', 'mad', 'count') if k in a)
        base = base or flat
        assert flat == base
        assert {c[0] for c in codec.rank_calls} == set(range(lanes))
        assert all(k % lanes == lane for lane, keys, *_ in codec.rank_calls for k in keys)      # chunk k on lane k mod lanes
        if lanes == 2:
            n_calls = len(codec.rank_calls)
            monkeypatch.setattr(api, 'QUANTILE_CALL_BYTES', 1)         # one chunk per call: every window of 2500 rows is split over calls
            got = r.quantile([0.2, 0.5], 7, -9, window=2500)
            assert len(codec.rank_calls) - n_calls > 7 and max(len(c[1]) for c in codec.rank_calls[n_calls:]) == 1
            assert got.quantile.tobytes() == res[1].quantile.tobytes()
            monkeypatch.setattr(api, 'QUANTILE_CALL_BYTES', 1 << 30)
            monkeypatch.setattr(api, 'QUANTILE_SLAB_BYTES', 1)         # one window per run
            n_calls = len(codec.rank_calls)
            got = r.quantile([0.2, 0.5], 7, -9, window=2500)
            assert got.quantile.tobytes() == res[1].quantile.tobytes() and got.lower.tobytes() == res[1].lower.tobytes()
            assert {(c[3], c[4]) for c in codec.rank_calls[n_calls:]} == {(7, 2507), (2507, 5007), (5007, 6391)}
            assert r.mad(7, -9, window=2500).mad.tobytes() == res[2].mad.tobytes()
            monkeypatch.setattr(api, 'QUANTILE_SLAB_BYTES', 1 << 30)
        r.close()


def test_cache_use_no_insertion_miss_retry_and_errors(tmp_cfg):
    x = _recording(rows=5200, nc=4, seed=10)
    codec = SelectOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, x, codec)
    cold = r.median(window=1700)
    assert all(not c for c in codec.caches.values())                # a scan inserts nothing
    assert all(all(n > 0 for n in c[2]) for c in codec.rank_calls)
    r[1005:1010]
    r[2005:2010]                                                    # chunks 1 and 2 resident, on lanes 1 and 0
    before = {cid: sorted(c) for cid, c in codec.caches.items()}
    assert sorted(k for v in before.values() for k in v) == [1, 2]
    n_calls = len(codec.rank_calls)
    warm = r.median(window=1700)
    assert warm.tobytes() == cold.tobytes()
    assert {cid: sorted(c) for cid, c in codec.caches.items()} == before
    for lane, keys, lens, *_ in codec.rank_calls[n_calls:]:        # resident chunks went without bytes, the others with
        assert [n == 0 for n in lens] == [k in (1, 2) for k in keys]
    # an entry dropped between the query and the call: E_MISS, then everything is sent
    real, state = codec.rank_hist, {'n': 0}

    def dropping(cache_id, keys, *a, **kw):
        if state['n'] == 0 and 1 in keys:
            state['n'] = 1
            codec.caches[cache_id].pop(1)
        return real(cache_id, keys, *a, **kw)
    codec.rank_hist = dropping
    n_calls = len(codec.rank_calls)
    assert r.median(window=1700).tobytes() == cold.tobytes()
    retried = [c for c in codec.rank_calls[n_calls:] if 1 in c[1]]
    assert retried[0][2][retried[0][1].index(1)] == 0 and all(n > 0 for n in retried[1][2])
    codec.rank_hist = real
    r.close()
    # a damaged chunk: the IOError of Reader[...]
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    o = r.chunk_offsets
    data[o[3] + 20:o[3] + 40] = b'\x00' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=SelectOracleCodec(n_lanes=2, capacity_chunks=8),
                               check_after_decompress=False)
    for call in (lambda: r.median(), lambda: r.quantile(0.9, window=500), lambda: r.mad(window=1700)):
        with pytest.raises(IOError, match='#3'):
            call()
    assert same_values(r.median(0, 3000), np_median(x, 0, 3000, None))
    r.close()
    # a codec without the capability
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=OracleCodec(), check_after_decompress=False)
    for call in (lambda: r.median(), lambda: r.quantile(0.5), lambda: r.mad()):
        with pytest.raises(NotImplementedError):
            call()
    r.close()


@pytest.mark.parametrize('dtype', ['uint8', 'int16', 'int32', 'float32', 'int64', 'float64'])
def test_round_cap(tmp_cfg, dtype):
    """At most ceil(key_bits / 8) rounds per scan of two ranks, whatever the data: spread over the whole type, and an adversary whose
    candidates never share a bit (so no bit is skipped)."""
    x = _recording(rows=2048, nc=3, seed=11, dtype=dtype)
    if np.dtype(dtype).kind != 'f':
        x[:, 0] = (np.arange(2048) * (np.iinfo(dtype).max // 2048 + 1)).astype(dtype)
    r = _write(tmp_cfg, x, SelectOracleCodec(n_lanes=1, capacity_chunks=8), do_time_diff=False)
    kb = 8 * np.dtype(dtype).itemsize
    codec = r.codec

    def rounds_of(run):
        """The rounds a call reports, checked against the device calls the codec saw (one lane, one call per round here)."""
        n = len(codec.rank_calls)
        got = run()
        assert got.rounds == len(codec.rank_calls) - n
        return got
    for mode_bits, run in ((kb, lambda: r.quantile(0.5, method='midpoint')), (64, lambda: r.quantile(0.5, center=0.25, absolute=True))):
        assert 1 <= rounds_of(run).rounds <= -(-mode_bits // 8), dtype
    assert rounds_of(lambda: r.quantile([0.1, 0.5, 0.9])).rounds <= 3 * -(-kb // 8)       # up to 6 distinct ranks: 3 scans of 2
    assert rounds_of(lambda: r.mad()).rounds <= -(-kb // 8) + 8                            # the median, then the float64 keys
    const = np.full((500, 2), 7, dtype)
    r.close()
    r = _write(tmp_cfg, const, SelectOracleCodec(n_lanes=1, capacity_chunks=8))
    codec = r.codec
    got = rounds_of(lambda: r.quantile(0.5, method='midpoint'))
    assert (got.quantile == 7).all() and got.rounds == 1            # kmin == kmax: resolved by the first round
    assert (r.median() == 7).all() and r.quantile(0.5, channels=[]).rounds == 0
    r.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_mad_equals_scipy(tmp_cfg, dtype):
    pytest.importorskip('scipy')
    x = _recording(rows=2100, nc=3, seed=3, dtype=dtype, spread=None if dtype not in ('int64', 'uint64') else 1 << 52)
    r = _write(tmp_cfg, x, SelectOracleCodec(n_lanes=2, capacity_chunks=8))
    x = r[:]
    for n in (1, 2, 7, 1000, 1001):
        assert same_values(r.mad(50, 50 + n).mad, scipy_mad(x, 50, 50 + n, None))
    assert same_values(r.mad(window=700).mad, scipy_mad(x, 0, 2100, 700))
    r.close()
