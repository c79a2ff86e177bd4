"""Reader.decimate, host side: the default taps, the contract against scipy, stitching, lanes, calls, argument handling and
errors, driven through a numpy restatement of mts_decimate (tests/decimate_oracle.py).  The kernel: tests/test_gpu_decimate.py."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api
from tests.codec_oracle import OracleCodec
from tests.decimate_oracle import DecimateOracleCodec


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


def _recording(rows=4500, nc=5, seed=0, dtype=np.int16):
    rs = np.random.RandomState(seed)
    t = np.arange(rows)[:, None]
    x = 3000 * np.sin(t * (0.01 + 0.003 * np.arange(nc))) + rs.randn(rows, nc) * 200
    return x.astype(dtype)


@pytest.mark.parametrize('q', [2, 3, 12, 40])
def test_decimate_taps_match_firwin(q):
    signal = pytest.importorskip('scipy.signal')
    want = signal.firwin(20 * q + 1, 1. / q, window='hamming')
    got = api.decimate_taps(q)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want).max())


def test_decimate_taps_arguments():
    for bad in (0, 1, -2, 2.0, True):
        with pytest.raises(ValueError):
            api.decimate_taps(bad)


@pytest.mark.parametrize('q', [2, 5, 12])
def test_zeros_edge_matches_scipy(tmp_cfg, q):
    signal = pytest.importorskip('scipy.signal')
    arr = _recording()
    r = _write(tmp_cfg, arr, DecimateOracleCodec(n_lanes=1, capacity_chunks=8))
    x = r[:].astype(np.float64)
    for start, stop in [(0, None), (123, 4001), (1000, 1000 + 7 * q + 1)]:
        got = r.decimate(q, start, stop, dtype=np.float64)
        seg = x[start:stop]
        want = signal.decimate(seg, q, ftype='fir', zero_phase=True, axis=0)
        assert got.shape == want.shape
        assert np.allclose(got, want, rtol=0, atol=1e-9 * np.abs(seg).max())
        taps = np.random.RandomState(q).randn(8)
        got = r.decimate(q, start, stop, taps=taps, dtype=np.float64)
        want = signal.resample_poly(seg, 1, q, window=taps, axis=0)
        assert got.shape == want.shape
        assert np.allclose(got, want, rtol=0, atol=1e-9 * np.abs(seg).max() * np.abs(taps).sum())
    r.close()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_recording_edge_stitches_bit_for_bit(tmp_cfg, dtype):
    arr = _recording(rows=5000, seed=1)
    r = _write(tmp_cfg, arr, DecimateOracleCodec(n_lanes=1, capacity_chunks=8))
    q = 12
    whole = r.decimate(q, 36, 4836, edge='recording', dtype=dtype)
    parts = [r.decimate(q, a, b, edge='recording', dtype=dtype) for a, b in [(36, 1236), (1236, 1248), (1248, 4836)]]
    assert np.array_equal(whole, np.concatenate(parts))
    assert whole.dtype == dtype and whole.shape == (400, 5)
    r.close()


@pytest.mark.parametrize('n_lanes', [2, 3])
def test_lanes_give_identical_bytes(tmp_cfg, n_lanes):
    arr = _recording(rows=7000, seed=2, dtype=np.float32)
    arr[1234, 2] = np.nan
    one = _write(tmp_cfg, arr, DecimateOracleCodec(n_lanes=1, capacity_chunks=8))
    codec = DecimateOracleCodec(n_lanes=n_lanes, capacity_chunks=8)
    many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    for q, edge in [(3, 'zeros'), (12, 'recording'), (97, 'zeros')]:
        a, b = one.decimate(q, 10, 6990, edge=edge), many.decimate(q, 10, 6990, edge=edge)
        assert a.tobytes() == b.tobytes()
    assert {lane for lane, _, _ in codec.decimate_calls} == set(range(n_lanes))
    for lane, keys, _ in codec.decimate_calls:                   # a lane reads adjacent chunks
        assert keys == list(range(keys[0], keys[-1] + 1))


def test_small_call_bytes_give_identical_bytes(tmp_cfg, monkeypatch):
    arr = _recording(rows=9000, seed=3)
    codec = DecimateOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    want = r.decimate(12, 500, 8700, edge='recording')
    codec.decimate_calls.clear()
    monkeypatch.setattr(api, 'DECIMATE_CALL_BYTES', 1)
    got = r.decimate(12, 500, 8700, edge='recording')
    assert got.tobytes() == want.tobytes()
    assert len(codec.decimate_calls) >= 8
    r.close()


def test_exact_taps_and_channel_forms(tmp_cfg):
    arr = _recording(rows=3500, nc=6, seed=4)
    r = _write(tmp_cfg, arr, DecimateOracleCodec(n_lanes=1, capacity_chunks=8))
    x = r[:]
    assert np.array_equal(r.decimate(3, taps=[1.0]), x[::3].astype(np.float32))
    assert np.array_equal(r.decimate(1, 5, 20, taps=[1.0], dtype=np.float64), x[5:20].astype(np.float64))
    y = r.decimate(4, 100, 3000, taps=[0, 0, 1], edge='zeros')          # half = 1: row k * q - 1, 0 before the range
    want = np.vstack([np.zeros((1, 6)), x[100 + 3:3000:4]]).astype(np.float32)[:y.shape[0]]
    assert np.array_equal(y, want)
    y = r.decimate(4, 100, 3000, taps=[0, 0, 1], edge='recording')
    assert np.array_equal(y, x[99:3000:4][:y.shape[0]].astype(np.float32))
    taps = np.random.RandomState(5).randn(10)                            # even length
    full = r.decimate(5, 200, 3200, taps=taps)
    for channels, cols in [(2, [2]), (-1, [5]), (slice(1, None, 2), [1, 3, 5]), ([4, 0, 0, -2], [4, 0, 0, 4])]:
        got = r.decimate(5, 200, 3200, channels=channels, taps=taps)
        want = full[:, cols]
        assert np.array_equal(got, want[:, 0] if isinstance(channels, int) else want)
    assert r.decimate(5, -1000, -10, taps=taps).shape == (198, 6)
    assert np.array_equal(r.decimate(5, -1000, -10, taps=taps), r.decimate(5, 2500, 3490, taps=taps))
    for start, stop in [(2000, 1000), (3500, None), (100, 100)]:
        e = r.decimate(7, start, stop)
        assert e.shape == (0, 6) and e.dtype == np.float32
    assert r.decimate(7, 5, 5, channels=2).shape == (0,)
    assert r.decimate(7, channels=[]).shape == (500, 0)
    r.close()


def test_nan_and_inf_times_zero_taps(tmp_cfg):
    arr = _recording(rows=2000, nc=3, seed=6, dtype=np.float64)
    arr[500, 1] = np.inf
    codec = DecimateOracleCodec(n_lanes=1, capacity_chunks=8)
    raw = tmp_cfg / 'data.bin'
    arr.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', sample_rate=1000., n_channels=3, dtype=np.float64, codec=codec,
                         do_time_diff=False, check_after_compress=False)
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    y = r.decimate(2, taps=[0.0, 0.0, 0.0], dtype=np.float64)          # inf * 0: NaN where row 500 is in the support (rows 2k + 1 - j)
    assert np.isnan(y[250, 1]) and not np.isnan(y[:, [0, 2]]).any()
    assert np.isnan(y[:, 1]).sum() == 1 and not y[~np.isnan(y)].any()
    r.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    arr = _recording(rows=6000, nc=4, seed=7)
    codec = DecimateOracleCodec(n_lanes=1, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    cache = r._cache_for(0)
    cold = r.decimate(12)
    assert not codec.caches[cache]                               # a scan inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    codec.decimate_calls.clear()
    warm = r.decimate(12)
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens), = codec.decimate_calls
    assert [k for k, n in zip(keys, lens) if n == 0] == resident
    assert warm.tobytes() == cold.tobytes()
    r.close()


def test_damaged_chunk_in_the_halo_raises(tmp_cfg):
    arr = _recording(rows=5000, nc=4, seed=8)
    codec = DecimateOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    r.close()
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    ch = r.chunk_offsets
    data[ch[3] + 20:ch[3] + 40] = b'\xff' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    with pytest.raises(IOError, match='#3'):
        r.decimate(12, 0, 3000, edge='recording')               # chunk 3 (rows 3000..) is in the support of the last outputs
    r.decimate(12, 0, 3000 - 120, edge='recording')               # (default taps: half = 120)
    r.close()


def test_argument_errors(tmp_cfg):
    arr = _recording(rows=2000, nc=3, seed=9)
    r = _write(tmp_cfg, arr, DecimateOracleCodec(n_lanes=1, capacity_chunks=8))
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            r.decimate(bad)
    with pytest.raises(ValueError):
        r.decimate(1)                                           # q == 1 needs taps
    with pytest.raises(ValueError):
        r.decimate(2, taps=np.ones(8193))
    for bad in ([], [[1.0]], [np.nan], [np.inf]):
        with pytest.raises(ValueError):
            r.decimate(2, taps=bad)
    for bad in (np.int16, np.float16, 'complex64', 'nonsense'):
        with pytest.raises(ValueError):
            r.decimate(2, dtype=bad)
    with pytest.raises(ValueError):
        r.decimate(2, edge='reflect')
    with pytest.raises(IndexError):
        r.decimate(2, channels=3)
    assert r.decimate(409).shape == (5, 3)                      # 8181 taps: the longest default
    r.close()


def test_needs_a_device_codec(tmp_cfg):
    r = _write(tmp_cfg, _recording(rows=2000, nc=3), OracleCodec())
    with pytest.raises(NotImplementedError):
        r.decimate(4)
    r.close()
