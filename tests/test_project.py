"""Reader.project, host side: slices, channel forms, lanes, calls, cache use, argument handling and errors, driven through a numpy
restatement of mts_project (tests/project_oracle.py).  The kernel: tests/test_gpu_project.py."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.codec_oracle import OracleCodec
from tests.project_oracle import ProjectOracleCodec, assert_same_bits, project_chain


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _write(tmp, arr, codec, **kw):
    raw = tmp / 'data.bin'
    arr.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'data.cbin', tmp / 'data.ch', sample_rate=1000., n_channels=arr.shape[1], dtype=arr.dtype,
                         codec=codec, check_after_compress=False, **kw)
    return mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', codec=codec, check_after_decompress=False)


def _recording(rows=4500, nc=6, seed=0, dtype=np.int16):
    rs = np.random.RandomState(seed)
    t = np.arange(rows)[:, None]
    x = 3000 * np.sin(t * (0.01 + 0.003 * np.arange(nc))) + rs.randn(rows, nc) * 200
    return x.astype(dtype)


def test_has_the_feature():
    assert callable(api.Reader.project) and callable(api.HipCodec.project) and callable(api.whitening_weights)
    assert callable(hip.project) and callable(hip.dev_project)
    assert hip.PROJECT_MAX_COLS == hip.PROJECT_MAX_OUT == 1024
    assert {'mts_project', 'mts_dev_project'} <= set(hip.EXPORTS)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_slices_and_ranges(tmp_cfg, dtype):
    arr = _recording()
    r = _write(tmp_cfg, arr, ProjectOracleCodec(n_lanes=1, capacity_chunks=8))
    x = r[:]
    rs = np.random.RandomState(1)
    w, off = rs.randn(6, 4), rs.randn(6) * 100
    whole = project_chain(x, off, w, dtype)
    assert r.chunk_bounds[1] == 1000                                 # (slices below start and stop mid-chunk)
    for start, stop in [(0, None), (123, 4001), (1500, 1501), (999, 1001), (None, 2500), (-1000, -10), (-100000, 100000), (4400, 99999)]:
        got = r.project(w, start, stop, offset=off, dtype=dtype)
        assert got.dtype == dtype
        assert_same_bits(got, whole[slice(start, stop)])
    for start, stop in [(2000, 1000), (4500, None), (100, 100)]:
        e = r.project(w, start, stop, dtype=dtype)
        assert e.shape == (0, 4) and e.dtype == dtype
    r.close()


def test_channel_forms_weights_and_offsets(tmp_cfg):
    arr = _recording(rows=3500, seed=4)
    codec = ProjectOracleCodec(n_lanes=1, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    x = r[:]
    rs = np.random.RandomState(5)
    for channels, cols in [(2, [2]), (-1, [5]), (slice(1, None, 2), [1, 3, 5]), ([4, 0, 3, 1, 5, 2], [4, 0, 3, 1, 5, 2]), ([4, 0, 0, -2], [4, 0, 0, 4])]:
        w = rs.randn(len(cols), 3)
        off = rs.randn(len(cols))
        assert_same_bits(r.project(w, 200, 3200, channels=channels, offset=off), project_chain(x[200:3200][:, cols], off, w, np.float32))
        y1 = r.project(w[:, 0], 200, 3200, channels=channels, offset=2.5)            # 1-D weights: one output, a 1-D result
        assert y1.shape == (3000,)
        assert_same_bits(y1, project_chain(x[200:3200][:, cols], np.full(len(cols), 2.5), w[:, :1], np.float32)[:, 0])
    assert r.project(np.ones(6), 5, 5).shape == (0,)
    n = len(codec.project_calls)
    z = r.project(np.zeros((0, 3)), channels=[])                                       # no columns: zeros, without a device call
    assert z.shape == (3500, 3) and not z.any() and len(codec.project_calls) == n
    assert r.project(np.ones(6), 7, 7).shape == (0,) and len(codec.project_calls) == n # an empty range: no device call either
    # the uses the call is for: selecting and scaling, common-average reference
    sel = np.zeros((6, 2))
    sel[1, 0], sel[4, 1] = 2.0, -0.5
    assert np.array_equal(r.project(sel, dtype=np.float64), x[:, [1, 4]] * np.array([2.0, -0.5]))
    car = r.project(np.eye(6) - 1.0 / 6, dtype=np.float64)
    assert np.allclose(car, x - x.mean(axis=1, keepdims=True), rtol=0, atol=1e-9)
    r.close()


@pytest.mark.parametrize('n_lanes', [2, 3])
def test_lanes_give_identical_bytes(tmp_cfg, n_lanes):
    arr = _recording(rows=7000, seed=2, dtype=np.float32)
    arr[1234, 2] = np.nan
    one = _write(tmp_cfg, arr, ProjectOracleCodec(n_lanes=1, capacity_chunks=8))
    codec = ProjectOracleCodec(n_lanes=n_lanes, capacity_chunks=8)
    many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    w = np.random.RandomState(3).randn(6, 5)
    for dtype in (np.float32, np.float64):
        a, b = one.project(w, 10, 6990, offset=1.5, dtype=dtype), many.project(w, 10, 6990, offset=1.5, dtype=dtype)
        assert a.tobytes() == b.tobytes()
    assert {lane for lane, *_ in codec.project_calls} == set(range(n_lanes))
    for lane, keys, _, a, b in codec.project_calls:                  # a lane reads the adjacent chunks of its rows and no others
        assert keys == list(range(keys[0], keys[-1] + 1))
        assert many.chunk_bounds[keys[0]] <= a < many.chunk_bounds[keys[0] + 1] and many.chunk_bounds[keys[-1]] < b <= many.chunk_bounds[keys[-1] + 1]


def test_small_call_and_out_bytes_give_identical_bytes(tmp_cfg, monkeypatch):
    arr = _recording(rows=9000, seed=3)
    codec = ProjectOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    w = np.random.RandomState(4).randn(6, 3)
    want = r.project(w, 500, 8700)
    codec.project_calls.clear()
    monkeypatch.setattr(api, 'PROJECT_CALL_BYTES', 1)
    got = r.project(w, 500, 8700)
    assert got.tobytes() == want.tobytes()
    assert len(codec.project_calls) >= 9                            # a round of calls per chunk
    monkeypatch.setattr(api, 'PROJECT_CALL_BYTES', 1 << 30)
    codec.project_calls.clear()
    monkeypatch.setattr(api, 'PROJECT_OUT_BYTES', 700 * 3 * 4)      # 700 rows of the result per round
    got = r.project(w, 500, 8700)
    assert got.tobytes() == want.tobytes()
    assert len(codec.project_calls) >= 12 and max(b - a for *_, a, b in codec.project_calls) <= 700
    r.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    arr = _recording(rows=6000, nc=4, seed=7)
    codec = ProjectOracleCodec(n_lanes=1, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    cache = r._cache_for(0)
    w = np.random.RandomState(8).randn(4, 4)
    cold = r.project(w)
    assert not codec.caches[cache]                                  # a scan inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    codec.project_calls.clear()
    warm = r.project(w)
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens, _, _), = codec.project_calls
    assert [k for k, n in zip(keys, lens) if n == 0] == resident
    assert warm.tobytes() == cold.tobytes()
    codec.miss_next_project = True                                  # an entry dropped between the query and the call: sent whole
    assert r.project(w).tobytes() == cold.tobytes()
    r.close()


def test_damaged_chunk_raises(tmp_cfg):
    arr = _recording(rows=5000, nc=4, seed=8)
    codec = ProjectOracleCodec(n_lanes=2, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    r.close()
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    ch = r.chunk_offsets
    data[ch[3] + 20:ch[3] + 40] = b'\xff' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    w = np.ones((4, 2))
    with pytest.raises(IOError, match='#3'):
        r.project(w, 0, 3001)
    r.project(w, 0, 3000)                                           # (no halo: the rows before chunk 3 do not read it)
    r.project(w, 4000, None)
    r.close()


def test_argument_errors(tmp_cfg):
    arr = _recording(rows=2000, nc=3, seed=9)
    codec = ProjectOracleCodec(n_lanes=1, capacity_chunks=8)
    r = _write(tmp_cfg, arr, codec)
    ok = np.ones((3, 2))
    for bad in (np.ones((2, 2)), np.ones((4, 2)), np.ones(2), np.ones((3, 2, 1)), np.float64(1.0), np.ones((3, 0)), np.ones((3, 1025)),
                np.array([[1.0, np.nan]] * 3), np.array([[np.inf, 1.0]] * 3), np.array([['a', 'b']] * 3), np.ones((3, 2), complex)):
        with pytest.raises(ValueError):
            r.project(bad)
    for bad in (np.nan, np.inf, [1.0, 2.0], [1.0, np.nan, 0.0], np.ones((3, 1)), 'x'):
        with pytest.raises(ValueError):
            r.project(ok, offset=bad)
    for bad in (np.int16, np.float16, 'complex64', 'nonsense'):
        with pytest.raises(ValueError):
            r.project(ok, dtype=bad)
    with pytest.raises(ValueError):
        r.project(np.ones((1025, 1)), channels=[0] * 1025)
    with pytest.raises(IndexError):
        r.project(np.ones(1), channels=3)
    with pytest.raises(ValueError):
        r.project(ok, channels=slice(None, None, -1))
    assert not codec.project_calls                                  # all of them before the device is touched
    assert r.project(np.ones((1024, 2)), 0, 10, channels=[0, 1] * 512).shape == (10, 2)
    assert r.project(np.ones((3, 1024)), 0, 10).shape == (10, 1024)
    r.close()


def test_needs_a_device_codec(tmp_cfg):
    r = _write(tmp_cfg, _recording(rows=2000, nc=3), OracleCodec())
    with pytest.raises(NotImplementedError):
        r.project(np.ones((3, 1)))
    r.close()
