"""Reader.decimate and mts_decimate / mts_dev_decimate on the MI355X: the FIR kernel against a float64 numpy restatement over the
oracle's decode of every golden file, exact taps, bit-identity across calls, pieces, lanes, the cache and the two entry points,
special float values, a damaged chunk in the halo, argument errors and the configs[1] recording in HBM."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.decimate_oracle import assert_within_bound, fir_decimate, fir_decimate_f64
from tests.test_gpu_window_stats import GOLDEN, CASES, _golden_reader, _hbm_recording, _oracle_decode

pytestmark = pytest.mark.gpu

RATE = 30000


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _check(r, dec, q, start, stop, channels, taps, edge, dtype):
    got = r.decimate(q, start, stop, channels=channels, taps=taps, edge=edge, dtype=dtype)
    n = dec.shape[0]
    i0, i1 = r._validate_index(start, 0), max(r._validate_index(start, 0), r._validate_index(stop, n))
    t = api.decimate_taps(q) if taps is None else np.asarray(taps, np.float64)
    vb, ve = (i0, i1) if edge == 'zeros' else (0, n)
    cols = [channels] if isinstance(channels, int) else list(range(*channels.indices(dec.shape[1]))) if isinstance(channels, slice) else channels
    y64, a = fir_decimate_f64(dec[:, cols], vb, ve, i0 + (t.size - 1) // 2, -(-(i1 - i0) // q), q, t)
    assert got.dtype == dtype
    assert_within_bound(got.reshape(y64.shape), y64, a, t.size, dtype)
    return got


@pytest.mark.parametrize('name', GOLDEN)
def test_golden_files(name, tmp_cfg):
    case = CASES[name]
    r, hdr = _golden_reader(tmp_cfg, case)
    dec = _oracle_decode(case)
    nc, n = hdr['n_channels'], hdr['shape'][0]
    shuffled = [int(c) for c in np.random.RandomState(len(name)).permutation(nc)] + [0, nc - 1, 0]
    even = np.random.RandomState(7).randn(16)
    for q in (2, 3, 12, 97):
        for taps in (None, even):
            for edge, dtype in (('zeros', np.float32), ('recording', np.float64)):
                _check(r, dec, q, 0, None, slice(None), taps, edge, dtype)
        _check(r, dec, q, n // 3, -1, shuffled, even, 'recording', np.float32)
    r.close()


@pytest.mark.parametrize('dtype', ['int8', 'int64', 'uint32', 'uint64', 'uint8', 'uint16', 'int16', 'int32', 'float32', 'float64'])
def test_every_item_type_and_exact_taps(tmp_cfg, dtype):
    rows, nc = 3000, 70
    rs = np.random.RandomState(3)
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 100).astype(dt)
    else:
        info = np.iinfo(dt)
        x = rs.randint(max(info.min, -2 ** 62), min(info.max, 2 ** 62), size=(rows, nc), dtype=np.int64).astype(dt)
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=700., n_channels=nc, dtype=dt, check_after_compress=False)
    r = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False)
    ro = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', codec=OracleCodec(), check_after_decompress=False)
    dec = ro[:]                                                          # the reference: the oracle's decode, not the device's
    ro.close()
    if dt.kind != 'f':
        assert np.array_equal(dec, x)                                    # (integers: the decode is the input)
    for out_dt in (np.float32, np.float64):
        _check(r, dec, 12, 0, None, slice(None), None, 'recording', out_dt)
        # bit for bit against the numpy restatement in the output type
        got = r.decimate(5, 13, 2900, taps=np.random.RandomState(1).randn(9), edge='recording', dtype=out_dt)
        want = fir_decimate(dec, 0, 0, rows, 13 + 4, got.shape[0], 5, np.random.RandomState(1).randn(9), out_dt)
        assert got.tobytes() == want.tobytes()
        if dt.itemsize <= 2 or dt.kind == 'f':
            assert got.dtype == out_dt
            assert np.array_equal(r.decimate(3, 7, 2999, taps=[1.0], dtype=out_dt), dec[7:2999:3].astype(out_dt))
            y = r.decimate(3, 7, 2999, taps=[0, 0, 1], dtype=out_dt)
            want = np.vstack([np.zeros((1, nc)), dec[9:2999:3]]).astype(out_dt)[:y.shape[0]]
            assert np.array_equal(y, want)
    r.close()


def _tiny(tmp_cfg, nc=40, rows=8 * 5000, dtype='int16', seed=4):
    x = synth_int16(0, rows, nc, seed).astype(dtype)
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=5000., n_channels=nc, dtype=dtype, check_after_compress=False)
    return x


def _open(tmp_cfg, **kw):
    return mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, **kw)


def test_bit_identity_calls_lanes_cache_and_repeats(tmp_cfg, monkeypatch):
    x = _tiny(tmp_cfg)
    one, two = _open(tmp_cfg, codec=api.HipCodec(devices=[0])), _open(tmp_cfg, codec=api.HipCodec(devices=[0, 0]))
    want = one.decimate(12, 0, None, edge='recording')
    assert want.tobytes() == one.decimate(12, 0, None, edge='recording').tobytes()                 # the same call twice
    assert two.decimate(12, 0, None, edge='recording').tobytes() == want.tobytes()                 # one device == two lanes
    stitched = np.concatenate([one.decimate(12, a, b, edge='recording') for a, b in [(0, 4800), (4800, 4812), (4812, 40000)]])
    assert stitched.tobytes() == want.tobytes()                                                    # one call == many
    monkeypatch.setattr(api, 'DECIMATE_CALL_BYTES', 1)
    assert one.decimate(12, 0, None, edge='recording').tobytes() == want.tobytes()
    monkeypatch.setattr(api, 'DECIMATE_CALL_BYTES', 1 << 30)
    keys = list(range(one.n_chunks))
    one[:]                                                                                         # (read-ahead makes chunks resident)
    for k in range(one.n_chunks):
        one[one.chunk_bounds[k]:one.chunk_bounds[k] + 1]
    cache = one._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 40 for b in before) >= len(keys) // 2
    assert one.decimate(12, 0, None, edge='recording').tobytes() == want.tobytes()                 # resident == cold
    assert hip.cache_query(cache, keys).tolist() == before
    one.close()
    two.close()
    y64, a = fir_decimate_f64(x, 0, x.shape[0], 120, want.shape[0], 12, api.decimate_taps(12))
    assert_within_bound(want, y64, a, 241, np.float32)


def test_pipe_bytes_do_not_change_the_result(tmp_cfg):
    _tiny(tmp_cfg)
    script = ("import sys, numpy as np, mtscomp_amd; sys.path.insert(0, %r); "
              "r = mtscomp_amd.decompress(%r, %r, check_after_decompress=False); "
              "np.save(sys.argv[1], r.decimate(12, 33, None, edge='recording'))") % (os.getcwd(), str(tmp_cfg / 'd.cbin'), str(tmp_cfg / 'd.ch'))
    outs = []
    for pipe in (None, str(200 * 1024)):
        env = dict(os.environ)
        env.pop('MTS_PIPE_BYTES', None)
        if pipe:
            env['MTS_PIPE_BYTES'] = pipe
        p = tmp_cfg / ('o%d.npy' % len(outs))
        subprocess.run([sys.executable, '-c', script, str(p)], env=env, check=True, timeout=300)
        outs.append(np.load(p))
    assert outs[0].tobytes() == outs[1].tobytes()


def test_cache_unchanged_by_a_scan(tmp_cfg):
    _tiny(tmp_cfg, nc=64, rows=6 * RATE // 6)
    r = _open(tmp_cfg)
    keys = list(range(r.n_chunks))
    r[r.chunk_bounds[1] + 5:r.chunk_bounds[1] + 10]
    cache = r._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    r.decimate(12)
    assert hip.cache_query(cache, keys).tolist() == before
    r.close()


def test_damaged_chunk_in_the_halo(tmp_cfg):
    _tiny(tmp_cfg, nc=16, rows=5 * 3000)
    r = _open(tmp_cfg)
    b, o = r.chunk_bounds, r.chunk_offsets
    r.close()
    data = bytearray((tmp_cfg / 'd.cbin').read_bytes())
    data[o[2] + 30:o[2] + 60] = b'\x00' * 30
    (tmp_cfg / 'd.cbin').write_bytes(bytes(data))
    r = _open(tmp_cfg)
    # stop = b[2] - 50: every row of [start, stop) lies in chunks 0 and 1; the last output's newest row (start + k q + half, half =
    # 120) is b[2] + 48, so only the halo reaches chunk 2
    assert 120 + (-(-(b[2] - 50) // 12) - 1) * 12 >= b[2]
    with pytest.raises(IOError, match='#2'):
        r.decimate(12, 0, b[2] - 50, edge='recording')
    r.decimate(12, 0, b[2] - 50, edge='zeros')                     # (the same range without the halo beyond it: fine)
    r.decimate(12, 0, b[2] - 120, edge='recording')
    r.close()


def test_special_float_values(tmp_cfg):
    rows, nc = 4000, 5
    x = (np.random.RandomState(1).randn(rows, nc) * 10).astype(np.float32)
    x[510, 1] = np.nan
    x[1100, 2] = np.inf
    raw = tmp_cfg / 'f.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'f.cbin', tmp_cfg / 'f.ch', sample_rate=1000., n_channels=nc, dtype=np.float32,
                         do_time_diff=False, check_after_compress=False)
    r = mtscomp_amd.decompress(tmp_cfg / 'f.cbin', tmp_cfg / 'f.ch', check_after_decompress=False)
    taps = np.array([0.5, 0.0, 0.25])
    y = r.decimate(2, taps=taps)
    want = fir_decimate(x, 0, 0, rows, 1, y.shape[0], 2, taps, np.float32)
    assert np.array_equal(y, want, equal_nan=True)
    assert np.isnan(y[:, 1]).sum() == 1 and np.isnan(y[550, 2])         # NaN and inf * 0 propagate as numpy does (rows 2k + 1 - j)
    r.close()


def test_device_entry_equals_host_entry_and_config1():
    nc = 385
    raw, cbuf, slots, sizes, bounds = _hbm_recording(nc=nc)
    x = raw.download(dtype=np.int16).reshape(-1, nc)
    n = x.shape[0]
    flags = hip.make_flags(True, False, 'F')
    rows = np.diff(bounds)
    taps = api.decimate_taps(12)
    n_out = n // 12
    st, got, _ = hip.dev_decimate(cbuf, slots, sizes, bounds[:-1], rows, nc, np.int16, flags, 0, n, 120, n_out, 12, taps, np.float32, np.arange(nc))
    assert st == [0] * len(rows)
    sel = slice(None, None, 97)                                          # every 97th output: the reference at 1/97 of the cost
    y64, a = fir_decimate_f64(x, 0, n, 120, got[sel].shape[0], 12 * 97, taps)
    assert_within_bound(got[sel], y64, a, taps.size, np.float32)
    # the host entry on the same chunks (a part of them): the same bits
    host = cbuf.download()
    keep = np.arange(10, 14)
    fr = bounds[10] + 500 * 12 + 120
    st_h, y_h = hip.decimate(0, keep, bounds[keep], host, slots[keep], sizes[keep], rows[keep], nc, np.int16, flags, 0, n, fr, 5000, 12, taps,
                             np.float32, np.arange(nc))
    st_d, y_d, _ = hip.dev_decimate(cbuf, slots[keep], sizes[keep], bounds[keep], rows[keep], nc, np.int16, flags, 0, n, fr, 5000, 12, taps,
                                    np.float32, np.arange(nc))
    assert st_h == st_d == [0] * 4
    assert y_h.tobytes() == y_d.tobytes()
    k0 = (fr - 120) // 12
    assert y_h.tobytes() == got[k0:k0 + 5000].tobytes()


def test_c_abi_argument_errors():
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = np.arange(400, dtype=np.int16).reshape(100, nc)
    z = hip.compress_chunks(x, [0, 100], hip.make_flags(), 6)[0]
    data = np.frombuffer(z + b'\0' * 16, dtype=np.uint8)
    keep = []

    def call(row0=0, rows=100, q=2, taps=(1.0, 0.5), vb=0, ve=100, first_row=1, n_out=50, osz=4, cols=(0, 1), itemsize=2, flags=hip.make_flags()):
        a = [np.array(v, dtype=np.int64) for v in ([0], [row0], [0], [len(z)], [rows])]
        c = np.array(cols, dtype=np.int32)
        t = np.array(taps, dtype=np.float64)
        out = np.zeros(1 << 16, np.uint8)
        st = np.full(1, 99, np.int32)
        keep.append((a, c, t, out, st))
        rc = L.mts_decimate(0, 0, 1, a[0].ctypes.data_as(C.POINTER(C.c_long)), a[1].ctypes.data_as(C.POINTER(C.c_long)), data.ctypes.data_as(C.c_void_p),
                            a[2].ctypes.data_as(C.POINTER(C.c_long)), a[3].ctypes.data_as(C.POINTER(C.c_long)), a[4].ctypes.data_as(C.POINTER(C.c_long)),
                            nc, itemsize, flags, vb, ve, first_row, n_out, q, len(t), t.ctypes.data_as(C.POINTER(C.c_double)), osz, len(c),
                            c.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.POINTER(C.c_int)))
        return rc, st[0]
    assert call() == (0, 0)
    for bad in (dict(q=0), dict(taps=()), dict(taps=(np.nan,)), dict(taps=(np.inf, 1.0)), dict(taps=np.ones(8193)), dict(osz=2),
                dict(cols=(0, 4)), dict(cols=(-1,)), dict(cols=()), dict(row0=10), dict(rows=50), dict(n_out=-1), dict(itemsize=3),
                dict(flags=hip.FLAG_FLOAT, itemsize=2), dict(vb=50, ve=20)):
        rc, st = call(**bad)
        assert rc == -1, bad                                       # MTS_E_ARG ...
        assert st == 99, bad                                       # ... before anything ran


def test_dev_c_abi_argument_errors():
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = np.arange(400, dtype=np.int16).reshape(100, nc)
    z = hip.compress_chunks(x, [0, 100], hip.make_flags(), 6)[0]
    cbuf = hip.DevBuffer(len(z) + 256)
    host = np.frombuffer(z + b'\0' * 256, dtype=np.uint8).copy()
    hip._check(L.mts_dev_copy(0, None, cbuf.at(), hip._ptr(host), host.nbytes, 0), 'mts_dev_copy')
    out = hip.DevBuffer(1 << 16)
    keep = []

    def call(row0=0, rows=100, q=2, taps=(1.0, 0.5), vb=0, ve=100, first_row=1, n_out=50, osz=4, cols=(0, 1), itemsize=2, flags=hip.make_flags(),
             d_out=True):
        a = [np.array(v, dtype=np.int64) for v in ([0], [len(z)], [row0], [rows])]
        c = np.array(cols, dtype=np.int32)
        t = np.array(taps, dtype=np.float64)
        st = np.full(1, 99, np.int32)
        keep.append((a, c, t, st))
        lp = [v.ctypes.data_as(C.POINTER(C.c_long)) for v in a]
        rc = L.mts_dev_decimate(0, None, cbuf.at(), lp[0], lp[1], lp[2], lp[3], 1, nc, itemsize, flags, vb, ve, first_row, n_out, q, len(t),
                                t.ctypes.data_as(C.POINTER(C.c_double)), osz, len(c), c.ctypes.data_as(C.POINTER(C.c_int)),
                                out.at() if d_out else None, st.ctypes.data_as(C.POINTER(C.c_int)))
        return rc, st[0]
    assert call() == (0, 0)
    got = np.empty((50, 2), np.float32)
    hip._check(L.mts_dev_copy(0, None, hip._ptr(got), out.at(), got.nbytes, 1), 'mts_dev_copy')
    xf = x[:, :2].astype(np.float32)
    assert np.array_equal(got, (np.float32(0) + np.float32(1.0) * xf[1::2]) + np.float32(0.5) * xf[0::2])     # rows 2k + 1 - j
    for bad in (dict(q=0), dict(taps=()), dict(taps=(np.nan,)), dict(taps=np.ones(8193)), dict(osz=2), dict(cols=(0, 4)), dict(cols=()),
                dict(row0=10), dict(rows=50), dict(n_out=-1), dict(itemsize=3), dict(flags=hip.FLAG_FLOAT, itemsize=2), dict(vb=50, ve=20),
                dict(d_out=False)):
        rc, st = call(**bad)
        assert rc == -1, bad
        assert st == 99, bad
    out.free()
    cbuf.free()
