"""Reader.window_stats and mts_window_stats / mts_dev_window_stats on the MI355X: the statistics kernels against numpy over
the oracle's decode of the golden files, special float values, the configs[1] recording in HBM, the decoded-chunk cache, lanes,
damaged chunks and argument errors."""
import ctypes as C
import json

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from oracle import oracle as O
from tests.stats_oracle import assert_stats_equal, numpy_window_stats
from tests.test_golden import CASES, golden_cbin

pytestmark = pytest.mark.gpu

RATE = 30000


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _golden_reader(tmp, case, codec=None):
    hdr = json.loads(case['ch_text'])
    p = tmp / (case['name'] + '.cbin')
    p.write_bytes(golden_cbin(case))
    r = mtscomp_amd.Reader(codec=codec, check_after_decompress=False)
    r.open(p, cmeta=hdr)
    return r, hdr


def _oracle_decode(case):
    hdr = json.loads(case['ch_text'])
    data = golden_cbin(case)
    flags = hip.make_flags(hdr['do_time_diff'], hdr['do_spatial_diff'], hdr['chunk_order'])
    b, o = hdr['chunk_bounds'], hdr['chunk_offsets']
    parts = []
    for i in range(len(b) - 1):
        rc, a = O.decompress_chunk(data[o[i]:o[i + 1]], b[i + 1] - b[i], hdr['n_channels'], hdr['dtype'], flags)
        assert rc == 0
        parts.append(a)
    return np.concatenate(parts, axis=0)


GOLDEN = sorted(n for n, c in CASES.items() if golden_cbin(c) is not None)


@pytest.mark.parametrize('name', GOLDEN)
def test_golden_files(name, tmp_cfg):
    case = CASES[name]
    r, hdr = _golden_reader(tmp_cfg, case)
    dec = _oracle_decode(case)
    nc, n = hdr['n_channels'], hdr['shape'][0]
    shuffled = list(np.random.RandomState(len(name)).permutation(nc)) + [0, nc - 1, 0]
    chunk_len = hdr['chunk_bounds'][1] - hdr['chunk_bounds'][0]
    for window in (1, 7, chunk_len, 3001, n + 5, None):
        for channels in (slice(None), slice(1, None, 3), shuffled):
            got = r.window_stats(window, channels=channels)
            cols = list(range(*channels.indices(nc))) if isinstance(channels, slice) else [int(c) for c in channels]
            if not cols:
                continue
            assert_stats_equal(got, numpy_window_stats(dec, window or max(n, 1), 0, n, cols), dec.dtype)
    got = r.window_stats(1000, start=-n // 2, stop=-1, channels=-1)          # (a sub-range, one column squeezed)
    assert_stats_equal(got, numpy_window_stats(dec, 1000, n - n // 2, n - 1, [nc - 1]), dec.dtype, squeeze=True)
    r.close()


def test_special_float_values(tmp_cfg):
    rows, nc, w = 4000, 5, 500
    x = (np.random.RandomState(1).randn(rows, nc) * 10).astype(np.float32)
    x[510, 1] = np.nan                                                   # window 1
    x[1100, 2] = np.inf                                                  # window 2
    x[1600, 3], x[1700, 3] = np.inf, -np.inf                             # window 3: sum is NaN
    x[2000:2500, 4] = -0.0                                               # window 4: min == max == 0
    x[3000:3500, 0] = 0.0
    x[3100, 0] = -0.0
    raw = tmp_cfg / 'f.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'f.cbin', tmp_cfg / 'f.ch', sample_rate=1000., n_channels=nc, dtype=np.float32,
                         do_time_diff=False, check_after_compress=False)
    r = mtscomp_amd.decompress(tmp_cfg / 'f.cbin', tmp_cfg / 'f.ch', check_after_decompress=False)
    assert np.array_equal(r[:], x, equal_nan=True)                       # (no time diff: the values come back as they are)
    got = r.window_stats(w)
    assert_stats_equal(got, numpy_window_stats(x, w, 0, rows, range(nc)), np.float32)
    assert np.isnan(got.min[1, 1]) and np.isnan(got.max[1, 1]) and np.isnan(got.sum[1, 1])
    assert got.max[2, 2] == np.inf and got.sum[2, 2] == np.inf and np.isnan(got.sum[3, 3])
    assert got.min[4, 4] == 0 and got.max[4, 4] == 0 and got.sum[4, 4] == 0
    r.close()


def _hbm_recording(seconds=60, nc=385):
    """configs[1]: 60 s x 385 int16 of the synthetic recording, compressed on the device; the chunks stay in HBM."""
    n, chunk_bytes = seconds, RATE * nc * 2
    raw = hip.DevBuffer(n * chunk_bytes)
    hip.dev_synth_int16(raw, 0, 0, n * RATE, nc, 0)
    cb = (hip.compress_bound(chunk_bytes) + 255) // 256 * 256
    cbuf = hip.DevBuffer(n * cb)
    bounds = np.arange(n + 1, dtype=np.int64) * RATE
    slots = np.arange(n, dtype=np.int64) * cb
    sizes = np.zeros(n, dtype=np.int64)
    hip.dev_compress_chunks(raw, nc, 2, bounds, hip.make_flags(True, False, 'F'), 6, cbuf, slots, sizes)
    return raw, cbuf, slots, sizes, bounds


def test_config1_in_hbm_bit_identical():
    nc = 385
    raw, cbuf, slots, sizes, bounds = _hbm_recording(nc=nc)
    x = raw.download(dtype=np.int16).reshape(-1, nc)
    n = x.shape[0]
    flags = hip.make_flags(True, False, 'F')
    rows = np.diff(bounds)
    out = None
    for window in (30000, 3001):
        st, got, out = hip.dev_window_stats(cbuf, slots, sizes, bounds[:-1], rows, nc, np.int16, flags, 0, n, window, np.arange(nc), out=out)
        assert st == [0] * len(rows)
        want = numpy_window_stats(x, window, 0, n, range(nc))
        assert np.array_equal(got['count'], want['count'])
        for key in ('min', 'max', 'sum'):
            assert np.array_equal(got[key], want[key]), key
        assert got['sumsq'].dtype == np.uint64 and np.array_equal(got['sumsq'].astype(np.float64), want['sumsq'])
    # a window range that starts and ends inside chunks, a shuffled column list, every other chunk (a lane's share)
    cols = np.random.RandomState(2).randint(0, nc, 50)
    keep = np.arange(1, 60, 2)
    st, got, _ = hip.dev_window_stats(cbuf, slots[keep], sizes[keep], bounds[keep], rows[keep], nc, np.int16, flags, 12345, n - 777, 4567, cols)
    want_parts = []
    sel = np.zeros(n, bool)
    for k in keep:
        sel[bounds[k]:bounds[k + 1]] = True
    for w0 in range(12345, n - 777, 4567):
        seg = slice(w0, min(w0 + 4567, n - 777))
        rows_in = x[seg][sel[seg]][:, cols]
        want_parts.append((rows_in.shape[0], rows_in))
    assert got['count'].tolist() == [c for c, _ in want_parts]
    for w, (c, seg) in enumerate(want_parts):
        if c:
            assert np.array_equal(got['min'][w], seg.min(0)) and np.array_equal(got['sum'][w], seg.astype(np.int64).sum(0))
        else:
            assert (got['min'][w] == 32767).all() and (got['max'][w] == -32768).all() and not got['sum'][w].any()


def test_cache_untouched_by_a_scan_and_resident_chunks_read_in_place(tmp_cfg):
    nc, seconds = 64, 6
    x = synth_int16(0, seconds * RATE, nc, 3)
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=float(RATE), n_channels=nc, dtype=np.int16,
                         check_after_compress=False)
    r = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False)
    keys = list(range(seconds))
    r[RATE + 5:RATE + 10]                                               # chunk 1 (and what is read ahead) resident
    cache = r._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert before[1] == nc
    warm = r.window_stats(7000)
    assert hip.cache_query(cache, keys).tolist() == before              # a whole-file scan changes nothing in the cache
    want = numpy_window_stats(x, 7000, 0, x.shape[0], range(nc))
    assert_stats_equal(warm, want, np.int16)
    # resident (c_lengths = 0) against cold: the same results
    data = (tmp_cfg / 'd.cbin').read_bytes()
    offs = np.array(r.chunk_offsets[:-1])
    lens = np.diff(r.chunk_offsets)
    bounds = np.array(r.chunk_bounds)
    flags = r._flags()
    resident = [k for k, p in zip(keys, before) if p]
    lens_w = np.where(np.isin(keys, resident), 0, lens)
    st_w, a = hip.window_stats(cache, keys, bounds[:-1], data, offs, lens_w, np.diff(bounds), nc, np.int16, flags, 0, x.shape[0], 3001, range(nc))
    st_c, b = hip.window_stats(0, keys, bounds[:-1], data, offs, lens, np.diff(bounds), nc, np.int16, flags, 0, x.shape[0], 3001, range(nc))
    assert st_w == st_c == [0] * seconds
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert hip.cache_query(cache, keys).tolist() == before
    # a chunk sent without bytes that is not resident: E_MISS, nothing launched
    cold = [k for k in keys if k not in resident][0]
    lens_bad = lens_w.copy()
    lens_bad[cold] = 0
    with pytest.raises(hip.HipError) as e:
        hip.window_stats(cache, keys, bounds[:-1], data, offs, lens_bad, np.diff(bounds), nc, np.int16, flags, 0, x.shape[0], 3001, range(nc))
    assert e.value.code == hip.E_MISS
    r.close()


@pytest.mark.parametrize('dtype', ['int16', 'float32'])
def test_two_lanes_on_one_device(tmp_cfg, dtype):
    nc, rows = 40, 8 * 5000
    x = synth_int16(0, rows, nc, 4)
    x = x.astype(dtype) * (np.float32(0.37) if dtype == 'float32' else 1)
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=5000., n_channels=nc, dtype=dtype, check_after_compress=False)
    one = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, codec=api.HipCodec(devices=[0]))
    two = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, codec=api.HipCodec(devices=[0, 0]))
    dec = one[:]
    for window in (3001, 5000, None):
        a, b, c = one.window_stats(window), two.window_stats(window), two.window_stats(window)
        assert_stats_equal(b, numpy_window_stats(dec, window or rows, 0, rows, range(nc)), dtype)
        for key in ('count', 'min', 'max', 'sum', 'sumsq', 'mean', 'rms'):
            assert np.array_equal(b[key], c[key], equal_nan=True), key           # the same twice
            if dtype == 'int16':
                assert np.array_equal(a[key], b[key]), key                       # integers: one lane == two, bit for bit
    one.close()
    two.close()


def test_damaged_chunk(tmp_cfg):
    nc, rows = 16, 5 * 3000
    x = synth_int16(0, rows, nc, 5)
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=3000., n_channels=nc, dtype=np.int16, check_after_compress=False)
    hdr = json.loads((tmp_cfg / 'd.ch').read_text())
    o = hdr['chunk_offsets']
    data = bytearray((tmp_cfg / 'd.cbin').read_bytes())
    data[o[2] + 30:o[2] + 60] = b'\x00' * 30
    (tmp_cfg / 'd.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False)
    with pytest.raises(IOError, match='#2'):
        r.window_stats(1000)
    b = np.array(hdr['chunk_bounds'])
    st, res = hip.window_stats(0, range(5), b[:-1], bytes(data), o[:-1], np.diff(o), np.diff(b), nc, np.int16, r._flags(), 0, rows, 1000, range(nc))
    assert st == [0, 0, hip.CHUNK_CORRUPT, 0, 0]                         # only that chunk
    assert res['count'].tolist() == [1000] * 6 + [0] * 3 + [1000] * 6    # its rows count nowhere
    want = numpy_window_stats(x, 1000, 0, rows, range(nc))
    ok = res['count'] > 0
    assert np.array_equal(res['min'][ok], want['min'][ok]) and np.array_equal(res['sum'][ok], want['sum'][ok])
    r.close()


def test_c_abi_argument_errors():
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = np.arange(400, dtype=np.int16).reshape(100, nc)
    z = hip.compress_chunks(x, [0, 100], hip.make_flags(), 6)[0]
    data = np.frombuffer(z + b'\0' * 16, dtype=np.uint8)
    keep = []

    def call(row0=0, rows=100, window=10, rb=0, re=100, cols=(0, 1), itemsize=2, flags=hip.make_flags()):
        a = [np.array(v, dtype=np.int64) for v in ([0], [row0], [0], [len(z)], [rows])]
        c = np.array(cols, dtype=np.int32)
        outs = [np.zeros(4096, np.uint8) for _ in range(4)]
        cnt, st = np.zeros(512, np.int64), np.full(1, 99, np.int32)
        keep.append((a, c, outs, cnt, st))
        rc = L.mts_window_stats(0, 0, 1, a[0].ctypes.data_as(C.POINTER(C.c_long)), a[1].ctypes.data_as(C.POINTER(C.c_long)), data.ctypes.data_as(C.c_void_p),
                                a[2].ctypes.data_as(C.POINTER(C.c_long)), a[3].ctypes.data_as(C.POINTER(C.c_long)), a[4].ctypes.data_as(C.POINTER(C.c_long)),
                                nc, itemsize, flags, rb, re, window, len(c), c.ctypes.data_as(C.POINTER(C.c_int)),
                                *[o.ctypes.data_as(C.c_void_p) for o in outs], cnt.ctypes.data_as(C.POINTER(C.c_long)), st.ctypes.data_as(C.POINTER(C.c_int)))
        return rc, st[0]
    assert call() == (0, 0)
    for bad in (dict(window=0), dict(window=-5), dict(cols=(0, 4)), dict(cols=(-1,)), dict(cols=()), dict(rb=100, re=200),
                dict(rb=50, re=20), dict(row0=1000), dict(itemsize=3), dict(flags=hip.FLAG_FLOAT, itemsize=2),
                dict(rb=0, re=(1 << 31) + 10, window=(1 << 31) + 5)):
        rc, st = call(**bad)
        assert rc == -1, bad                                             # MTS_E_ARG ...
        assert st == 99, bad                                             # ... before anything ran
