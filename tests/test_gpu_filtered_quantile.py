"""Reader.quantile / median / mad(taps=, reference=) and mts_filtered_rank_hist / mts_dev_filtered_rank_hist on the MI355X: k_zrank_hist
and its slab loop against tests/filtered_select_oracle.py (z of tests/detect_oracle.py ordered by tests/select_oracle.py).  Recordings of
3 H + 1234 rows (H = hip.ZRANK_BLOCK_ROWS, the rows of a workgroup) in chunks of 5000, so that chunk and window boundaries fall inside
blocks; column counts around the wave width; windows around H; the three key modes; a constant, a two-valued and a ramp column; special
floats; slab and piece seams; residency; the device entry; count ranges; argument errors.  Every comparison is exact: histograms and
keys by bytes, quantiles by value."""
import ctypes as C
import functools

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.filtered_select_oracle import filtered_round, z_rows
from tests.select_oracle import S, check_quantile, np_mad, np_median, same_values

pytestmark = pytest.mark.gpu

E_ARG = -1
H = hip.ZRANK_BLOCK_ROWS
ROWS, NC, CHUNK = 3 * H + 1234, 385, 5000
HP = api.highpass_taps(300, 30000)                                      # 101 taps
TAPS = {1: [1.0], 2: [0.75, -0.25], 101: HP}


def _int16_recording():
    rs = np.random.RandomState(1)
    x = (rs.randn(ROWS, NC) * 900 + rs.randn(NC) * 3000).clip(-32768, 32767).astype(np.int16)
    x[:, 0] = -1234                                                     # a constant column: all waves meet on one counter
    x[:, 1] = np.where(rs.rand(ROWS) < 0.5, -7, 300)                    # two values
    x[:, 2] = np.arange(ROWS) % 1000 - 500                              # a ramp
    return x


def _float_recording():
    rs = np.random.RandomState(6)
    x = (rs.randn(H + 1234, 9) * 10).astype(np.float32)
    x[1000, 1] = np.nan
    x[4200, 1] = -np.nan
    x[3000, 2] = np.inf
    x[4500, 3] = -np.inf
    x[:, 5] = 0
    x[::2, 5] = -0.0
    x[:, 6] = np.where(rs.rand(len(x)) < 0.5, -0.0, 0.0)
    x[7, 6], x[8, 6] = np.finfo(np.float32).tiny / 4, -np.finfo(np.float32).max
    x[:, 7] = np.float32(1e-41) * rs.randint(-50, 50, len(x)).astype(np.float32)        # denormals
    x[:, 8] = np.float32(2.5)
    return x


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """The two recordings, written once: name -> (directory, the array)."""
    out = {}
    for name, x, kw in (('int16', _int16_recording(), {}), ('float32', _float_recording(), dict(do_time_diff=False))):
        d = tmp_path_factory.mktemp(name)
        x.tofile(d / 'd.bin')
        _compress(d, x, kw)
        out[name] = (d, x)
    return out


def _compress(d, x, kw):
    """(a module fixture cannot take monkeypatch: the config path is set and put back by hand)"""
    api.CONFIG_PATH, keep = d / '.mtscomp', api.CONFIG_PATH
    try:
        mtscomp_amd.compress(d / 'd.bin', d / 'd.cbin', d / 'd.ch', sample_rate=float(CHUNK), n_channels=x.shape[1], dtype=x.dtype,
                             chunk_duration=1.0, check_after_compress=False, **kw)
    finally:
        api.CONFIG_PATH = keep


@pytest.fixture
def cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)


def _open(d, codec=None):
    return mtscomp_amd.decompress(d / 'd.cbin', d / 'd.ch', codec=codec, check_after_decompress=False)


_Z = {}


def _z(name, x, cols, n_taps, reference):
    """The oracle's z of the whole recording over `cols`, computed once per (recording, columns, taps, reference) and left unchanged."""
    key = (name, tuple(cols), n_taps, bool(reference))
    if key not in _Z:
        _Z[key] = z_rows(x[:, list(cols)], 0, 0, len(x), 0, len(x), TAPS[n_taps], 1 if reference else 0)
        _Z[key].setflags(write=False)
    return _Z[key]


def _check(r, z, start, stop, window, cols, n_taps, reference, q=(0.0, 0.5, 1.0), modes=(0, 1, 2), method='linear'):
    """quantile in the key modes asked for (a center per cell), then median and mad, of rows [start, stop) against z."""
    kw = dict(channels=list(cols), window=window, taps=TAPS[n_taps], reference=reference)
    n_win = 1 if window is None else -(-(stop - start) // window)
    cen = np.random.RandomState(len(cols) + n_win).randn(n_win, len(cols)) * 40
    for mode in modes:
        more = {} if mode == 0 else dict(center=cen, absolute=mode == 2)
        got = r.quantile(list(q), start, stop, method=method, **kw, **more)
        assert got.lower.dtype == (np.float64 if mode else np.float32)
        check_quantile(got, z, start, stop, window, q, method, mode=mode, center=cen if mode else None)
    if 0 in modes:
        got = r.mad(start, stop, **kw)
        assert same_values(got.center, np_median(z, start, stop, window)) and same_values(got.mad, np_mad(z, start, stop, window))
        assert same_values(r.median(start, stop, **kw), got.center)


@pytest.mark.parametrize('k', [1, 63, 64, 65, 385])
def test_column_counts_taps_and_reference(files, cfg, k):
    """1, 2 (even) and 101 taps, the median reference off and on, over column sets around the wave width -- the last group of 385
    has one lane -- holding the constant, the two-valued and the ramp column; start is no multiple of the chunk or H."""
    d, x = files['int16']
    rs = np.random.RandomState(k)
    cols = ([0, 1, 2] + sorted(rs.choice(np.arange(3, NC), max(k - 3, 0), replace=False).tolist()))[:k] if k < NC else list(range(NC))
    r = _open(d)
    cases = [(1, None), (2, 'median'), (101, 'median')] if k == NC else [(n, ref) for n in (1, 2, 101) for ref in (None, 'median')]
    for n_taps, reference in cases:
        z = _z('int16', x, cols, n_taps, reference)
        _check(r, z, 37, ROWS - 11, None, cols, n_taps, reference, modes=(0, 2) if k == NC else (0, 1, 2))
    r.close()


@pytest.mark.parametrize('window', [None, 1, 7, H - 1, H, H + 1, CHUNK, 999])
def test_window_sizes(files, cfg, window):
    """Windows around the rows of a workgroup, a chunk length, a value that divides nothing, and windows of 1 and 7 rows across a
    block boundary (a cell costs a histogram: three columns and no mad for those); start is no multiple of the window, the chunk or H."""
    d, x = files['int16']
    r = _open(d)
    small = window in (1, 7)
    cols = [0, 1, 384] if small else [0, 1, 2, 5, 70, 200, 384]
    start, stop = (CHUNK - 40, CHUNK - 40 + H + 9) if small else (37, ROWS - 11)
    z = _z('int16', x, cols, 2, 'median')
    _check(r, z, start, stop, window, cols, 2, 'median', q=(0.0, 0.3, 1.0), modes=(0,) if window == 1 else (0, 1, 2), method='nearest')
    if window == H:
        _check(r, _z('int16', x, cols, 101, None), 37, ROWS - 11, window, cols, 101, None)
    r.close()


@pytest.mark.parametrize('reference', [None, 'median'])
def test_special_floats(files, cfg, reference):
    """NaN, +-inf, +-0 and denormals in a float32 recording; with the median reference a NaN in a row makes every column's window NaN."""
    d, x = files['float32']
    n = len(x)
    cols = list(range(x.shape[1]))
    r = _open(d)
    assert np.array_equal(r[:], x, equal_nan=True)
    z = _z('float32', x, cols, 1, reference)
    for window in (None, 2000):
        _check(r, z, 0, n, window, cols, 1, reference, q=(0.0, 0.5, 0.9999, 1.0))
    z2 = _z('float32', x, cols, 2, reference)
    _check(r, z2, 3, n - 5, 999, cols, 2, reference)
    med = r.median(window=2000, reference=reference, taps=[1.0])
    if reference:
        assert np.isnan(med[0]).all() and np.isnan(med[2]).all() and np.isfinite(med[1, [0, 1, 4]]).all()      # rows 1000 and 4200 hold a NaN
    else:
        assert np.isnan(med[0, 1]) and np.isfinite(med[:, 0]).all()
    zero = r.quantile(0.5, channels=5, method='lower', taps=[1.0])       # -0 and +0 are one key and come back as +0
    assert zero.lower[0] == 0 and not np.signbit(zero.lower[0])
    r.close()


def _results(r, cols):
    out = []
    for w, lo, hi in ((None, 0, ROWS), (4321, 1234, ROWS - 77)):
        s = r.quantile([0, 0.37, 1], lo, hi, channels=cols, window=w, taps=HP, reference='median')
        m = r.mad(lo, hi, channels=cols, window=w, center=0.0, taps=HP, reference='median')
        out += [s[k].tobytes() for k in ('count', 'quantile', 'lower', 'upper')] + [m.mad.tobytes()]
    return out


def test_seams_residency_and_lanes_do_not_change_a_bit(files, cfg, monkeypatch):
    """Slabs that own fewer rows than a window and than a block, pieces of one chunk, sub-batches of one chunk, calls of one chunk, two
    lanes, resident chunks: the same bytes as the default plan, and right by the oracle.  A scan inserts nothing."""
    d, x = files['int16']
    cols = [0, 1, 2] + list(range(100, 140))
    r = _open(d, api.HipCodec(devices=[0]))
    keys = list(range(r.n_chunks))
    cache = r._cache_for(0)
    base = _results(r, cols)
    assert not any(hip.cache_query(cache, keys).tolist())               # a scan inserts nothing
    z = _z('int16', x, cols, 101, 'median')
    got = r.quantile([0, 0.37, 1], 1234, ROWS - 77, channels=cols, window=4321, taps=HP, reference='median')
    check_quantile(got, z, 1234, ROWS - 77, 4321, [0, 0.37, 1], 'linear')
    row_bytes = 4 * len(cols)
    for slab_rows in (1000, H + 100):                                   # fewer rows than a window and a block; a block and a bit
        monkeypatch.setenv('MTS_ZRANK_SLAB_BYTES', str(slab_rows * row_bytes))
        assert _results(r, cols) == base, slab_rows
    monkeypatch.setenv('MTS_PIPE_BYTES', str(CHUNK * NC * 2))           # pieces of one chunk
    monkeypatch.setenv('MTS_BATCH_BYTES', str(1 << 20))                 # ... decoded in sub-batches of one chunk
    assert _results(r, cols) == base
    monkeypatch.setenv('MTS_ZRANK_SLAB_BYTES', str(7 * row_bytes))      # seven rows a slab, on a short range
    short = r.quantile(0.5, CHUNK - 300, CHUNK + 300, channels=cols, window=250, taps=HP, reference='median')
    for name in ('MTS_ZRANK_SLAB_BYTES', 'MTS_PIPE_BYTES', 'MTS_BATCH_BYTES'):
        monkeypatch.delenv(name)
    want = r.quantile(0.5, CHUNK - 300, CHUNK + 300, channels=cols, window=250, taps=HP, reference='median')
    assert short.quantile.tobytes() == want.quantile.tobytes() and short.lower.tobytes() == want.lower.tobytes()
    monkeypatch.setattr(api, 'QUANTILE_CALL_BYTES', 1)                  # a call per chunk
    assert _results(r, cols) == base
    monkeypatch.setattr(api, 'QUANTILE_CALL_BYTES', 1 << 30)
    two = _open(d, api.HipCodec(devices=[0, 0]))                        # two lanes on one device
    assert _results(two, cols) == base
    two.close()
    # resident against cold
    r[CHUNK + 5:CHUNK + 10]
    before = hip.cache_query(cache, keys).tolist()
    assert before[1] == NC
    assert _results(r, cols) == base
    assert hip.cache_query(cache, keys).tolist() == before
    r.close()


def _table(r, d):
    data = (d / 'd.cbin').read_bytes()
    offs, lens, bounds = np.array(r.chunk_offsets[:-1]), np.diff(r.chunk_offsets), np.array(r.chunk_bounds)
    return data, offs, lens, bounds


def _selectors(z, nw, mode, rs):
    """Selector 0: every item at the top digit; selector 1: one digit down under the top digit of an item of the column."""
    kb, C_ = (64 if mode else 32), z.shape[1]
    cen = rs.randn(nw, C_) * 40 if mode else None
    pref = np.zeros((nw, S, C_), np.uint64)
    shift = np.zeros((nw, S, C_), np.int32)
    shift[:, 0], shift[:, 1] = kb - 8, kb - 16
    pick = z[rs.randint(0, len(z), size=(nw, C_)), np.arange(C_)[None, :]]
    pref[:, 1] = hip.rank_keys(pick, mode, cen) >> np.uint64(kb - 8)
    return cen, pref, shift


def test_c_abi_rounds_counts_and_the_device_entry(files, cfg):
    """One round of the C ABI in the three modes with two active selectors against the oracle by bytes; a count range that is a strict
    sub-range of the grid; the sums over a partition of the range equal the whole; mts_dev_filtered_rank_hist equals the host entry
    byte for byte; resident chunks without bytes equal the cold call and a chunk that is not resident is a miss."""
    d, x = files['int16']
    r = _open(d, api.HipCodec(devices=[0]))
    data, offs, lens, bounds = _table(r, d)
    keys = list(range(r.n_chunks))
    cols = [0, 1, 2] + list(range(300, 364))                            # 67 columns: a second group of three lanes
    taps, flags = np.asarray(TAPS[2]), r._flags()
    z = _z('int16', x, cols, 2, 'median')
    rs = np.random.RandomState(12)
    rb, re, window = 37, ROWS - 11, H + 1
    nw = -(-(re - rb) // window)
    head = (keys, bounds[:-1], data, offs, lens, np.diff(bounds), NC, np.int16, flags)
    cbuf = hip.DevBuffer(len(data) + 256)
    cbuf.upload(np.frombuffer(data, np.uint8))
    dev_head = (cbuf, offs, lens, bounds[:-1], np.diff(bounds), NC, np.int16, flags)
    out = None
    for mode in (0, 1, 2):
        cen, pref, shift = _selectors(z, nw, mode, rs)
        mid = (0, ROWS, taps, cols, 1, rb, re, window)
        sel = (mode, cen, pref, shift)

        def want(cb, ce):
            return filtered_round(x[:, cols], 0, 0, ROWS, taps, 1, rb, re, window, cb, ce, mode, cen, pref, shift.astype(np.int64))

        def same(got, ref):
            for key, w in zip(('hist', 'kmin', 'kmax', 'count'), ref):
                assert got[key].tobytes() == w.tobytes() and got[key].dtype == w.dtype, (mode, key)
        st, whole = hip.filtered_rank_hist(0, *head, *mid, rb, re, *sel)
        assert st == [0] * len(keys)
        same(whole, want(rb, re))
        cuts = [rb, rb + 1, H + 5, CHUNK, CHUNK + 1, 2 * H + 77, re]    # a strict sub-range each; together a partition
        parts = []
        for cb, ce in zip(cuts[:-1], cuts[1:]):
            st, got = hip.filtered_rank_hist(0, *head, *mid, cb, ce, *sel)
            assert st == [0] * len(keys)
            if mode == 0 or ce - cb < 200:
                same(got, want(cb, ce))
            parts.append(got)
        assert sum(p['hist'].astype(np.uint64) for p in parts).astype(np.uint32).tobytes() == whole['hist'].tobytes()
        assert functools.reduce(np.minimum, [p['kmin'] for p in parts]).tobytes() == whole['kmin'].tobytes()
        assert functools.reduce(np.maximum, [p['kmax'] for p in parts]).tobytes() == whole['kmax'].tobytes()
        assert sum(p['count'] for p in parts).tolist() == whole['count'].tolist()
        st, empty = hip.filtered_rank_hist(0, *head, *mid, CHUNK, CHUNK, *sel)          # nothing to count: the identities
        same(empty, want(CHUNK, CHUNK))
        # the device entry, the whole range and a sub-range
        for cb, ce in ((rb, re), (H + 5, CHUNK + 1)):
            st, got, out = hip.dev_filtered_rank_hist(*dev_head, *mid, cb, ce, *sel, out=out)
            assert st == [0] * len(keys)
            same(got, want(cb, ce) if (cb, ce) != (rb, re) else [whole[k] for k in ('hist', 'kmin', 'kmax', 'count')])
    # a call with exactly the chunks of its support: two taps read rows t - 1 and t, so chunk 1's rows need the last row of chunk 0
    cb, ce = CHUNK, 2 * CHUNK
    k1 = [0, 1]
    h1 = (k1, bounds[k1], data, offs[k1], lens[k1], np.diff(bounds)[k1], NC, np.int16, flags)
    cen, pref, shift = _selectors(z, nw, 0, rs)
    st, got = hip.filtered_rank_hist(0, *h1, 0, ROWS, taps, cols, 1, rb, re, window, cb, ce, 0, None, pref, shift)
    assert st == [0, 0]
    ref = filtered_round(x[:, cols], 0, 0, ROWS, taps, 1, rb, re, window, cb, ce, 0, None, pref, shift.astype(np.int64))
    assert got['hist'].tobytes() == ref[0].tobytes() and got['count'].tolist() == ref[3].tolist()
    # resident chunks go without bytes; one that is not resident is a miss
    cache = r._cache_for(0)
    r[CHUNK + 5:CHUNK + 10]
    before = hip.cache_query(cache, keys).tolist()
    assert before[1] == NC
    lens_w = np.where(np.array(before) > 0, 0, lens)
    args = (0, ROWS, taps, cols, 1, rb, re, window, rb, re, 0, None, pref, shift)
    st_w, a = hip.filtered_rank_hist(cache, keys, bounds[:-1], data, offs, lens_w, *head[5:], *args)
    st_c, b = hip.filtered_rank_hist(0, *head, *args)
    assert st_w == st_c == [0] * len(keys)
    for key in ('hist', 'kmin', 'kmax', 'count'):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert hip.cache_query(cache, keys).tolist() == before
    if not all(before):
        lens_bad = lens_w.copy()
        lens_bad[[k for k in keys if not before[k]][0]] = 0
        with pytest.raises(hip.HipError) as e:
            hip.filtered_rank_hist(cache, keys, bounds[:-1], data, offs, lens_bad, *head[5:], *args)
        assert e.value.code == hip.E_MISS
    cbuf.free()
    r.close()


def test_damaged_chunk(files, cfg, tmp_path):
    """A bad adler32 that the decoder reports: the IOError of Reader[...] wherever the chunk is in the support, the status in the C ABI."""
    d, x = files['int16']
    r = _open(d)
    data = bytearray((d / 'd.cbin').read_bytes())
    o = r.chunk_offsets
    r.close()
    data[o[2] - 4:o[2]] = bytes(b ^ 0x55 for b in data[o[2] - 4:o[2]])          # the adler32 of chunk 1
    (tmp_path / 'd.cbin').write_bytes(bytes(data))
    (tmp_path / 'd.ch').write_bytes((d / 'd.ch').read_bytes())
    r = _open(tmp_path)
    cols = [0, 5, 9]
    for call in (lambda: r.median(channels=cols, taps=HP), lambda: r.quantile(0.3, channels=cols, window=1000, reference='median'),
                 lambda: r.mad(channels=cols, center=0.0, taps=HP), lambda: r.median(CHUNK - 30, CHUNK - 5, channels=cols, taps=HP),
                 lambda: r.median(2 * CHUNK + 5, 2 * CHUNK + 30, channels=cols, taps=HP)):       # (the last two: chunk 1 in the halo only)
        with pytest.raises(IOError, match='#1'):
            call()
    assert same_values(r.median(0, CHUNK - 60, channels=cols, taps=HP), np_median(_z('int16', x, cols, 101, None), 0, CHUNK - 60, None))
    bounds = np.array(r.chunk_bounds)
    pref = np.zeros((1, S, 3), np.uint64)
    shift = np.full((1, S, 3), 24, np.int32)
    st, _ = hip.filtered_rank_hist(0, range(3), bounds[:-1], bytes(data), o[:-1], np.diff(o), np.diff(bounds), NC, np.int16, r._flags(), 0, ROWS,
                                   HP, cols, 0, 0, ROWS, ROWS, 0, ROWS, 0, None, pref, shift)
    assert st == [0, hip.CHUNK_CORRUPT, 0]
    r.close()


def test_end_to_end_noise_level_and_detect(files, cfg):
    """mad(center=0.0, taps=hp, reference='median') is np_mad of the oracle's z, and detect runs with the threshold made of it."""
    d, x = files['int16']
    cols = list(range(3, 67))
    r = _open(d)
    z = _z('int16', x, cols, 101, 'median')
    noise = r.mad(channels=cols, center=0.0, taps=HP, reference='median')
    assert same_values(noise.mad, np_mad(z, 0, ROWS, None, center=0.0))
    assert noise.reference == 'median' and noise.taps.tobytes() == np.asarray(HP, np.float64).tobytes() and noise.rounds <= 8
    thr = 5 * noise.mad[0] / 0.6745
    assert np.isfinite(thr).all() and (thr > 0).all()
    ev = r.detect(thr, channels=cols, taps=HP, reference='median', exclude=10, spread=2)
    zc = z[ev.sample, np.searchsorted(cols, ev.channel)]
    assert ev.amplitude.tobytes() == zc.tobytes() and (-zc > thr[np.searchsorted(cols, ev.channel)].astype(np.float32)).all()
    r.close()


def test_c_abi_argument_errors():
    """MTS_E_ARG for every argument error, before anything is allocated or launched (the status array is untouched)."""
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = np.arange(800, dtype=np.int16).reshape(200, nc)
    zs = hip.compress_chunks(x, [0, 100, 200], hip.make_flags(), 6)
    data = np.frombuffer(zs[0] + zs[1] + b'\0' * 16, dtype=np.uint8)
    dbuf = hip.DevBuffer(data.size + 256)
    dbuf.upload(data)
    keep = []
    outd = hip.DevBuffer(1 << 22)

    def call(dev, row0=(0, 100), rows=(100, 100), vb=0, ve=200, taps=(0.5, 0.5), n_taps=None, reference=0, rb=0, re=200, window=10, cb=None,
             ce=None, cols=(0, 1), itemsize=2, flags=hip.make_flags(), mode=0, center=True, shift=8, prefix=0):
        a = [np.array(v, dtype=np.int64) for v in ([0, 1], list(row0), [0, len(zs[0])], [len(zs[0]), len(zs[1])], list(rows))]
        c = np.array(cols, dtype=np.int32)
        t = np.array(taps, dtype=np.float64)
        nw = max(-(-(re - rb) // window), 1) if window >= 1 else 1
        pre = np.full((nw, S, max(len(c), 1)), prefix, np.uint64)
        shf = np.full((nw, S, max(len(c), 1)), shift, np.int32)
        cen = np.zeros((nw, max(len(c), 1)))
        oh, ok_, ox = np.zeros(pre.size * 256, np.uint32), np.zeros(pre.size, np.uint64), np.zeros(pre.size, np.uint64)
        cnt = np.zeros(nw, np.int64)
        st = np.full(2, 99, np.int32)
        keep.append((a, c, t, pre, shf, cen, oh, ok_, ox, cnt, st))
        P = lambda v: v.ctypes.data_as(C.POINTER(C.c_long))  # noqa: E731
        U = lambda v: v.ctypes.data_as(C.POINTER(C.c_ulonglong))  # noqa: E731
        I = lambda v: v.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731,E741
        D = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        mid = (vb, ve, len(t) if n_taps is None else n_taps, D(t), len(c), I(c), reference, rb, re, window, rb if cb is None else cb,
               re if ce is None else ce, mode, D(cen) if center else None, U(pre), I(shf))
        if dev:
            rc = L.mts_dev_filtered_rank_hist(0, None, dbuf.at(), P(a[2]), P(a[3]), P(a[1]), P(a[4]), 2, nc, itemsize, flags, *mid, outd.at(),
                                              outd.at(1 << 21), outd.at(3 << 20), P(cnt), I(st))
        else:
            rc = L.mts_filtered_rank_hist(0, 0, 2, P(a[0]), P(a[1]), data.ctypes.data_as(C.c_void_p), P(a[2]), P(a[3]), P(a[4]), nc, itemsize,
                                          flags, *mid, oh.ctypes.data_as(C.POINTER(C.c_uint)), U(ok_), U(ox), P(cnt), I(st))
        return rc, int(st[0])
    for dev in (False, True):
        assert call(dev, shift=24) == (0, 0)
        assert call(dev, rb=30, re=170, cb=41, ce=163, mode=2, shift=56, reference=1) == (0, 0)
        assert call(dev, shift=-1) == (0, 0)
        assert call(dev, cb=50, ce=50, shift=24) == (0, 0)
        for bad in (
                # what mts_detect refuses of its filter arguments
                dict(cols=()), dict(cols=(0, 4)), dict(cols=(-1,)), dict(n_taps=0), dict(n_taps=8193), dict(taps=(1.0, float('nan'))),
                dict(taps=(float('inf'),)), dict(reference=2), dict(reference=-1), dict(reference=1, cols=(0,) * 1025), dict(vb=-1),
                dict(vb=150, ve=100), dict(itemsize=3), dict(flags=hip.FLAG_FLOAT, itemsize=2), dict(row0=(0, 99)), dict(rows=(0, 100)),
                dict(row0=(50, 150)),                                  # (the support is not covered)
                # the grid and the count range
                dict(window=0), dict(window=-3), dict(rb=50, re=20), dict(re=201), dict(vb=10, rb=5), dict(cb=-1), dict(rb=20, cb=19),
                dict(ce=201), dict(re=150, ce=151), dict(cb=80, ce=70),
                # what mts_rank_hist refuses of its selectors, with the key_bits of a float32 item
                dict(mode=3), dict(mode=-1), dict(mode=1, center=False), dict(shift=25), dict(shift=57, mode=1), dict(shift=16, prefix=256),
                dict(shift=24, prefix=1)):
            rc, st = call(dev, **dict(dict(shift=24), **bad))
            assert rc == E_ARG, (dev, bad)                             # MTS_E_ARG ...
            assert st == 99, (dev, bad)                                # ... before anything ran
