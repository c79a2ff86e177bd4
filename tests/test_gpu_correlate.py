"""Reader.correlate and mts_correlate / mts_dev_correlate on the MI355X: the kernel against the numpy restatement of the definition
(tests/correlate_oracle.py) over the oracle's decode, for exact equality of every byte: the column groups and bands, the output tiles,
template lengths and offsets at both ends of the recording, the filter and the reference, item types, special and subnormal values,
bit-identity across the cache, lanes, calls, slabs, pieces and the two entry points, cross-checks against project and detect,
argument errors and a damaged chunk."""
import ctypes as C

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.correlate_oracle import NAN_BITS, correlate
from tests.zfamily_errors import filter_errors, template_errors

pytestmark = pytest.mark.gpu


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _make(tmp, x, rate, **kw):
    """The recording x on disk; -> (Reader on the device, the oracle's decode of the file)."""
    raw = tmp / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'd.cbin', tmp / 'd.ch', sample_rate=float(rate), n_channels=x.shape[1], dtype=x.dtype,
                         check_after_compress=False, do_time_diff=x.dtype.kind != 'f')
    ro = mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', codec=OracleCodec(), check_after_decompress=False)
    dec = ro[:]                                                     # the reference: the oracle's decode, not the device's
    ro.close()
    return _open(tmp, **kw), dec


def _open(tmp, **kw):
    return mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', check_after_decompress=False, **kw)


def _want(dec, k, i0, i1, before, channels=slice(None), taps=None, reference=None):
    cols = np.arange(dec.shape[1])[channels] if isinstance(channels, slice) else np.asarray(channels)
    return correlate(dec[:, cols], 0, 0, dec.shape[0], i0, i1, [1.0] if taps is None else taps, 1 if reference else 0, before, k)


def _check(r, dec, k, i0, i1, before, channels=slice(None), taps=None, reference=None, want=None):
    """Reader.correlate on rows [i0, i1) against the definition (or the rows of `want`, the definition over the whole file)."""
    got = r.correlate(k, i0, i1, channels=channels, before=before, taps=taps, reference=reference)
    want = _want(dec, k, i0, i1, before, channels, taps, reference) if want is None else want[i0:i1]
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    return got


TAPS65 = api.highpass_taps(300, 5000, 65)
TAPS9 = np.random.RandomState(1).randn(9)


@pytest.mark.parametrize('n_cols', [1, 3, 4, 5, 15, 16, 17, 65])
def test_column_groups_and_bands(tmp_cfg, n_cols):
    x = synth_int16(0, 300, 70, 6)
    r, dec = _make(tmp_cfg, x, 100)                                     # three chunks of 100 rows
    rs = np.random.RandomState(n_cols)
    k = rs.randn(5, 7, n_cols)
    for cols in (list(range(n_cols)), [int(c) for c in rs.randint(0, 70, n_cols)]):      # in order; shuffled with repeats
        for reference in (None, 'median'):
            want = _want(dec, k, 0, 300, 3, cols, TAPS9, reference)
            _check(r, dec, k, 0, 300, 3, cols, TAPS9, reference, want)
            _check(r, dec, k, 5, 298, 3, cols, TAPS9, reference, want)   # starts off a tile, no multiple of 64 rows
    r.close()


def test_many_bands_at_production_width(tmp_cfg):
    x = synth_int16(0, 200, 385, 3)
    r, dec = _make(tmp_cfg, x, 100)
    k = np.random.RandomState(0).randn(3, 61, 385)
    _check(r, dec, k, 0, 200, 20, taps=TAPS9, reference='median')
    r.close()


@pytest.mark.parametrize('n_out', [1, 15, 16, 17, 63, 64, 65, 130])
def test_output_tiles_and_subsets(tmp_cfg, n_out):
    x = synth_int16(0, 200, 6, 5)
    r, dec = _make(tmp_cfg, x, 100)
    rs = np.random.RandomState(n_out)
    k = rs.randn(n_out, 5, 6)
    got = _check(r, dec, k, 0, 200, 2, taps=TAPS9, reference='median')
    # a template's scores do not depend on the other templates of the call, nor on the tile they land in
    sub = np.unique(rs.randint(0, n_out, max(1, n_out // 3)))
    assert r.correlate(k[sub], before=2, taps=TAPS9, reference='median').tobytes() == np.ascontiguousarray(got[:, sub]).tobytes()
    assert r.correlate(k[n_out - 1], 3, 77, before=2, taps=TAPS9, reference='median').tobytes() == got[3:77, n_out - 1].tobytes()
    r.close()


@pytest.mark.parametrize('T', [1, 2, 61, 256])
def test_template_length_and_offset(tmp_cfg, T):
    x = synth_int16(0, 700, 5, 2)
    r, dec = _make(tmp_cfg, x, 100)                                     # seven chunks: T = 256 reaches over three of them
    assert r.n_chunks == 7
    k = np.random.RandomState(T).randn(3, T, 5)
    for before in sorted({0, min(20, T), T}):
        for taps, reference in ((None, None), (TAPS65, 'median')):
            want = _want(dec, k, 0, 700, before, taps=taps, reference=reference)
            _check(r, dec, k, 0, 700, before, taps=taps, reference=reference, want=want)      # row 0 and the last row: zero rows both sides
            for i0, i1 in ((70, 201), (0, 1), (699, 700), (1, 66), (630, 700)):
                _check(r, dec, k, i0, i1, before, taps=taps, reference=reference, want=want)
    r.close()


def test_pipeline_combinations(tmp_cfg):
    x = synth_int16(0, 600, 17, 4)
    r, dec = _make(tmp_cfg, x, 200)
    k = np.random.RandomState(4).randn(4, 9, 17)
    for taps in (None, TAPS9, TAPS65):
        for reference in (None, 'median'):
            _check(r, dec, k, 0, 600, 4, taps=taps, reference=reference)
            _check(r, dec, k[:, :, :16], 33, 470, 4, channels=slice(0, 16), taps=taps, reference=reference)     # an even median
    r.close()


@pytest.mark.parametrize('dtype', ['int16', 'uint8', 'int64', 'float32', 'float64'])
def test_item_types(tmp_cfg, dtype):
    rows, nc = 400, 7
    rs = np.random.RandomState(3)
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 100).astype(dt)
    else:
        info = np.iinfo(dt)
        x = rs.randint(max(info.min, -2 ** 62), min(info.max, 2 ** 62), size=(rows, nc), dtype=np.int64).astype(dt)
    r, dec = _make(tmp_cfg, x, 100)
    k = rs.randn(3, 5, nc)
    for taps, reference in ((None, None), (TAPS9, 'median')):
        _check(r, dec, k, 0, rows, 2, taps=taps, reference=reference)
    r.close()


def test_special_values(tmp_cfg):
    rows, nc = 300, 9
    x = (np.random.RandomState(1).randn(rows, nc) * 10).astype(np.float32)
    x[51, 1] = np.nan
    x[110, 2] = np.inf
    x[130, 3] = -np.inf
    x[150:153] = 0.0
    x[151] = -0.0
    x[170, [0, 8]] = [np.inf, -np.inf]
    x[200:212, :] = np.nan
    r, dec = _make(tmp_cfg, x, 100)
    k = np.random.RandomState(2).randn(4, 5, nc)
    k[1] = 0.0                                                          # inf against a zero entry is NaN: nothing is skipped
    k[2, :, 2] = 0.0
    for taps in (None, [0.25, 0.5, 0.25]):
        for reference in (None, 'median'):
            for channels in (slice(None), slice(0, 8)):                  # odd and even medians
                kk = k[:, :, :8] if channels != slice(None) else k
                got = _check(r, dec, kk, 0, rows, 2, channels=channels, taps=taps, reference=reference)
                nan = np.isnan(got)
                assert nan.any() and set(got[nan].view(np.uint32).tolist()) == {NAN_BITS}
                if taps is None and not reference:
                    assert np.isnan(got[108:113, 1]).all() and np.isnan(got[108:113, 2]).all()      # inf * 0
                    assert np.isinf(got[108:113, 0]).all() and not np.isnan(got[140:160]).any()
                    assert (got[150:152, 1] == 0).all()
    r.close()


def test_subnormal_products(tmp_cfg):
    rs = np.random.RandomState(8)
    x = (rs.randn(330, 19) * 1e-20).astype(np.float32)
    r, dec = _make(tmp_cfg, x, 100)
    k = rs.randn(6, 7, 19) * 1e-20
    k[rs.randint(0, 6, 30), rs.randint(0, 7, 30), rs.randint(0, 19, 30)] = 0.0
    got = _check(r, dec, k, 0, 330, 3)
    assert (np.abs(got[got != 0]) < np.finfo(np.float32).tiny).all() and (got != 0).mean() > 0.5
    r.close()


def _upload(data):
    cbuf = hip.DevBuffer(len(data) + 256)
    host = np.frombuffer(data + b'\0' * 256, dtype=np.uint8).copy()
    hip._check(hip.lib().mts_dev_copy(0, None, cbuf.at(), hip._ptr(host), host.nbytes, 0), 'mts_dev_copy')
    return cbuf


def test_bit_identity_across_configurations(tmp_cfg, monkeypatch):
    x = synth_int16(0, 3000, 20, 4)
    one, dec = _make(tmp_cfg, x, 500, codec=api.HipCodec(devices=[0]))   # six chunks of 20 000 bytes
    two = _open(tmp_cfg, codec=api.HipCodec(devices=[0, 0]))
    k = np.random.RandomState(5).randn(10, 61, 20)
    kw = dict(before=20, taps=TAPS65, reference='median')
    want = _check(one, dec, k, 0, 3000, 20, taps=TAPS65, reference='median')                     # cold, one lane, one call, one slab
    assert one.correlate(k, **kw).tobytes() == want.tobytes()                                     # the same call twice
    assert two.correlate(k, **kw).tobytes() == want.tobytes()                                     # one lane == two
    for a, b, c in ((0, 1500, 3000), (0, 1, 3000), (0, 1777, 2999)):                             # the whole range == two halves
        assert np.concatenate([one.correlate(k, a, b, **kw), one.correlate(k, b, c, **kw)]).tobytes() == want[a:c].tobytes()
    monkeypatch.setattr(api, 'CORRELATE_CALL_BYTES', 1)                                           # a call per chunk
    assert one.correlate(k, **kw).tobytes() == want.tobytes()
    monkeypatch.setattr(api, 'CORRELATE_CALL_BYTES', 1 << 30)
    monkeypatch.setattr(api, 'CORRELATE_OUT_BYTES', 450 * 10 * 4)                                 # 450 rows per call
    assert two.correlate(k, **kw).tobytes() == want.tobytes()
    monkeypatch.setattr(api, 'CORRELATE_OUT_BYTES', 1 << 30)
    # slabs and pieces (both are read from the environment by every call): 760 rows of 80 bytes hold 700 owned rows -- five slabs
    # of the one piece; with pieces of one chunk, every piece its own slabs; a bound of one byte: a slab per row
    monkeypatch.setenv('MTS_CORRELATE_SLAB_BYTES', str(760 * 80))
    assert one.correlate(k, **kw).tobytes() == want.tobytes()
    monkeypatch.setenv('MTS_PIPE_BYTES', str(20000))
    assert one.correlate(k, **kw).tobytes() == want.tobytes()
    monkeypatch.setenv('MTS_CORRELATE_SLAB_BYTES', str(200 * 80))
    assert one.correlate(k, **kw).tobytes() == want.tobytes()
    monkeypatch.setenv('MTS_CORRELATE_SLAB_BYTES', '1')
    assert one.correlate(k, 1930, 2070, **kw).tobytes() == want[1930:2070].tobytes()
    monkeypatch.delenv('MTS_CORRELATE_SLAB_BYTES')
    monkeypatch.delenv('MTS_PIPE_BYTES')
    # resident == cold, and a scan inserts nothing
    keys = list(range(one.n_chunks))
    one[:]
    for c in range(one.n_chunks):
        one[one.chunk_bounds[c]:one.chunk_bounds[c] + 1]
    cache = one._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 20 for b in before) >= len(keys) // 2
    assert one.correlate(k, **kw).tobytes() == want.tobytes()
    assert hip.cache_query(cache, keys).tolist() == before
    # mts_correlate == mts_dev_correlate, on the file's chunks in host and in device memory
    data = (tmp_cfg / 'd.cbin').read_bytes()
    offs, bounds = np.asarray(one.chunk_offsets, np.int64), np.asarray(one.chunk_bounds, np.int64)
    args = (20, np.int16, one._flags(), 0, 3000, 40, 2950, TAPS65, np.arange(20), 1, 20, k)
    st, host = hip.correlate(0, keys, bounds[:-1], data, offs[:-1], np.diff(offs), np.diff(bounds), *args)
    assert st == [0] * one.n_chunks and host.tobytes() == want[40:2950].tobytes()
    cbuf = _upload(data)
    st, res, out = hip.dev_correlate(cbuf, offs[:-1], np.diff(offs), bounds[:-1], np.diff(bounds), *args)
    assert st == [0] * one.n_chunks and res.tobytes() == host.tobytes()
    out.free()
    cbuf.free()
    one.close()
    two.close()


def test_t1_is_project_and_one_hot_is_detects_amplitude(tmp_cfg):
    x = synth_int16(0, 1500, 24, 4)
    r, dec = _make(tmp_cfg, x, 500)
    k = np.random.RandomState(6).randn(9, 1, 24)
    got = r.correlate(k, 7, 1400, before=0)
    with np.errstate(over='ignore'):
        w = k[:, 0, :].astype(np.float32).T
    assert got.tobytes() == r.project(w, 7, 1400, dtype=np.float32).tobytes()
    # template j is 1 at (before, j): its score at an event of column j is z there -- detect's amplitude
    for reference in (None, 'median'):
        ev = r.detect(12.0, taps=TAPS65, sign='both', reference=reference, exclude=7, spread=3)
        assert ev.sample.size >= 50
        hot = np.zeros((24, 5, 24))
        hot[np.arange(24), 2, np.arange(24)] = 1.0
        score = r.correlate(hot, before=2, taps=TAPS65, reference=reference)
        assert np.array_equal(score[ev.sample, ev.channel], ev.amplitude)
    r.close()


def test_c_abi_argument_errors():
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = np.arange(400, dtype=np.int16).reshape(100, nc)
    z = hip.compress_chunks(x, [0, 100], hip.make_flags(), 6)[0]
    data = np.frombuffer(z + b'\0' * 16, dtype=np.uint8)
    cbuf = _upload(z)
    d_out = hip.DevBuffer(1 << 16)
    keep = []

    def call(dev=False, row0=0, rows=100, taps=(1.0, 0.5), vb=0, ve=100, rb=10, re=90, cols=(0, 1), ref=0, before=1, T=3, K=2, tpl=None,
             itemsize=2, flags=hip.make_flags(), outs=True, templates=True):
        a = [np.array(v, dtype=np.int64) for v in ([0], [row0], [0], [len(z)], [rows])]
        c, t = np.array(cols, dtype=np.int32), np.array(taps, dtype=np.float64)
        k = np.ones((max(K, 1), max(T, 1), max(len(c), 1)), np.float32) if tpl is None else np.asarray(tpl, np.float32)
        o = np.full(4096, 5, np.float32)
        st = np.full(1, 99, np.int32)
        keep.append((a, c, t, k, o, st))
        lp = [v.ctypes.data_as(C.POINTER(C.c_long)) for v in a]
        mid = (vb, ve, rb, re, len(t), t.ctypes.data_as(C.POINTER(C.c_double)), len(c), c.ctypes.data_as(C.POINTER(C.c_int)), ref, before, T, K,
               k.ctypes.data_as(C.POINTER(C.c_float)) if templates else None)
        stp = st.ctypes.data_as(C.POINTER(C.c_int))
        if dev:
            rc = L.mts_dev_correlate(0, None, cbuf.at(), lp[2], lp[3], lp[1], lp[4], 1, nc, itemsize, flags, *mid, d_out.at(0) if outs else None, stp)
        else:
            rc = L.mts_correlate(0, 0, 1, lp[0], lp[1], data.ctypes.data_as(C.c_void_p), lp[2], lp[3], lp[4], nc, itemsize, flags, *mid,
                                 hip._ptr(o) if outs else None, stp)
        return rc, int(st[0]), o
    for dev in (False, True):
        rc, st, o = call(dev=dev)
        assert (rc, st) == (0, 0)
        if not dev:
            want = correlate(x[:, :2], 0, 0, 100, 10, 90, [1.0, 0.5], 0, 1, np.ones((2, 3, 2)))
            assert o[:160].tobytes() == want.tobytes() and o[160] == 5
        rc, st, o = call(dev=dev, rb=40, re=40, outs=False)              # no rows: MTS_OK, nothing written
        assert (rc, st) == (0, 0)
        assert call(dev=dev, before=0, T=1)[:2] == (0, 0) and call(dev=dev, before=256, T=256)[:2] == (0, 0)
        others = (dict(outs=False), dict(taps=(np.inf, 1.0)), dict(cols=(0, 4)), dict(cols=(-1,)), dict(row0=10),
                  dict(rows=50), dict(rb=-1), dict(re=101), dict(rb=50, re=40), dict(itemsize=3), dict(flags=hip.FLAG_FLOAT, itemsize=2))
        # (a shared argument, one bad at a time: the text is the one the library gave before the five ops shared their checks)
        for bad, text in [(b, None) for b in others] + filter_errors('correlate') + template_errors('correlate'):
            rc, st, o = call(dev=dev, **bad)
            assert rc == -1, bad                                       # MTS_E_ARG ...
            assert st == 99 and (o == 5).all(), bad                    # ... before anything ran
            said = hip.lib().mts_last_error().decode()
            assert said and text in (None, said), (bad, said)
    d_out.free()
    cbuf.free()


def test_damaged_chunk_sets_its_status_and_raises(tmp_cfg):
    x = synth_int16(0, 2500, 8, 4)
    r, _ = _make(tmp_cfg, x, 500)
    b, o = r.chunk_bounds, r.chunk_offsets
    flags = r._flags()
    r.close()
    data = bytearray((tmp_cfg / 'd.cbin').read_bytes())
    data[o[2] + 30:o[2] + 60] = b'\x00' * 30
    (tmp_cfg / 'd.cbin').write_bytes(bytes(data))
    k = np.random.RandomState(7).randn(2, 61, 8)
    offs, bounds = np.asarray(o, np.int64), np.asarray(b, np.int64)
    st, _ = hip.correlate(0, list(range(5)), bounds[:-1], bytes(data), offs[:-1], np.diff(offs), np.diff(bounds), 8, np.int16, flags, 0, 2500, 0,
                          2500, TAPS65, np.arange(8), 1, 20, k)
    assert st[2] != hip.CHUNK_OK and [s for i, s in enumerate(st) if i != 2] == [hip.CHUNK_OK] * 4
    r = _open(tmp_cfg)
    kw = dict(before=20, taps=TAPS65, reference='median')
    with pytest.raises(IOError, match='#2'):
        r.correlate(k, 0, b[2] - 71, **kw)                              # rows of chunks 0 and 1 only; row + 40 + 32 reaches chunk 2
    with pytest.raises(IOError, match='#2'):
        r.correlate(k, b[3] + 51, b[4], **kw)                           # ... and from above: row - 20 + 32 - 64
    r.correlate(k, 0, b[2] - 72, **kw)
    r.correlate(k, b[3] + 52, b[4], **kw)
    r.close()
