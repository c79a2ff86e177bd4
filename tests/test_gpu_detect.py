"""Reader.detect and mts_detect / mts_dev_detect on the MI355X: the kernels against the numpy restatement of the definition
(tests/detect_oracle.py) over the oracle's decode, for exact equality of the events: every item type, column tiling, row edges, ties
and plateaus, special values, bit-identity across calls, lanes, pieces, slabs, the cache and the two entry points, capacity, argument
errors and a damaged chunk in the halo."""
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
from tests.detect_oracle import SIGNS, detect_events, filtered, tied_events
from tests.zfamily_errors import filter_errors, wide_errors

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


def _check(r, dec, threshold, start=0, stop=None, channels=slice(None), taps=None, sign='neg', reference=None, exclude=0, spread=0):
    got = r.detect(threshold, start, stop, channels=channels, taps=taps, sign=sign, reference=reference, exclude=exclude, spread=spread)
    n = dec.shape[0]
    i0 = r._validate_index(start, 0)
    i1 = max(i0, r._validate_index(stop, n))
    cols = np.arange(dec.shape[1])[channels] if isinstance(channels, slice) else np.asarray(channels) % dec.shape[1]
    want = detect_events(dec[:, cols], 0, 0, n, i0, i1, [1.0] if taps is None else taps, threshold, SIGNS[sign], 1 if reference else 0,
                         exclude, spread)
    assert got.sample.dtype == got.channel.dtype == np.int64 and got.amplitude.dtype == np.float32
    assert got.sample.tobytes() == want[0].tobytes(), (got.sample[:8], want[0][:8], got.sample.size, want[0].size)
    assert got.channel.tobytes() == cols.astype(np.int64)[want[1]].tobytes()
    assert got.amplitude.tobytes() == want[2].tobytes()
    return got


def _same(a, b):
    for key in ('sample', 'channel', 'amplitude'):
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize('dtype', ['int8', 'int64', 'uint32', 'uint64', 'uint8', 'uint16', 'int16', 'int32', 'float32', 'float64'])
def test_every_item_type(tmp_cfg, dtype):
    rows, nc = 3000, 70
    rs = np.random.RandomState(3)
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 100).astype(dt)
    else:
        info = np.iinfo(dt)
        x = rs.randint(max(info.min, -2 ** 62), min(info.max, 2 ** 62), size=(rows, nc), dtype=np.int64).astype(dt)
    r, dec = _make(tmp_cfg, x, 700)
    for taps in (np.random.RandomState(1).randn(9), [1.0]):
        y = filtered(dec, 0, 0, rows, 0, rows, np.asarray(taps, np.float64)).astype(np.float64)
        for reference in (None, 'median'):
            z = y - np.median(y, axis=1)[:, None] if reference else y
            thr = 1.5 * float(z.std())                                  # the oracle's own filtered rows set the scale of the type
            for R in (0, 1, 7):
                for S in (0, 3):
                    for sign in ('neg', 'pos', 'both'):
                        got = _check(r, dec, thr, 13, 2950, taps=taps, sign=sign, reference=reference, exclude=R, spread=S)
                        if sign == 'both':
                            assert got.sample.size >= 50
    r.close()


@pytest.mark.parametrize('n_cols', [1, 2, 63, 64, 65, 129])
def test_column_tiling(tmp_cfg, n_cols):
    x = synth_int16(0, 1200, 131, 6)
    r, dec = _make(tmp_cfg, x, 500)
    taps = api.highpass_taps(300, 5000, 17)
    rs = np.random.RandomState(n_cols)
    n_ev = 0
    for cols in (list(range(n_cols)), [int(c) for c in rs.randint(0, 131, n_cols)]):      # in order; shuffled with repeats
        for reference in (None, 'median'):
            for S in (0, 3):                                                               # 3 crosses the 64-position words
                n_ev += _check(r, dec, 8.0, 5, 1190, channels=cols, taps=taps, sign='both', reference=reference, exclude=2, spread=S).sample.size
    assert n_ev >= 50
    r.close()


def test_row_edges(tmp_cfg):
    n, nc = 1000, 5
    x = (synth_int16(0, n, nc, 2) // 4).astype(np.int16)
    start, stop = 230, 770
    for t in (0, n - 1, start, stop - 1):
        x[t, 1] = 3000
    for b in range(100, n, 100):
        x[b - 1, 2], x[b, 3], x[b + 1, 4] = 3000, 3000, 3000
    x[start, 0], x[start - 1, 0] = 2000, 2500                        # a larger peak just outside suppresses the one inside
    x[stop - 1, 4], x[stop, 4] = -2000, -2500
    r, dec = _make(tmp_cfg, x, 100)
    assert r.n_chunks == 10
    rs = np.random.RandomState(0)
    n_ev = 0
    for L in (1, 2, 65, 257):                                         # 257: more than two chunks of halo
        taps = [1.0] if L == 1 else (rs.randn(L) / np.sqrt(L))
        for R in (0, 99, 100, 255):
            for a, b in ((0, None), (start, stop)):
                got = _check(r, dec, 900.0, a, b, taps=taps, sign='both', exclude=R, spread=0)
                assert got.sample.size >= 1
                n_ev += got.sample.size
    assert n_ev >= 100
    plain = _check(r, dec, 900.0, start, stop, sign='both', exclude=1, spread=0)
    pairs = set(zip(plain.sample.tolist(), plain.channel.tolist()))
    assert (start, 1) in pairs and (stop - 1, 1) in pairs and (start, 0) not in pairs and (stop - 1, 4) not in pairs
    assert {(299, 2), (300, 3), (301, 4)} <= pairs
    whole = _check(r, dec, 900.0, sign='both', exclude=1, spread=0)
    pairs = set(zip(whole.sample.tolist(), whole.channel.tolist()))
    assert {(0, 1), (n - 1, 1), (start - 1, 0), (stop, 4)} <= pairs
    r.close()


def test_ties_and_plateaus(tmp_cfg):
    x = (synth_int16(0, 2000, 70, 9) // 8).astype(np.int16)
    r, dec = _make(tmp_cfg, x, 700)
    for S, n_ev, n_tied in [(0, 3208, 1772), (2, 2024, 1268)]:
        got = _check(r, dec, 2.5, sign='both', exclude=3, spread=S)
        tied = tied_events(dec, 0, 0, 2000, 0, 2000, [1.0], 2, 0, 3, S, got.sample, got.channel)
        assert (got.sample.size, tied) == (n_ev, n_tied) and tied >= 1000
    r.close()


def test_worst_inputs_for_the_early_exit(tmp_cfg):
    flat = np.full((4000, 130), 7, np.int16)
    r, dec = _make(tmp_cfg, flat, 1000)
    got = _check(r, dec, 1.0, sign='pos', exclude=255, spread=32)    # one chain: (first row, position 0)
    assert (got.sample.tolist(), got.channel.tolist()) == ([0], [0])
    got = _check(r, dec, 1.0, 1000, 3000, sign='pos', exclude=255, spread=32)
    assert got.sample.size == 0                                       # the rows before the range win
    got = _check(r, dec, 1.0, sign='both', exclude=255, spread=0)    # every column is a chain of its own
    assert (got.sample.tolist(), got.channel.tolist()) == ([0] * 130, list(range(130)))
    r.close()
    ramp = (np.arange(4000, dtype=np.int16)[:, None] + 1) * np.ones((1, 130), np.int16)
    r, dec = _make(tmp_cfg, ramp, 1000)
    got = _check(r, dec, 1.0, sign='pos', exclude=255, spread=32)    # strictly rising: the last row
    assert (got.sample.tolist(), got.channel.tolist()) == ([3999], [0])
    r.close()


def test_special_float_values(tmp_cfg):
    rows, nc = 2000, 9
    x = (np.random.RandomState(1).randn(rows, nc) * 10).astype(np.float32)
    x[510, 1] = np.nan
    x[1100, 2] = np.inf
    x[1300, 3] = -np.inf
    x[1500:1503] = 0.0
    x[1501, 4] = -0.0
    x[1700, [0, 8]] = [np.inf, -np.inf]
    r, dec = _make(tmp_cfg, x, 500)
    taps = [0.25, 0.5, 0.25]
    for reference in (None, 'median'):
        for channels in (slice(None), slice(0, 8)):                    # odd and even medians
            for sign in ('neg', 'pos', 'both'):
                got = _check(r, dec, 6.0, channels=channels, taps=taps, sign=sign, reference=reference, exclude=3, spread=2)
                assert got.sample.size >= 20
                near = np.isin(got.sample, [509, 510, 511])                   # the rows whose filter support holds the NaN
                assert not (near & (got.channel == 1)).any()
                if reference:
                    assert not near.any()
    r.close()


def test_bit_identity_calls_lanes_cache_and_repeats(tmp_cfg, monkeypatch):
    x = synth_int16(0, 40000, 40, 4)
    one, dec = _make(tmp_cfg, x, 5000, codec=api.HipCodec(devices=[0]))
    two = _open(tmp_cfg, codec=api.HipCodec(devices=[0, 0]))
    kw = dict(taps=api.highpass_taps(300, 5000, 65), sign='both', reference='median', exclude=30, spread=5)
    want = _check(one, dec, 14.0, 100, 39000, **kw)
    assert want.sample.size >= 200
    _same(one.detect(14.0, 100, 39000, **kw), want)                                                # the same call twice
    _same(two.detect(14.0, 100, 39000, **kw), want)                                                # one device == two lanes
    parts = [one.detect(14.0, a, b, **kw) for a, b in [(100, 15000), (15000, 15003), (15003, 39000)]]
    for key in ('sample', 'channel', 'amplitude'):
        assert np.concatenate([p[key] for p in parts]).tobytes() == want[key].tobytes()            # one call == many
    monkeypatch.setattr(api, 'DETECT_CALL_BYTES', 1)
    _same(one.detect(14.0, 100, 39000, **kw), want)
    monkeypatch.setattr(api, 'DETECT_CALL_BYTES', 1 << 30)
    monkeypatch.setattr(api, 'DETECT_GUESS_MIN', 3)                                                # a short buffer: the call is made twice
    monkeypatch.setattr(api, 'DETECT_GUESS_SAMPLES', 1 << 40)
    _same(one.detect(14.0, 100, 39000, **kw), want)
    monkeypatch.setattr(api, 'DETECT_GUESS_MIN', 4096)
    monkeypatch.setattr(api, 'DETECT_GUESS_SAMPLES', 256)
    keys = list(range(one.n_chunks))
    one[:]                                                                                         # (read-ahead makes chunks resident)
    for k in range(one.n_chunks):
        one[one.chunk_bounds[k]:one.chunk_bounds[k] + 1]
    cache = one._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 40 for b in before) >= len(keys) // 2
    _same(one.detect(14.0, 100, 39000, **kw), want)                                                # resident == cold
    assert hip.cache_query(cache, keys).tolist() == before                                         # the scan changed nothing
    one.close()
    two.close()


def test_pipe_and_slab_bytes_do_not_change_the_result(tmp_cfg):
    x = synth_int16(0, 40000, 40, 4)
    r, _ = _make(tmp_cfg, x, 5000)
    r.close()
    script = ("import sys, numpy as np, mtscomp_amd; sys.path.insert(0, %r); from mtscomp_amd import api; "
              "r = mtscomp_amd.decompress(%r, %r, check_after_decompress=False); "
              "e = r.detect(14.0, 33, None, taps=api.highpass_taps(300, 5000, 65), sign='both', reference='median', exclude=30, spread=5); "
              "np.savez(sys.argv[1], s=e.sample, c=e.channel, a=e.amplitude)") % (os.getcwd(), str(tmp_cfg / 'd.cbin'), str(tmp_cfg / 'd.ch'))
    outs = []
    for pipe, slab in ((None, None), (str(200 * 1024), str(100 * 1024))):
        env = dict(os.environ)
        env.pop('MTS_PIPE_BYTES', None)
        env.pop('MTS_DETECT_SLAB_BYTES', None)
        if pipe:
            env['MTS_PIPE_BYTES'], env['MTS_DETECT_SLAB_BYTES'] = pipe, slab
        p = tmp_cfg / ('o%d.npz' % len(outs))
        subprocess.run([sys.executable, '-c', script, str(p)], env=env, check=True, timeout=300)
        outs.append(np.load(p))
    assert outs[0]['s'].size >= 200
    for key in 'sca':
        assert outs[0][key].tobytes() == outs[1][key].tobytes()


def _abi_recording(nc=4, rows=300, chunk=100):
    rs = np.random.RandomState(2)
    x = rs.randint(-50, 50, size=(rows, nc)).astype(np.int16)
    bounds = list(range(0, rows + 1, chunk))
    zs = hip.compress_chunks(x, bounds, hip.make_flags(), 6)
    offs = np.concatenate(([0], np.cumsum([len(z) for z in zs])))
    return x, np.array(bounds, np.int64), zs, offs


def test_capacity_and_device_entry():
    hip.require_device()
    nc = 4
    x, bounds, zs, offs = _abi_recording(nc)
    data = b''.join(zs)
    n = x.shape[0]
    flags = hip.make_flags()
    rows = np.diff(bounds)
    keys = np.arange(3)
    args = (nc, np.int16, flags, 0, n, 10, 290, [0.5, 0.25, -0.5], np.arange(nc), 8.0, 2, 1, 2, 1)
    want = detect_events(x, 0, 0, n, 10, 290, [0.5, 0.25, -0.5], 8.0, 2, 1, 2, 1)
    total = want[0].size
    assert total >= 50
    st, n_ev, row, pos, amp = hip.detect(0, keys, bounds[:-1], data, offs[:-1], np.diff(offs), rows, *args, total + 10)
    assert st == [0, 0, 0] and n_ev == total
    assert (row.tobytes(), pos.astype(np.int64).tobytes(), amp.tobytes()) == tuple(w.tobytes() for w in want)
    for cap in (total, total - 1, 7, 1):                            # a short buffer: the full count and the exact prefix
        st, n_ev, r2, p2, a2 = hip.detect(0, keys, bounds[:-1], data, offs[:-1], np.diff(offs), rows, *args, cap)
        assert n_ev == total and r2.size == cap
        assert (r2.tobytes(), p2.tobytes(), a2.tobytes()) == (row[:cap].tobytes(), pos[:cap].tobytes(), amp[:cap].tobytes())
    st, n_ev, r2, p2, a2 = hip.detect(0, keys, bounds[:-1], data, offs[:-1], np.diff(offs), rows, *args, 0)
    assert n_ev == total and r2.size == 0
    # the device entry on the same bytes
    cbuf = hip.DevBuffer(len(data) + 256)
    host = np.frombuffer(data + b'\0' * 256, dtype=np.uint8).copy()
    hip._check(hip.lib().mts_dev_copy(0, None, cbuf.at(), hip._ptr(host), host.nbytes, 0), 'mts_dev_copy')
    st, n_ev, res, out = hip.dev_detect(cbuf, offs[:-1], np.diff(offs), bounds[:-1], rows, *args, total + 10)
    assert st == [0, 0, 0] and n_ev == total
    assert (res[0].tobytes(), res[1].tobytes(), res[2].tobytes()) == (row.tobytes(), pos.tobytes(), amp.tobytes())
    st, n_ev, res, out = hip.dev_detect(cbuf, offs[:-1], np.diff(offs), bounds[:-1], rows, *args, 5, out=out)
    assert n_ev == total and res[0].tobytes() == row[:5].tobytes() and res[2].tobytes() == amp[:5].tobytes()
    out.free()
    cbuf.free()


def test_c_abi_argument_errors():
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = np.arange(400, dtype=np.int16).reshape(100, nc)
    z = hip.compress_chunks(x, [0, 100], hip.make_flags(), 6)[0]
    data = np.frombuffer(z + b'\0' * 16, dtype=np.uint8)
    cbuf = hip.DevBuffer(len(z) + 256)
    host = np.frombuffer(z + b'\0' * 256, dtype=np.uint8).copy()
    hip._check(L.mts_dev_copy(0, None, cbuf.at(), hip._ptr(host), host.nbytes, 0), 'mts_dev_copy')
    d_out = hip.DevBuffer(1 << 16)
    keep = []

    def call(dev=False, row0=0, rows=100, taps=(1.0, 0.5), vb=0, ve=100, rb=10, re=90, cols=(0, 1), thr=(1.0, 1.0), sign=0, ref=0, R=1, S=1,
             cap=64, itemsize=2, flags=hip.make_flags(), outs=True, n_ev=True):
        a = [np.array(v, dtype=np.int64) for v in ([0], [row0], [0], [len(z)], [rows])]
        c, t, th = np.array(cols, dtype=np.int32), np.array(taps, dtype=np.float64), np.array(thr, dtype=np.float32)
        o = (np.zeros(256, np.int64), np.zeros(256, np.int32), np.zeros(256, np.float32))
        st, ne = np.full(1, 99, np.int32), np.full(1, -7, np.int64)
        keep.append((a, c, t, th, o, st, ne))
        lp = [v.ctypes.data_as(C.POINTER(C.c_long)) for v in a]
        tail = (vb, ve, rb, re, len(t), t.ctypes.data_as(C.POINTER(C.c_double)), len(c), c.ctypes.data_as(C.POINTER(C.c_int)),
                th.ctypes.data_as(C.POINTER(C.c_float)), sign, ref, R, S, cap)
        nep = ne.ctypes.data_as(C.POINTER(C.c_long)) if n_ev else None
        stp = st.ctypes.data_as(C.POINTER(C.c_int))
        if dev:
            po = (d_out.at(0), d_out.at(8192), d_out.at(16384)) if outs else (None, None, None)
            rc = L.mts_dev_detect(0, None, cbuf.at(), lp[2], lp[3], lp[1], lp[4], 1, nc, itemsize, flags, *tail, *po, nep, stp)
        else:
            po = tuple(hip._ptr(v) for v in o) if outs else (None, None, None)
            rc = L.mts_detect(0, 0, 1, lp[0], lp[1], data.ctypes.data_as(C.c_void_p), lp[2], lp[3], lp[4], nc, itemsize, flags, *tail, *po, nep, stp)
        return rc, int(st[0]), int(ne[0])
    for dev in (False, True):
        rc, st, ne = call(dev=dev)
        assert (rc, st) == (0, 0) and ne >= 0
        assert call(dev=dev, cap=0, outs=False)[:2] == (0, 0)
        for bad in (dict(taps=()), dict(taps=(np.nan,)), dict(taps=(np.inf, 1.0)), dict(taps=np.ones(8193)), dict(cols=(0, 4), thr=(1, 1)),
                    dict(cols=(-1,), thr=(1,)), dict(cols=(), thr=()), dict(thr=(1.0, 0.0)), dict(thr=(-1.0, 1.0)), dict(thr=(np.nan, 1.0)),
                    dict(thr=(np.inf, 1.0)), dict(sign=3), dict(sign=-1), dict(ref=2), dict(ref=-1), dict(R=-1), dict(R=256), dict(S=-1),
                    dict(S=33), dict(cap=-1), dict(outs=False), dict(n_ev=False), dict(row0=10), dict(rows=50), dict(rb=-1), dict(re=101),
                    dict(rb=50, re=40), dict(vb=50, ve=20), dict(vb=20), dict(ve=80), dict(itemsize=3), dict(flags=hip.FLAG_FLOAT, itemsize=2),
                    dict(ref=1, cols=[0] * 1025, thr=[1.0] * 1025)):
            rc, st, ne = call(dev=dev, **bad)
            assert rc == -1, bad                                       # MTS_E_ARG ...
            assert st == 99 and ne == -7, bad                          # ... before anything ran
        # a shared argument, one bad at a time: the text is the one the library gave before the five ops shared their checks
        for bad, text in filter_errors('detect') + wide_errors('detect'):
            if 'cols' in bad:
                bad = dict(bad, thr=[1.0] * len(bad['cols']))          # (a threshold per column)
            rc, st, ne = call(dev=dev, **bad)
            assert (rc, st, ne) == (-1, 99, -7), bad
            assert hip.lib().mts_last_error().decode() == text, bad
    d_out.free()
    cbuf.free()


def test_damaged_chunk_in_the_halo(tmp_cfg):
    x = synth_int16(0, 15000, 16, 4)
    r, _ = _make(tmp_cfg, x, 3000)
    b, o = r.chunk_bounds, r.chunk_offsets
    r.close()
    data = bytearray((tmp_cfg / 'd.cbin').read_bytes())
    data[o[2] + 30:o[2] + 60] = b'\x00' * 30
    (tmp_cfg / 'd.cbin').write_bytes(bytes(data))
    r = _open(tmp_cfg)
    taps = api.highpass_taps(300, 5000, 65)
    with pytest.raises(IOError, match='#2'):
        r.detect(12.0, 0, b[2] - 50, taps=taps, exclude=30)       # rows of chunks 0 and 1 only; row + 30 + 32 reaches chunk 2
    with pytest.raises(IOError, match='#2'):
        r.detect(12.0, b[3] + 10, b[4], taps=taps, exclude=30)    # ... and from above: row - 30 + 32 - 64
    r.detect(12.0, 0, b[2] - 62, taps=taps, exclude=30)
    r.detect(12.0, b[3] + 62, b[4], taps=taps, exclude=30)
    r.close()
