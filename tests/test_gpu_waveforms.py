"""Reader.waveforms and mts_waveforms / mts_dev_waveforms on the MI355X: the kernel against the numpy restatement of the definition
(tests/waveforms_oracle.py) over the oracle's decode, for exact equality of every byte: the base case with its edge counts, every
item type, column tiling, row edges, extrema on flat, ramp and special values, bit-identity across the cache, lanes, calls, pieces,
slabs, gaps and the two entry points, a sparse list with damaged chunks, argument errors."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.detect_oracle import detect_events
from tests.waveforms_oracle import BASE_COUNTS, FILL, edge_counts, waveforms
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


def _check(r, dec, sample, channel=None, before=20, after=41, neighbours=None, channels=slice(None), taps=None, reference=None):
    """Reader.waveforms, with and without the snippets, against the definition.  -> the Bunch."""
    got = r.waveforms(sample, channel, before=before, after=after, neighbours=neighbours, channels=channels, taps=taps, reference=reference)
    cols = np.arange(dec.shape[1])[channels] if isinstance(channels, slice) else np.asarray(channels) % dec.shape[1]
    sample = np.asarray(sample, dtype=np.int64)
    if neighbours is None:
        col0, W = np.zeros(sample.size, np.int64), cols.size
    else:
        col0, W = np.array([cols.tolist().index(c) for c in np.asarray(channel)], np.int64) - neighbours, 2 * neighbours + 1
    wave, vmin, amin, vmax, amax = waveforms(dec[:, cols], 0, 0, dec.shape[0], [1.0] if taps is None else taps, 1 if reference else 0, sample,
                                             col0, before, after, W)
    assert got.waveforms.dtype == np.float32 and got.waveforms.shape == wave.shape
    assert got.waveforms.tobytes() == wave.tobytes(), np.argwhere(got.waveforms.view(np.uint32) != wave.view(np.uint32))[:4]
    assert np.array_equal(got.position, col0) and np.array_equal(got.sample, sample)
    bare = r.waveforms(sample, channel, before=before, after=after, neighbours=neighbours, channels=channels, taps=taps, reference=reference,
                       waveforms=False)
    assert bare.waveforms is None
    for b in (got, bare):
        for name, v, i in (('trough', vmin, amin), ('peak', vmax, amax)):
            e = b[name]
            assert e.value.dtype == np.float32 and e.index.dtype == e.offset.dtype == e.channel.dtype == np.int64
            assert e.value.tobytes() == v.tobytes(), name
            assert e.index.tobytes() == i.tobytes(), name
            some = i >= 0
            assert np.array_equal(e.offset, np.where(some, i // W - before, 0))
            assert np.array_equal(e.channel, np.where(some, cols[np.where(some, col0 + i % W, 0)], -1))
    return got


def _same(a, b):
    assert a.waveforms.tobytes() == b.waveforms.tobytes()
    for name in ('trough', 'peak'):
        for key in ('value', 'index', 'offset', 'channel'):
            assert a[name][key].tobytes() == b[name][key].tobytes(), (name, key)


TAPS65 = api.highpass_taps(300, 5000, 65)


@pytest.mark.parametrize('reference', [None, 'median'])
def test_base_case(tmp_cfg, reference):
    x = synth_int16(0, 3000, 70, 4)
    r, dec = _make(tmp_cfg, x, 700)
    row, pos, amp = detect_events(dec, 0, 0, 3000, 0, 3000, TAPS65, 12, 0, 1 if reference else 0, 7, 3)
    assert edge_counts(row, pos - 8, 20, 41, 17, 3000, 70) == BASE_COUNTS[1 if reference else 0]      # no edge is reached vacuously
    got = _check(r, dec, row, pos, neighbours=8, taps=TAPS65, reference=reference)
    ev = r.detect(12, taps=TAPS65, sign='neg', reference=reference, exclude=7, spread=3)
    assert ev.sample.tobytes() == row.tobytes()
    assert got.waveforms[np.arange(row.size), 20, ev.channel - got.position].tobytes() == ev.amplitude.tobytes()
    r.close()


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
    sample = np.concatenate(([0, rows - 1, 1, 999, 1000], rs.randint(0, rows, 55)))
    channel = rs.randint(0, nc, sample.size)
    assert sample.size >= 50
    for taps in (np.random.RandomState(1).randn(9), [1.0]):
        for reference in (None, 'median'):
            for before, after in ((5, 9), (0, 1), (1, 0)):
                for k in (None, 0, 2):
                    _check(r, dec, sample, channel, before, after, k, taps=taps, reference=reference)
    r.close()


@pytest.mark.parametrize('n_cols', [1, 2, 63, 64, 65, 129])
def test_column_tiling(tmp_cfg, n_cols):
    x = synth_int16(0, 1200, 131, 6)
    r, dec = _make(tmp_cfg, x, 500)
    taps = api.highpass_taps(300, 5000, 17)
    rs = np.random.RandomState(n_cols)
    sample = np.concatenate(([0, 1199, 499, 500], rs.randint(0, 1200, 60)))
    for cols in (list(range(n_cols)), [int(c) for c in rs.randint(0, 131, n_cols)]):      # in order; shuffled with repeats
        channel = np.asarray(cols)[rs.randint(0, n_cols, sample.size)]
        channel[:2] = cols[0], cols[-1]
        for reference in (None, 'median'):
            for k in (0, 1, 32, None):
                _check(r, dec, sample, channel, 6, 7, k, channels=cols, taps=taps, reference=reference)
    r.close()


def test_row_edges(tmp_cfg):
    n, nc = 1000, 5
    x = (synth_int16(0, n, nc, 2) // 4).astype(np.int16)
    r, dec = _make(tmp_cfg, x, 100)
    assert r.n_chunks == 10
    sample = np.array([0, n - 1, 450, 499, 500, 501, 299, 300, 0, n - 1, 1, n - 2])       # the ends, mid-chunk, both sides of chunk boundaries
    channel = np.arange(sample.size) % nc
    rs = np.random.RandomState(0)
    for L in (1, 65, 257):                                              # 257: more than two chunks of filter support
        taps = [1.0] if L == 1 else (rs.randn(L) / np.sqrt(L))
        for before, after in ((0, 1), (1, 0), (20, 41), (2048, 2048), (4096, 0), (0, 4096)):   # T = 1, 61 and 4096: past both ends from anywhere
            for reference in (None, 'median'):
                got = _check(r, dec, sample, channel, before, after, None if before + after == 61 else 1, taps=taps, reference=reference)
                if before + after == 4096:
                    assert np.isnan(got.waveforms).sum() >= sample.size * 3 * (4096 - n)
    r.close()


def test_extrema_flat_and_ramp(tmp_cfg):
    n, nc = 2000, 9
    flat = np.full((n, nc), 7, np.int16)
    r, dec = _make(tmp_cfg, flat, 1000)
    sample = np.array([0, 3, 19, 20, 1000, n - 1, 5, 700])
    channel = np.array([0, 1, 8, 4, 4, 8, 0, 7])
    got = _check(r, dec, sample, channel, 20, 41, 2)
    # all equal: the first entry that is not fill -- index 0, or the first row and position inside for clipped events
    first = np.maximum(0, 20 - sample) * 5 + np.maximum(0, 2 - channel)
    assert np.array_equal(got.trough.index, first) and np.array_equal(got.peak.index, first) and first[4] == 0 and first[0] == 20 * 5 + 2
    assert (got.trough.value == 7).all() and (got.peak.value == 7).all()
    r.close()
    ramp = (np.arange(n, dtype=np.int32)[:, None] * nc + np.arange(nc, dtype=np.int32)[None, :])
    r, dec = _make(tmp_cfg, ramp, 1000)
    got = _check(r, dec, sample, channel, 20, 41, 2)
    assert np.array_equal(got.trough.index, first)                     # strictly rising in (tau, w): the first and the last entry inside
    last = (np.minimum(61, n - sample + 20) - 1) * 5 + np.minimum(4, nc - 1 - channel + 2)
    assert np.array_equal(got.peak.index, last) and last[4] == 61 * 5 - 1
    _check(r, dec, sample, before=3, after=4, reference='median')      # (the median of a ramp's row: its middle column)
    r.close()


def test_extrema_special_float_values(tmp_cfg):
    rows, nc = 2000, 9
    x = (np.random.RandomState(1).randn(rows, nc) * 10).astype(np.float32)
    x[510, 1] = np.nan
    x[1100, 2] = np.inf
    x[1300, 3] = -np.inf
    x[1500:1503] = 0.0
    x[1501, 4] = -0.0
    x[1700, [0, 8]] = [np.inf, -np.inf]
    x[800:812, :] = np.nan                                               # whole snippets of NaN
    x[900:905, 2:5] = np.nan
    r, dec = _make(tmp_cfg, x, 500)
    sample = np.array([510, 505, 515, 1100, 1098, 1300, 1303, 1500, 1501, 1502, 1499, 1700, 805, 806, 902, 100, 0, rows - 1])
    channel = np.array([1, 1, 0, 2, 3, 3, 4, 4, 4, 3, 5, 0, 4, 0, 3, 7, 0, 8])
    for taps in (None, [0.25, 0.5, 0.25]):
        for reference in (None, 'median'):
            for channels in (slice(None), slice(0, 8)):                  # odd and even medians
                ch = np.minimum(channel, 7) if channels != slice(None) else channel
                got = _check(r, dec, sample, ch, 2, 3, 1, channels=channels, taps=taps, reference=reference)
                for e in (12, 13):                                       # rows 803 .. 808: nothing but NaN
                    assert got.trough.index[e] == got.peak.index[e] == -1
                    assert got.trough.value[e].tobytes() == got.peak.value[e].tobytes() == FILL.tobytes()
                    assert got.trough.channel[e] == -1 and got.peak.offset[e] == 0
                if taps is None and not reference:
                    assert got.peak.value[3] == np.inf and got.trough.value[5] == -np.inf
                    assert got.trough.index[14] == -1                    # rows 900 .. 904, positions 2 .. 4
                    z = got.waveforms[8]                                 # rows 1499 .. 1503, positions 3 .. 5: the planted zeros of both
                    assert (z[1:4] == 0).all() and not np.signbit(z[1:4]).any()   # signs (the filter's sum starts at +0: -0 comes out as +0)
                    assert got.trough.index[8] == 0 or got.trough.value[8] < 0
                _check(r, dec, sample, before=2, after=3, channels=channels, taps=taps, reference=reference)
    r.close()


_EVENTS = {}


def _events_with_gaps(dec):
    """>= 300 events of the 40000 x 40 recording, thinned so that three stretches of rows hold none (computed once)."""
    if 'all' not in _EVENTS:
        _EVENTS['all'] = detect_events(dec, 0, 0, 40000, 0, 40000, TAPS65, 14.0, 2, 1, 30, 5)
    row, pos, _ = _EVENTS['all']
    keep = ~(((row >= 12000) & (row < 13000)) | ((row >= 22000) & (row < 22800)) | ((row >= 31000) & (row < 31600)))
    row, pos = row[keep], pos[keep]
    order = np.random.RandomState(7).permutation(row.size)              # the caller's order is not the rows'
    return row[order], pos[order]


def test_bit_identity_cache_lanes_calls_and_the_device_entry(tmp_cfg, monkeypatch):
    x = synth_int16(0, 40000, 40, 4)
    one, dec = _make(tmp_cfg, x, 5000, codec=api.HipCodec(devices=[0]))
    two = _open(tmp_cfg, codec=api.HipCodec(devices=[0, 0]))
    sample, channel = _events_with_gaps(dec)
    assert sample.size >= 300
    kw = dict(before=20, after=41, neighbours=8, taps=TAPS65, reference='median')
    want = _check(one, dec, sample, channel, **kw)
    assert hip.waveforms_last_plan(0)['slabs'] >= 1
    _same(one.waveforms(sample, channel, **kw), want)                                              # the same call twice
    _same(two.waveforms(sample, channel, **kw), want)                                              # one device == two lanes
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1)
    _same(one.waveforms(sample, channel, **kw), want)
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1 << 30)
    monkeypatch.setattr(api, 'WAVEFORMS_OUT_BYTES', 7 * (4 * 61 * 17 + 16))                        # 7 events per call
    _same(one.waveforms(sample, channel, **kw), want)
    monkeypatch.setattr(api, 'WAVEFORMS_OUT_BYTES', 1 << 30)
    keys = list(range(one.n_chunks))
    one[:]                                                                                         # (read-ahead makes chunks resident)
    for k in range(one.n_chunks):
        one[one.chunk_bounds[k]:one.chunk_bounds[k] + 1]
    cache = one._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 40 for b in before) >= len(keys) // 2
    _same(one.waveforms(sample, channel, **kw), want)                                              # resident == cold
    assert hip.cache_query(cache, keys).tolist() == before                                         # the gather changed nothing
    # mts_dev_waveforms on the file's chunks in device memory, the events by ascending row
    data = (tmp_cfg / 'd.cbin').read_bytes()
    cbuf = hip.DevBuffer(len(data) + 256)
    host = np.frombuffer(data + b'\0' * 256, dtype=np.uint8).copy()
    hip._check(hip.lib().mts_dev_copy(0, None, cbuf.at(), hip._ptr(host), host.nbytes, 0), 'mts_dev_copy')
    offs, bounds = np.asarray(one.chunk_offsets, np.int64), np.asarray(one.chunk_bounds, np.int64)
    order = np.argsort(sample, kind='stable')
    for want_wave in (True, False):
        st, res, out = hip.dev_waveforms(cbuf, offs[:-1], np.diff(offs), bounds[:-1], np.diff(bounds), 40, np.int16, one._flags(), 0, 40000, TAPS65,
                                         np.arange(40), 1, sample[order], (channel - 8)[order], 20, 41, 17, want_wave)
        assert st == [0] * one.n_chunks and hip.waveforms_last_plan(0)['pieces'] == 1
        if want_wave:
            assert res[0].tobytes() == want.waveforms[order].tobytes()
        else:
            assert res[0] is None
        assert res[1].tobytes() == want.trough.value[order].tobytes() and res[3].tobytes() == want.peak.value[order].tobytes()
        assert np.array_equal(res[2], want.trough.index[order]) and np.array_equal(res[4], want.peak.index[order])
        out.free()
    cbuf.free()
    one.close()
    two.close()


CHILD = """
import json, sys, numpy as np, mtscomp_amd
sys.path.insert(0, %r)
from mtscomp_amd import api, hip
ev = np.load(sys.argv[1])
r = mtscomp_amd.decompress(%r, %r, check_after_decompress=False, codec=api.HipCodec(devices=[0]))
r._dev_cache_bytes = 0
w = r.waveforms(ev['s'], ev['c'], before=20, after=41, neighbours=8, taps=api.highpass_taps(300, 5000, 65), reference='median')
np.savez(sys.argv[2], w=w.waveforms, a=w.trough.value, b=w.trough.index, c=w.peak.value, d=w.peak.index)
print('PLAN ' + json.dumps(hip.waveforms_last_plan(0)))
"""


def test_pieces_slabs_and_gaps_do_not_change_the_result(tmp_cfg):
    x = synth_int16(0, 40000, 40, 4)
    r, dec = _make(tmp_cfg, x, 5000)
    sample, channel = _events_with_gaps(dec)
    want = r.waveforms(sample, channel, before=20, after=41, neighbours=8, taps=TAPS65, reference='median')
    r.close()
    np.savez(tmp_cfg / 'ev.npz', s=sample, c=channel)
    script = CHILD % (os.getcwd(), str(tmp_cfg / 'd.cbin'), str(tmp_cfg / 'd.ch'))
    plans = []
    # the chunks hold 400 000 bytes each: pieces of one chunk; slabs of 640 rows; the three empty stretches are gaps at 200 rows
    for pipe, slab, gap in ((None, None, None), (200 << 10, 100 << 10, 200), (200 << 10, None, -1), (None, 1, 0)):
        env = dict(os.environ)
        for name, v in (('MTS_PIPE_BYTES', pipe), ('MTS_WAVEFORMS_SLAB_BYTES', slab), ('MTS_WAVEFORMS_GAP_ROWS', gap)):
            env.pop(name, None)
            if v is not None:
                env[name] = str(v)
        p = tmp_cfg / ('o%d.npz' % len(plans))
        run = subprocess.run([sys.executable, '-c', script, str(tmp_cfg / 'ev.npz'), str(p)], env=env, check=True, timeout=300,
                             capture_output=True, text=True)
        plans.append(json.loads([ln for ln in run.stdout.splitlines() if ln.startswith('PLAN ')][-1][5:]))
        got = np.load(p)
        assert got['w'].tobytes() == want.waveforms.tobytes(), plans[-1]
        assert got['a'].tobytes() == want.trough.value.tobytes() and got['b'].tobytes() == want.trough.index.tobytes()
        assert got['c'].tobytes() == want.peak.value.tobytes() and got['d'].tobytes() == want.peak.index.tobytes()
    print(plans)
    assert plans[1]['pieces'] >= 3 and plans[1]['slabs'] >= 3 and plans[1]['gap_cuts'] >= 2, plans
    assert plans[2]['pieces'] >= 3 and plans[2]['gap_cuts'] == 0, plans
    assert plans[3]['slabs'] >= 100 and plans[0]['slabs'] < plans[1]['slabs'], plans          # (a cap of one row: T rows, nearly a slab per event)


def _damage(tmp, k, offsets):
    shutil.copy(tmp / 'good.cbin', tmp / 'd.cbin')
    data = bytearray((tmp / 'd.cbin').read_bytes())
    data[offsets[k] + 30:offsets[k] + 60] = b'\x00' * 30
    (tmp / 'd.cbin').write_bytes(bytes(data))
    return _open(tmp)


def test_sparse_list_and_damaged_chunks(tmp_cfg):
    x = synth_int16(0, 16000, 16, 4)
    r, dec = _make(tmp_cfg, x, 2000)
    assert r.n_chunks == 8
    b, o = r.chunk_bounds, r.chunk_offsets
    sample = np.array([b[5] + 700, 300, b[5] + 100, 1500, b[6] - 200, 0])          # chunks 0 and 5
    channel = np.arange(6)
    want = _check(r, dec, sample, channel, neighbours=3, taps=TAPS65, reference='median')
    r.close()
    shutil.copy(tmp_cfg / 'd.cbin', tmp_cfg / 'good.cbin')
    kw = dict(neighbours=3, taps=TAPS65, reference='median')
    r = _damage(tmp_cfg, 3, o)                                           # not read: nothing is raised
    _same(r.waveforms(sample, channel, **kw), want)
    with pytest.raises(IOError, match='#3'):
        r[b[3]:b[3] + 10]
    r.close()
    r = _damage(tmp_cfg, 5, o)
    with pytest.raises(IOError, match='#5'):
        r.waveforms(sample, channel, **kw)
    with pytest.raises(IOError, match='#5'):
        r.waveforms([b[5] - 41 - 32 + 1], [2], **kw)                     # rows of chunk 4 alone; the filter support of the last reaches chunk 5
    r.waveforms([b[5] - 41 - 32], [2], **kw)
    with pytest.raises(IOError, match='#5'):
        r.waveforms([b[6] + 20 + 32 - 1], [2], **kw)                     # ... and from above: row - 20 + 32 - 64
    r.waveforms([b[6] + 20 + 32], [2], **kw)
    r.waveforms(sample[[1, 3, 5]], channel[[1, 3, 5]], **kw)
    r.close()


def test_c_abi_arguments():
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = np.arange(400, dtype=np.int16).reshape(100, nc)
    z = hip.compress_chunks(x, [0, 100], hip.make_flags(), 6)[0]
    data = np.frombuffer(z + b'\0' * 16, dtype=np.uint8)
    cbuf = hip.DevBuffer(len(z) + 256)
    host = np.frombuffer(z + b'\0' * 256, dtype=np.uint8).copy()
    hip._check(L.mts_dev_copy(0, None, cbuf.at(), hip._ptr(host), host.nbytes, 0), 'mts_dev_copy')
    d_out = hip.DevBuffer(1 << 20)
    keep = []

    def call(dev=False, row0=0, rows=100, taps=(1.0, 0.5), vb=0, ve=100, cols=(0, 1), ref=0, ev=(10, 10, 50), col0=(0, -1, 1), n_ev=None,
             before=2, after=3, width=2, itemsize=2, flags=hip.make_flags(), wave=True, ext=(1, 1, 1, 1), events=True):
        a = [np.array(v, dtype=np.int64) for v in ([0], [row0], [0], [len(z)], [rows])]
        c, t = np.array(cols, dtype=np.int32), np.array(taps, dtype=np.float64)
        er, ec = np.array(ev, dtype=np.int64), np.array(col0, dtype=np.int32)
        o = (np.full(4096, 5, np.float32), np.full(16, 5, np.float32), np.full(16, 5, np.int32), np.full(16, 5, np.float32), np.full(16, 5, np.int32))
        st = np.full(1, 99, np.int32)
        keep.append((a, c, t, er, ec, o, st))
        lp = [v.ctypes.data_as(C.POINTER(C.c_long)) for v in a]
        n = len(er) if n_ev is None else n_ev
        mid = (vb, ve, len(t), t.ctypes.data_as(C.POINTER(C.c_double)), len(c), c.ctypes.data_as(C.POINTER(C.c_int)), ref, n,
               er.ctypes.data_as(C.POINTER(C.c_long)) if events else None, ec.ctypes.data_as(C.POINTER(C.c_int)) if events else None,
               before, after, width)
        stp = st.ctypes.data_as(C.POINTER(C.c_int))
        if dev:
            po = [d_out.at(0)] + [d_out.at((1 << 19) + 4096 * k) for k in range(4)]
        else:
            po = [hip._ptr(v) for v in o]
        po = [po[0] if wave else None] + [p if e else None for p, e in zip(po[1:], ext)]
        if dev:
            rc = L.mts_dev_waveforms(0, None, cbuf.at(), lp[2], lp[3], lp[1], lp[4], 1, nc, itemsize, flags, *mid, *po, stp)
        else:
            rc = L.mts_waveforms(0, 0, 1, lp[0], lp[1], data.ctypes.data_as(C.c_void_p), lp[2], lp[3], lp[4], nc, itemsize, flags, *mid, *po, stp)
        return rc, int(st[0]), o
    for dev in (False, True):
        rc, st, o = call(dev=dev)
        assert (rc, st) == (0, 0)
        if not dev:
            want = waveforms(x[:, :2], 0, 0, 100, [1.0, 0.5], 0, [10, 10, 50], [0, -1, 1], 2, 3, 2)
            assert o[0][:30].tobytes() == want[0].tobytes() and o[0][30] == 5
            assert [o[k][:3].tolist() for k in (1, 2, 3, 4)] == [want[k].tolist() for k in (1, 2, 3, 4)]
            rc, st, o2 = call(wave=False)                                # out_wave NULL: the extrema alone, the same bytes
            assert (rc, st) == (0, 0) and (o2[0] == 5).all()
            assert all(o2[k].tobytes() == o[k].tobytes() for k in (1, 2, 3, 4))
        rc, st, o = call(dev=dev, ev=(), col0=())                        # no events: MTS_OK, nothing written
        assert (rc, st) == (0, 0) and (o[1] == 5).all()
        assert call(dev=dev, n_ev=0, events=False)[:2] == (0, 0)
        assert call(dev=dev, before=0, after=1, width=1)[:2] == (0, 0) and call(dev=dev, before=4096, after=0, width=1, wave=False)[:2] == (0, 0)
        others = (dict(ev=(10, 9, 50)), dict(ev=(10, 10, 100)), dict(ev=(-1, 10, 50)), dict(vb=20), dict(ve=40),
                  dict(before=-1), dict(after=-1), dict(before=0, after=0), dict(before=4096, after=1), dict(before=2 ** 31 - 1, after=2),
                  dict(width=0), dict(width=-3), dict(width=1025), dict(n_ev=-1), dict(n_ev=(1 << 40) + 1), dict(events=False),
                  dict(ext=(0, 1, 1, 1)), dict(ext=(1, 0, 1, 1)), dict(ext=(1, 1, 0, 1)), dict(ext=(1, 1, 1, 0)), dict(ext=(0, 0, 0, 0)),
                  dict(taps=(np.inf, 1.0)), dict(cols=(0, 4)), dict(cols=(-1,)), dict(row0=10), dict(rows=50), dict(itemsize=3),
                  dict(flags=hip.FLAG_FLOAT, itemsize=2))
        # (a shared argument, one bad at a time: the text is the one the library gave before the five ops shared their checks)
        for bad, text in [(b, None) for b in others] + filter_errors('waveforms', rows_too=False) + wide_errors('waveforms'):
            rc, st, o = call(dev=dev, **bad)
            assert rc == -1, bad                                       # MTS_E_ARG ...
            assert st == 99 and (dev or all((v == 5).all() for v in o)), bad       # ... before anything ran
            said = hip.lib().mts_last_error().decode()
            assert said and text in (None, said), (bad, said)
    d_out.free()
    cbuf.free()
