"""mts_mean_waveforms / mts_dev_mean_waveforms and the Reader on top of them on the MI355X: k_mean_waveforms against the numpy
restatement of the definition (tests/mean_waveforms_oracle.py), for equality of every byte of sum, count and skipped: tile seams on
the scalar and the vector path, part seams, clipping at every edge, ties, skipped values and the limit, every seam of the host side
(chunks, pieces, slabs, gaps, residency), the sums formed from mts_dev_waveforms' own snippets, the Reader, argument errors."""
import ctypes as C

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.mean_waveforms_oracle import mean_of, mean_waveforms

pytestmark = pytest.mark.gpu

TAPS9 = np.random.RandomState(1).randn(9)
TAPS65 = api.highpass_taps(300, 5000, 65)
NAMES = ('sum', 'count', 'skipped')


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


class Chunks:
    """x compressed on the device in chunks of chunk_rows rows, as the two entry points take them."""

    def __init__(self, x, chunk_rows):
        hip.require_device()
        self.x, self.rows, self.nc = x, x.shape[0], x.shape[1]
        self.bounds = np.asarray(list(range(0, self.rows, chunk_rows)) + [self.rows], np.int64)
        self.flags = hip.make_flags(x.dtype.kind != 'f', False, 'F')
        z = hip.compress_chunks(x, self.bounds, self.flags, 6)
        self.data = b''.join(z)
        self.lens = np.asarray([len(b) for b in z], np.int64)
        self.offs = np.concatenate(([0], np.cumsum(self.lens)))[:-1]
        self.keys = list(range(len(z)))
        self.cbuf = None

    def host(self):
        return (0, self.keys, self.bounds[:-1], self.data, self.offs, self.lens, np.diff(self.bounds), self.nc, self.x.dtype, self.flags)

    def dev(self):
        if self.cbuf is None:
            self.cbuf = hip.DevBuffer(len(self.data) + 256)
            host = np.frombuffer(self.data + b'\0' * 256, dtype=np.uint8).copy()
            hip._check(hip.lib().mts_dev_copy(0, None, self.cbuf.at(), hip._ptr(host), host.nbytes, 0), 'mts_dev_copy')
        return (self.cbuf, self.offs, self.lens, self.bounds[:-1], np.diff(self.bounds), self.nc, self.x.dtype, self.flags)

    def mean(self, dev, *args):
        """(sum, count, skipped) of mts_dev_mean_waveforms / mts_mean_waveforms for the op's own arguments."""
        if dev:
            st, res, buf = hip.dev_mean_waveforms(*self.dev(), *args)
            buf.free()
        else:
            st, *res = hip.mean_waveforms(*self.host(), *args)
        assert st == [0] * len(self.keys)
        return tuple(res)

    def waveforms(self, *args):
        st, res, buf = hip.dev_waveforms(*self.dev(), *args)
        buf.free()
        assert st == [0] * len(self.keys)
        return res[0]

    def free(self):
        if self.cbuf is not None:
            self.cbuf.free()


def _same(got, want, what=None):
    for g, w, name, t in zip(got, want, NAMES, (np.int64, np.int32, np.int64)):
        assert g.dtype == t and g.shape == w.shape, (name, what)
        assert g.tobytes() == w.tobytes(), (name, what, np.argwhere(g != w)[:4].tolist())


def _events(rs, rows, n_cols, width, n, n_labels):
    """n events by ascending row: both ends of the recording, repeats, first positions from left of the columns to right of them."""
    row = np.sort(np.concatenate(([0, 0, 1, rows - 1, rows - 1, rows - 2, rows // 2, rows // 2, rows // 2], rs.randint(0, rows, n - 9)))).astype(np.int64)
    col0 = rs.randint(-width, n_cols + 1, n)
    col0[:4] = [0, -width + 1, n_cols - 1, max(0, n_cols - width)]
    return row, col0.astype(np.int64), rs.randint(0, n_labels, n).astype(np.int64)


# T, W, n_channels, the columns: T * W of 1, 15, 255, 256, 257 and 61 * 17 = 1037 (the scalar path below 1024 entries, the vector path
# from there on: 1037 leaves a tile of 13 entries and a thread with one of its four), then the vector path's three kinds of thread:
# four entries in one row (W % 4 == 0), rows as wide as z that follow each other in memory (an odd and an even n_cols), neither
SHAPES = [(1, 1, 5, None), (3, 5, 7, None), (15, 17, 21, None), (16, 16, 16, None), (257, 1, 3, None), (61, 17, 70, None),
          (64, 16, 20, None), (40, 33, 35, list(range(34, 1, -1))), (35, 36, 36, None), (300, 7, 9, None), (61, 17, 17, None)]


@pytest.mark.parametrize('T,W,nc,cols', SHAPES)
def test_tile_seams_on_both_paths(T, W, nc, cols):
    rs = np.random.RandomState(T * 1000 + W)
    rows = 2500
    cols = np.arange(nc) if cols is None else np.asarray(cols)
    n_cols = cols.size
    assert (T * W >= 1024) == ((T, W) in ((61, 17), (64, 16), (40, 33), (35, 36), (300, 7)))
    case = 0
    for dtype in (np.int16, np.float32):
        x = synth_int16(0, rows, nc, T + W) if dtype == np.int16 else (rs.randn(rows, nc) * 300).astype(np.float32)
        ck = Chunks(x, 700)
        for before in sorted({0, T // 3, T}):
            row, col0, label = _events(rs, rows, n_cols, W, 70, 5)
            if W == n_cols:
                col0[::2] = 0                                            # full-width snippets: whole rows of z, one behind the other
            ref, taps = case % 2, (TAPS9 if case % 3 else [1.0])
            case += 1
            args = (0, rows, taps, cols, ref, row, col0, label, 5, before, T - before, W, 2.0 ** -10)
            want = mean_waveforms(x[:, cols], 0, *args[:3], *args[4:])
            assert want[1].any() and want[1].min() < want[1].max()
            for dev in (False, True):
                _same(ck.mean(dev, *args), want, (dtype, before, dev))
        ck.free()


def test_part_seams(monkeypatch):
    rs = np.random.RandomState(3)
    rows, nc = 1500, 12
    x = synth_int16(0, rows, nc, 9)
    ck = Chunks(x, 400)

    def run(row, col0, label, K, expect_same=True):
        row, col0, label = (np.asarray(a, np.int64) for a in (row, col0, label))
        args = (0, rows, TAPS9, np.arange(nc), 1, row, col0, label, K, 4, 7, 5, 2.0 ** -16)
        want = mean_waveforms(x, 0, *args[:3], *args[4:])
        for part in ('2', None, '1', '3', '1000000'):
            if part is None:
                monkeypatch.delenv('MTS_MEAN_PART_EVENTS', raising=False)
            else:
                monkeypatch.setenv('MTS_MEAN_PART_EVENTS', part)
            for dev in (False, True):
                _same(ck.mean(dev, *args), want, (part, dev, K))
        monkeypatch.delenv('MTS_MEAN_PART_EVENTS', raising=False)
    # labels of 0, 1, 2, 3 and 5 events in one slab, interleaved
    label = np.array([4, 1, 3, 4, 2, 4, 3, 2, 4, 3, 4])
    assert np.bincount(label, minlength=5).tolist() == [0, 1, 2, 3, 5]
    row = np.sort(rs.randint(100, 300, label.size))
    run(row, rs.randint(-2, 10, label.size), label, 5)
    assert hip.waveforms_last_plan(0)['slabs'] == 1
    # all events on one label: more than an LDS batch of them, with repeats
    row = np.sort(rs.randint(0, rows, 700))
    run(row, rs.randint(-4, 12, 700), np.full(700, 2), 3)
    # one event per label, n_labels 1 and 300
    run([700], [3], [0], 1)
    run(np.sort(rs.randint(0, rows, 300)), rs.randint(-4, 12, 300), rs.permutation(300), 300)
    # no events: zeros, both entries
    for dev in (False, True):
        got = ck.mean(dev, 0, rows, TAPS9, np.arange(nc), 1, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), 3, 4, 7, 5, 1.0)
        assert got[0].shape == (3, 11, 5) and not got[0].any() and not got[1].any() and not got[2].any()
    ck.free()


def test_clipping_counts_per_entry():
    rows, nc, T, W = 900, 10, 9, 6
    x = synth_int16(0, rows, nc, 2)
    ck = Chunks(x, 250)
    row = np.array([0, 0, 1, 3, 450, rows - 4, rows - 1, rows - 1], np.int64)
    col0 = np.array([-5, 0, nc - 1, -2, nc - W, nc - W + 1, nc - 2, -W + 1], np.int64)            # left of 0 and past n_cols - width
    label = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int64)
    args = (0, rows, [1.0], np.arange(nc), 0, row, col0, label, 2, 4, 5, W, 1.0)
    want = mean_waveforms(x, 0, *args[:3], *args[4:])
    # every (tau, w) has its own count: rows clipped at both ends, positions at both edges
    for k in (0, 1):                                                     # rows clipped at one end, positions at both edges
        assert len(np.unique(want[1][k])) >= 3 and len(np.unique(want[1][k].sum(axis=1))) >= 3 and len(np.unique(want[1][k].sum(axis=0))) >= 3
    assert want[1].min() == 0 and want[1].max() >= 3
    for dev in (False, True):
        _same(ck.mean(dev, *args), want, dev)
    # the recording a window of the chunks' rows: the valid range clips as the file's ends do
    args = (200, 700, TAPS9, np.arange(nc), 1, np.array([200, 201, 699]), np.array([0, -1, 5]), np.array([0, 1, 1]), 2, 4, 5, W, 0.5)
    want = mean_waveforms(x[200:700], 200, *args[:3], *args[4:])
    for dev in (False, True):
        _same(ck.mean(dev, *args), want, dev)
    ck.free()


def test_ties_round_half_to_even():
    rs = np.random.RandomState(4)
    rows, nc = 1200, 6
    x = rs.randint(-40, 41, (rows, nc)).astype(np.int16)
    # with resolution 2 every odd sample is a tie: both signs, and halves that round down and up to reach an even number
    odd = x[x % 2 != 0].astype(np.int64)
    for sign in (-1, 1):
        for parity in (0, 1):
            assert ((np.sign(odd) == sign) & (np.floor(odd / 2.0) % 2 == parity)).sum() > 100
    ck = Chunks(x, 500)
    row = np.sort(rs.randint(0, rows, 200)).astype(np.int64)
    label = rs.randint(0, 3, 200)
    args = (0, rows, [1.0], np.arange(nc), 0, row, np.zeros(200, np.int64), label, 3, 2, 3, nc, 2.0)
    want = mean_waveforms(x, 0, *args[:3], *args[4:])
    assert not want[2].any()
    # (what the test is about, said once more without the oracle: Python's round is half to even)
    e = 17
    assert want[0][label[e]].sum() >= -10 ** 9 and row[e] >= 2
    lone = mean_waveforms(x, 0, 0, rows, [1.0], 0, row[e:e + 1], [0], [0], 1, 2, 3, nc, 2.0)[0][0]
    a, b = max(0, int(row[e]) - 2), min(rows, int(row[e]) + 3)
    assert lone[a - int(row[e]) + 2:b - int(row[e]) + 2].tolist() == [[round(int(v) / 2) for v in r] for r in x[a:b]]
    for dev in (False, True):
        _same(ck.mean(dev, *args), want, dev)
    ck.free()


@pytest.mark.parametrize('expo', [-16, -60, 60, 0])
def test_skipped_values_and_the_limit(expo):
    rs = np.random.RandomState(5)
    rows, nc = 800, 5
    resolution = 2.0 ** expo
    limit = np.float32(2.0 ** (42 + expo))                               # |z| >= limit is skipped
    x = (rs.randn(rows, nc) * 2.0 ** (expo + 20)).astype(np.float32)     # |d| around 2^20
    under = np.nextafter(limit, np.float32(0))
    x[100, 0], x[101, 1], x[102, 2] = np.nan, np.inf, -np.inf
    x[103, 3], x[104, 4], x[105, 0], x[106, 1] = limit, under, -limit, -under
    x[300:304] = np.nan                                                  # whole rows
    x[400, 2], x[401, 2] = 0.0, -0.0
    ck = Chunks(x, 300)
    row = np.sort(np.concatenate(([100, 102, 102, 104, 106, 301, 302, 400], rs.randint(0, rows, 60)))).astype(np.int64)
    label = rs.randint(0, 4, row.size)
    args = (0, rows, [1.0], np.arange(nc), 0, row, np.zeros(row.size, np.int64), label, 4, 3, 4, nc, resolution)
    want = mean_waveforms(x, 0, *args[:3], *args[4:])
    assert want[2].sum() >= 5 + 4 * nc * 2 and want[2].all()             # the planted values are skipped, under every label
    one = mean_waveforms(x, 0, 0, rows, [1.0], 0, [104], [0], [0], 1, 1, 3, nc, resolution)
    assert one[2][0] == 2 and one[1][0, 0, 3] == 0 and one[1][0, 1, 4] == 1 and one[1][0, 2, 0] == 0 and one[1][0, 3, 1] == 1
    assert abs(int(one[0][0, 1, 4])) == int(float(under) / resolution) == 2 ** 42 - 2 ** 18
    for dev in (False, True):
        _same(ck.mean(dev, *args), want, (expo, dev))
    ck.free()


def test_host_seams_and_the_snippets_of_dev_waveforms(monkeypatch):
    rs = np.random.RandomState(6)
    rows, nc = 6000, 16
    x = synth_int16(0, rows, nc, 11)
    row = rs.randint(0, rows, 260)
    row = np.sort(row[((row < 1200) | (row >= 1800)) & ((row < 4300) | (row >= 4800))]).astype(np.int64)      # two stretches without events, each inside a chunk
    n = row.size
    col0, label = rs.randint(-3, nc, n).astype(np.int64), rs.randint(0, 6, n)
    args = (0, rows, TAPS65, np.arange(nc), 1, row, col0, label, 6, 20, 41, 7, 2.0 ** -16)
    want = mean_waveforms(x, 0, *args[:3], *args[4:])
    knobs = ('MTS_PIPE_BYTES', 'MTS_WAVEFORMS_SLAB_BYTES', 'MTS_WAVEFORMS_GAP_ROWS', 'MTS_MEAN_PART_EVENTS')
    plans = []
    for chunk, pipe, slab, gap, part in ((1000, None, None, None, None), (1000, 40000, 20000, 100, None), (700, 40000, None, -1, '5'),
                                         (6000, None, 1, 0, None), (1000, None, 30000, None, '2')):
        ck = Chunks(x, chunk)
        for name, v in zip(knobs, (pipe, slab, gap, part)):
            monkeypatch.delenv(name, raising=False)
            if v is not None:
                monkeypatch.setenv(name, str(v))
        _same(ck.mean(False, *args), want, (chunk, pipe, slab, gap, part))
        plans.append(hip.waveforms_last_plan(0))
        _same(ck.mean(True, *args), want, (chunk, pipe, slab, gap, part, 'dev'))
        ck.free()
    for name in knobs:
        monkeypatch.delenv(name, raising=False)
    print(plans)
    # chunks of 32 000 bytes: pieces of one chunk; slabs of 312 rows; the two empty stretches are gaps at 100 rows
    assert plans[1]['pieces'] >= 3 and plans[1]['slabs'] > plans[0]['slabs'] and plans[1]['gap_cuts'] >= 2, plans
    assert plans[2]['pieces'] >= 3 and plans[2]['gap_cuts'] == 0, plans
    assert plans[3]['slabs'] >= 100 and plans[4]['slabs'] >= 3, plans    # (a cap of one row: T rows, nearly a slab per event)
    # the same sums formed from mts_dev_waveforms' own snippets of the same events
    ck = Chunks(x, 1000)
    w = ck.waveforms(0, rows, TAPS65, np.arange(nc), 1, row, col0, 20, 41, 7)
    inside = ~np.isnan(w)                                                # (int16 data through finite taps: every NaN is a fill entry)
    q = np.rint(w.astype(np.float64) / 2.0 ** -16)
    total, count = np.zeros((6, 61, 7), np.int64), np.zeros((6, 61, 7), np.int32)
    e, tau, pos = np.nonzero(inside)
    np.add.at(total, (label[e], tau, pos), q[inside].astype(np.int64))
    np.add.at(count, (label[e], tau, pos), 1)
    assert total.tobytes() == want[0].tobytes() and count.tobytes() == want[1].tobytes() and not want[2].any()
    ck.free()


def test_reader_on_detects_events_resident_cold_and_lanes(tmp_cfg, monkeypatch):
    x = synth_int16(0, 12000, 40, 4)
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=3000., n_channels=40, dtype=x.dtype, check_after_compress=False)
    one = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, codec=api.HipCodec(devices=[0]))
    two = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, codec=api.HipCodec(devices=[0, 0]))
    assert one.n_chunks >= 4
    ev = one.detect(14.0, taps=TAPS65, sign='both', reference='median', exclude=30, spread=5)
    assert ev.sample.size >= 100
    label = ev.channel % 5
    kw = dict(neighbours=8, taps=TAPS65, reference='median')
    cold = one.mean_waveforms(ev.sample, label, ev.channel, **kw)
    want = mean_waveforms(x, 0, 0, 12000, TAPS65, 1, ev.sample, ev.channel - 8, label, 5, 20, 41, 17, 2.0 ** -16)
    assert cold.sum.tobytes() == want[0].tobytes() and cold.count.tobytes() == want[1].astype(np.int64).tobytes()
    assert cold.skipped.tobytes() == want[2].tobytes() and cold.events.tolist() == np.bincount(label, minlength=5).tolist()
    assert cold.mean.tobytes() == mean_of(want[0], want[1], 2.0 ** -16).tobytes() and cold.mean.shape == (5, 61, 17)

    def same(b):
        for key in ('sum', 'count', 'skipped', 'events', 'mean'):
            assert b[key].tobytes() == cold[key].tobytes(), key
    order = np.random.RandomState(8).permutation(ev.sample.size)
    same(one.mean_waveforms(ev.sample[order], label[order], ev.channel[order], **kw))              # any order
    same(two.mean_waveforms(ev.sample, label, ev.channel, **kw))                                   # one device == two lanes
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1)
    same(one.mean_waveforms(ev.sample, label, ev.channel, **kw))
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1 << 30)
    monkeypatch.setattr(api, 'MEAN_WAVEFORMS_EVENT_BYTES', 7 * 24)                                  # 7 events per call
    same(one.mean_waveforms(ev.sample, label, ev.channel, **kw))
    monkeypatch.setattr(api, 'MEAN_WAVEFORMS_EVENT_BYTES', 1 << 28)
    keys = list(range(one.n_chunks))
    one[:]                                                                                         # (read-ahead makes chunks resident)
    for k in range(one.n_chunks):
        one[one.chunk_bounds[k]:one.chunk_bounds[k] + 1]
    cache = one._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 40 for b in before) >= len(keys) // 2
    same(one.mean_waveforms(ev.sample, label, ev.channel, **kw))                                   # resident == cold
    assert hip.cache_query(cache, keys).tolist() == before                                         # the sum inserted nothing
    # full width: np.nan_to_num(mean) is a templates argument
    full = one.mean_waveforms(ev.sample, label, taps=TAPS65, reference='median')
    want = mean_waveforms(x, 0, 0, 12000, TAPS65, 1, ev.sample, np.zeros(ev.sample.size, int), label, 5, 20, 41, 40, 2.0 ** -16)
    assert full.sum.tobytes() == want[0].tobytes() and full.count.tobytes() == want[1].astype(np.int64).tobytes()
    sc = one.correlate(np.nan_to_num(full.mean), start=1000, stop=1200, before=20, taps=TAPS65, reference='median')
    assert sc.shape == (200, 5) and np.isfinite(sc).all()
    one.close()
    two.close()


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

    def call(dev=False, row0=0, rows=100, taps=(1.0, 0.5), vb=0, ve=100, cols=(0, 1), ref=0, ev=(10, 10, 50), col0=(0, -1, 1), lab=(0, 2, 2),
             n_ev=None, K=3, before=2, after=3, width=2, res=0.5, itemsize=2, flags=hip.make_flags(), outs=(1, 1, 1), events=True, labels=True):
        a = [np.array(v, dtype=np.int64) for v in ([0], [row0], [0], [len(z)], [rows])]
        c, t = np.array(cols, dtype=np.int32), np.array(taps, dtype=np.float64)
        er, ec, el = np.array(ev, dtype=np.int64), np.array(col0, dtype=np.int32), np.array(lab, dtype=np.int32)
        o = (np.full(4096, 5, np.int64), np.full(4096, 5, np.int32), np.full(16, 5, np.int64))
        st = np.full(1, 99, np.int32)
        keep.append((a, c, t, er, ec, el, o, st))
        lp = [v.ctypes.data_as(C.POINTER(C.c_long)) for v in a]
        n = len(er) if n_ev is None else n_ev
        ip = C.POINTER(C.c_int)
        mid = (vb, ve, len(t), t.ctypes.data_as(C.POINTER(C.c_double)), len(c), c.ctypes.data_as(ip), ref, n,
               er.ctypes.data_as(C.POINTER(C.c_long)) if events else None, ec.ctypes.data_as(ip) if events else None,
               el.ctypes.data_as(ip) if labels else None, K, before, after, width, res)
        stp = st.ctypes.data_as(ip)
        po = [d_out.at((1 << 18) * k) for k in range(3)] if dev else [hip._ptr(v) for v in o]
        po = [p if e else None for p, e in zip(po, outs)]
        if dev:
            rc = L.mts_dev_mean_waveforms(0, None, cbuf.at(), lp[2], lp[3], lp[1], lp[4], 1, nc, itemsize, flags, *mid, *po, stp)
        else:
            rc = L.mts_mean_waveforms(0, 0, 1, lp[0], lp[1], data.ctypes.data_as(C.c_void_p), lp[2], lp[3], lp[4], nc, itemsize, flags, *mid, *po, stp)
        return rc, int(st[0]), o
    for dev in (False, True):
        rc, st, o = call(dev=dev)
        assert (rc, st) == (0, 0)
        if not dev:
            want = mean_waveforms(x[:, :2], 0, 0, 100, [1.0, 0.5], 0, [10, 10, 50], [0, -1, 1], [0, 2, 2], 3, 2, 3, 2, 0.5)
            assert o[0][:30].tobytes() == want[0].tobytes() and o[1][:30].tobytes() == want[1].tobytes() and o[2][:3].tobytes() == want[2].tobytes()
            assert o[0][30] == 5 and o[1][30] == 5 and o[2][3] == 5
            rc, st, o = call(ev=(), col0=(), lab=())                     # no events: zeros, written whole
            assert (rc, st) == (0, 0) and not o[0][:30].any() and not o[1][:30].any() and not o[2][:3].any() and o[0][30] == 5 and o[2][3] == 5
        assert call(dev=dev, n_ev=0, events=False, labels=False)[:2] == (0, 0)
        assert call(dev=dev, before=0, after=1, width=1, K=1, lab=(0, 0, 0))[:2] == (0, 0)
        assert call(dev=dev, res=2.0 ** 60)[:2] == (0, 0) and call(dev=dev, res=2.0 ** -60)[:2] == (0, 0)
        for bad in (dict(ev=(10, 9, 50)), dict(ev=(10, 10, 100)), dict(ev=(-1, 10, 50)), dict(vb=20), dict(ve=40),
                    dict(before=-1), dict(after=-1), dict(before=0, after=0), dict(before=4096, after=1), dict(width=0), dict(width=1025),
                    dict(n_ev=-1), dict(events=False), dict(labels=False), dict(lab=(0, 3, 2)), dict(lab=(0, -1, 2)), dict(K=0), dict(K=-2),
                    dict(K=4097), dict(K=4096, before=2048, after=2048, width=9), dict(K=2, lab=(0, 2, 1)),
                    dict(res=0.0), dict(res=-1.0), dict(res=3.0), dict(res=2.0 ** 61), dict(res=2.0 ** -61), dict(res=float('nan')),
                    dict(res=float('inf')), dict(outs=(0, 1, 1)), dict(outs=(1, 0, 1)), dict(outs=(1, 1, 0)),
                    dict(taps=(np.inf, 1.0)), dict(taps=()), dict(cols=(0, 4)), dict(cols=(-1,)), dict(cols=()), dict(ref=2), dict(row0=10),
                    dict(rows=50), dict(itemsize=3), dict(flags=hip.FLAG_FLOAT, itemsize=2)):
            rc, st, o = call(dev=dev, **bad)
            assert rc == -1, bad                                       # MTS_E_ARG ...
            assert st == 99 and (dev or all((v == 5).all() for v in o)), bad       # ... before anything ran
            said = hip.lib().mts_last_error().decode()
            assert said, bad
            if set(bad) & {'K', 'lab', 'res', 'labels', 'outs'}:
                assert said.startswith('mean_waveforms:'), (bad, said)
    # a label with more than 2^21 events in a call
    many = (1 << 21) + 1
    rc, st, _ = call(ev=np.full(many, 10), col0=np.zeros(many), lab=np.zeros(many))
    assert (rc, st) == (-1, 99) and 'more than' in hip.lib().mts_last_error().decode()
    d_out.free()
    cbuf.free()
