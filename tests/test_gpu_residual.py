"""mts_residual / mts_match_residual, their device variants and the Reader on top of them on the MI355X: k_subtract against the numpy
restatement of the definition (tests/residual_oracle.py), for exact equality of every byte: the vector and the scalar path, template
lengths and offsets, ties, deep overlaps, more events than an LDS batch, both ends of the recording, every seam (chunk, piece, slab),
a list long enough for the binary search, special values, the production width, the empty list, the exact peel, cache residency and
argument errors."""
import ctypes as C

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.correlate_oracle import FILL, correlate, correlate_chain, reference_rows
from tests.residual_oracle import match_residual, residual, residual_scores, sort_events, subtract_rows_t1
from tests.tmatch_oracle import events_of_scores

pytestmark = pytest.mark.gpu

TAPS9 = np.random.RandomState(1).randn(9)


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

    def residual(self, dev, *args):
        if dev:
            st, out, buf = hip.dev_residual(*self.dev(), *args)
            buf.free()
        else:
            st, out = hip.residual(*self.host(), *args)
        assert st == [0] * len(self.keys)
        return out

    def match(self, dev, *args):
        if dev:
            st, n, res, buf = hip.dev_match_residual(*self.dev(), *args)
            buf.free()
        else:
            st, n, *res = hip.match_residual(*self.host(), *args)
        assert st == [0] * len(self.keys) and n == res[0].size
        return tuple(np.ascontiguousarray(a).tobytes() for a in res)

    def free(self):
        if self.cbuf is not None:
            self.cbuf.free()


def _lists(rs, rows, K, T, before, seams):
    """The event lists of one shape, in sample order: none; one; and one list with ties, five events on one sample, events at sample 0
    and rows - 1, one astride every seam, and random ones."""
    s = [0, 0, rows - 1, rows - 1, rows // 2, rows // 2, rows // 2] + [rows // 3] * 5
    for b in seams:
        s += [min(rows - 1, max(0, b + before - T // 2)), min(rows - 1, max(0, b + before - 1)), min(rows - 1, b + before)]
    s = np.sort(np.concatenate([s, rs.randint(0, rows, 40)])).astype(np.int64)
    full = (s, rs.randint(0, K, s.size).astype(np.int32), (rs.randn(s.size) * 2).astype(np.float32))
    return ((np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)), tuple(v[5:6] for v in full), full)


@pytest.mark.parametrize('n_cols', [1, 4, 5, 17, 64])
def test_columns_template_rows_and_offsets(n_cols):
    """The vector path (4, 64), the scalar path (1, 5, 17) and, through a misaligned output, the scalar path on columns that would
    vectorise; T and before at their ends; int16 and float32 recordings, with and without the median; host and device entries."""
    rs = np.random.RandomState(n_cols)
    rows, chunk = 500, 130
    n_ch = n_cols + 2
    cols = np.arange(n_ch)[::-1][:n_cols].copy()
    case = 0
    for dtype in (np.int16, np.float32):
        x = (rs.randn(rows, n_ch) * 40).astype(dtype)
        ck = Chunks(x, chunk)
        xs = x[:, cols]
        for T in (1, 3, 61, 256):
            k = rs.randn(3, T, n_cols)
            for before in (0, T // 3, T):
                ref = case % 2
                taps = TAPS9 if case % 3 else [1.0]
                case += 1
                for ev in _lists(rs, rows, 3, T, before, (130, 260, 390)):
                    i0, i1 = (0, rows) if case % 2 else (7, rows - 3)
                    want = residual(xs, 0, 0, rows, i0, i1, taps, ref, before, k, *ev)
                    for dev in (False, True):
                        got = ck.residual(dev, 0, rows, i0, i1, taps, cols, ref, before, k, *ev)
                        assert got.dtype == np.float32 and got.shape == want.shape
                        assert got.tobytes() == want.tobytes(), (dtype, T, before, ref, dev, ev[0].size)
        if dtype == np.int16 and n_cols in (4, 64):
            # a device output that is not 16-byte aligned: the same bytes through the scalar path
            k = rs.randn(3, 3, n_cols)
            ev = _lists(rs, rows, 3, 3, 1, (130, 260, 390))[2]
            want = residual(xs, 0, 0, rows, 0, rows, TAPS9, 1, 1, k, *ev)
            head, n, status = hip._dev_chunks(*ck.dev())
            mid, shape, keep = hip._res_args(0, rows, 0, rows, TAPS9, cols, 1, 1, k, *ev)
            out = hip.DevBuffer(want.nbytes + 512)
            hip._check(hip.lib().mts_dev_residual(*head, *mid, out.at(4), status.ctypes.data_as(C.POINTER(C.c_int))), 'mts_dev_residual')
            got = np.empty(shape, np.float32)
            hip._check(hip.lib().mts_dev_copy(0, None, hip._ptr(got), out.at(4), got.nbytes, 1), 'mts_dev_copy')
            out.free()
            assert got.tobytes() == want.tobytes()
        ck.free()


def test_more_events_on_a_tile_than_an_lds_batch():
    rs = np.random.RandomState(2)
    rows = 400
    for n_cols in (4, 5):
        x = (rs.randn(rows, n_cols) * 40).astype(np.int16)
        ck = Chunks(x, 150)
        k = rs.randn(2, 3, n_cols)
        n = 700                                                         # three batches of 256 on the rows 198 .. 212, every row > 100 deep
        ev = (np.sort(rs.randint(200, 210, n)), rs.randint(0, 2, n), (rs.randn(n) * 0.01).astype(np.float32))
        want = residual(x, 0, 0, rows, 0, rows, [1.0], 0, 1, k, *ev)
        assert ck.residual(False, 0, rows, 0, rows, [1.0], np.arange(n_cols), 0, 1, k, *ev).tobytes() == want.tobytes()
        assert ck.residual(True, 0, rows, 190, 220, [1.0], np.arange(n_cols), 0, 1, k, *ev).tobytes() == want[190:220].tobytes()
        ck.free()


def test_a_list_past_two_to_the_sixteen():
    """10^5 events on 4 columns: the binary search ranges over indices past 2^16 and most tiles begin deep in the list."""
    rs = np.random.RandomState(4)
    rows, n = 40000, 100000
    x = (rs.randn(rows, 4) * 40).astype(np.int16)
    ck = Chunks(x, 10000)
    k = rs.randn(5, 1, 4)
    ev = sort_events(rs.randint(0, rows, n), rs.randint(0, 5, n), (rs.randn(n) * 2).astype(np.float32))
    z = reference_rows(x, 0, 0, rows, 0, rows, [1.0], 1)
    want = subtract_rows_t1(z.copy(), 0, 0, rows, *ev, 0, k)
    want[np.isnan(want)] = FILL
    args = (0, rows, 0, rows, [1.0], np.arange(4), 1, 0, k, ev[0], ev[1].astype(np.int32), ev[2])
    assert ck.residual(False, *args).tobytes() == want.tobytes() != z.tobytes()
    assert ck.residual(True, *args).tobytes() == want.tobytes()
    # ... and the scores of that residual: the events of mts_match_residual
    score = correlate_chain(want, k)
    thr = np.float32(np.percentile(score, 99))
    wev = events_of_scores(score, 0, 0, rows, thr, 3)
    margs = (0, rows, 0, rows, [1.0], np.arange(4), 1, 0, k, thr, 3, 1 << 16, ev[0], ev[1].astype(np.int32), ev[2])
    assert wev[0].size > 10
    for dev in (False, True):
        assert ck.match(dev, *margs) == (wev[0].tobytes(), wev[1].astype(np.int32).tobytes(), wev[2].tobytes())
    ck.free()


def test_special_values():
    rs = np.random.RandomState(6)
    rows, nc = 300, 4
    x = (rs.randn(rows, nc) * 10).astype(np.float32)
    x[120, 1] = np.nan
    x[200, 0] = np.inf
    x[40:60] = 0.0
    ck = Chunks(x, 100)
    k = rs.randn(3, 5, nc)
    k[1, 2] = 0.0                                                       # zero entries are not skipped: inf * 0 at row 200 is a NaN
    k[2] = 1e-30
    ev = (np.array([45, 50, 50, 52, 118, 119, 199, 201, 250, 250, 251]), np.array([2, 2, 2, 2, 0, 1, 1, 1, 0, 0, 0]),
          np.array([1e-30, 1e-30, 0.0, -0.0, 1.0, 2.0, 1.0, 0.0, 3e38, -3e38, 3e38], np.float32))
    for ref in (0, 1):
        want = residual(x, 0, 0, rows, 0, rows, [1.0], ref, 2, k, *ev)
        assert np.isnan(want).any() and np.isinf(want).any()
        if not ref:
            assert np.signbit(want[43:55]).any() and (want[43:55] == 0).all()      # +0 - 1e-60 is -0, and stays -0 under the events after it
        for dev in (False, True):
            assert ck.residual(dev, 0, rows, 0, rows, [1.0], np.arange(nc), ref, 2, k, *ev).tobytes() == want.tobytes()
        # an empty list gives z, a NaN as 0x7fc00000
        z = reference_rows(x, 0, 0, rows, 0, rows, [1.0], ref)
        z[np.isnan(z)] = FILL
        assert ck.residual(False, 0, rows, 0, rows, [1.0], np.arange(nc), ref, 2, k, [], [], []).tobytes() == z.tobytes()
        wev = match_residual(x, 0, 0, rows, 0, rows, [1.0], ref, 2, k, -3e38, 2, *ev)
        assert ck.match(False, 0, rows, 0, rows, [1.0], np.arange(nc), ref, 2, k, -3e38, 2, 512, *ev) == (
            wev[0].tobytes(), wev[1].astype(np.int32).tobytes(), wev[2].tobytes())
    ck.free()


def test_widest_templates():
    rs = np.random.RandomState(9)
    rows, W, T = 700, 1024, 256
    x = (rs.randn(rows, W) * 40).astype(np.int16)
    ck = Chunks(x, 400)
    k = rs.randn(2, T, W)
    ev = (np.array([0, 130, 130, 300, 399, 401, 699]), np.array([0, 1, 0, 1, 0, 1, 0]), (rs.randn(7) * 2).astype(np.float32))
    want = residual(x, 0, 0, rows, 0, rows, [1.0], 1, 85, k, *ev)
    for dev in (False, True):
        assert ck.residual(dev, 0, rows, 0, rows, [1.0], np.arange(W), 1, 85, k, *ev).tobytes() == want.tobytes()
    ck.free()


def test_empty_list_is_match_templates_byte_for_byte():
    rs = np.random.RandomState(3)
    x = synth_int16(0, 900, 7, 3)
    ck = Chunks(x, 300)
    k = rs.randn(4, 9, 7)
    thr = np.percentile(correlate(x, 0, 0, 900, 0, 900, TAPS9, 1, 4, k), 90, axis=0).astype(np.float32)
    args = (0, 900, 5, 880, TAPS9, np.arange(7), 1, 4, k, thr, 6, 1024)
    st, n, row, tpl, val = hip.match_templates(*ck.host(), *args)
    assert n == row.size > 3
    for dev in (False, True):
        assert ck.match(dev, *args, [], [], []) == (row.tobytes(), tpl.tobytes(), val.tobytes())
    # a short buffer with a list: the full count, the first max_events events
    ev = (np.array([100, 400, 400]), np.array([0, 1, 2]), np.array([5.0, -3.0, 2.0], np.float32))
    want = match_residual(x, 0, 0, 900, 5, 880, TAPS9, 1, 4, k, thr, 6, *ev)
    st, n, row, tpl, val = hip.match_residual(*ck.host(), *args[:-1], 3, *ev)
    assert n == want[0].size > 3 and (row.tobytes(), tpl.tobytes(), val.tobytes()) == (want[0][:3].tobytes(), want[1][:3].astype(np.int32).tobytes(),
                                                                                     want[2][:3].tobytes())
    ck.free()


def _make(tmp, x, rate, **kw):
    raw = tmp / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'd.cbin', tmp / 'd.ch', sample_rate=float(rate), n_channels=x.shape[1], dtype=x.dtype,
                         check_after_compress=False, do_time_diff=x.dtype.kind != 'f')
    return mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', check_after_decompress=False, **kw)


def test_seams_lanes_and_residency(tmp_cfg, monkeypatch):
    """An event astride every chunk, piece and slab seam; one lane and two; calls of one chunk; resident chunks read in place."""
    x = synth_int16(0, 3000, 20, 4)
    one = _make(tmp_cfg, x, 500, codec=api.HipCodec(devices=[0]))        # six chunks of 20 000 bytes
    two = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, codec=api.HipCodec(devices=[0, 0]))
    rs = np.random.RandomState(5)
    k = rs.randn(6, 61, 20)
    taps = api.highpass_taps(300, 5000, 65)
    s = np.concatenate([np.arange(480, 2600, 500), np.arange(500, 2600, 500), np.arange(520, 2600, 500), [0, 2999], rs.randint(0, 3000, 300)])
    ev = (s, rs.randint(0, 6, s.size), (rs.randn(s.size) * 3).astype(np.float32))     # ~6 events over every row
    kw = dict(before=20, taps=taps, reference='median')
    want = residual(x, 0, 0, 3000, 0, 3000, taps, 1, 20, k, *ev)
    thr = np.float32(np.percentile(residual_scores(x, 0, 0, 3000, 0, 3000, taps, 1, 20, k, *ev), 95))
    wev = tuple(v.tobytes() for v in match_residual(x, 0, 0, 3000, 0, 3000, taps, 1, 20, k, thr, 30, *ev))
    assert len(wev[0]) >= 8 * 10

    def check(r, a=0, b=3000):
        assert r.residual(*ev, k, a, b, **kw).tobytes() == want[a:b].tobytes()

    def events(r, *rng):
        got = r.match_templates(k, thr, *rng, exclude=30, subtract=ev, **kw)
        return got.sample.tobytes(), got.template.tobytes(), got.score.tobytes()
    check(one)
    check(two)
    check(one, 1777, 2999)
    assert events(one) == wev and events(two) == wev
    assert tuple(p + q for p, q in zip(events(one, 0, 1777), events(one, 1777, 3000))) == wev
    monkeypatch.setattr(api, 'RESIDUAL_CALL_BYTES', 1)                   # a call per chunk
    monkeypatch.setattr(api, 'TMATCH_CALL_BYTES', 1)
    check(one)
    assert events(one) == wev
    monkeypatch.setattr(api, 'RESIDUAL_CALL_BYTES', 1 << 30)
    monkeypatch.setattr(api, 'TMATCH_CALL_BYTES', 1 << 30)
    # pieces of one chunk, slabs of a few rows (both are read from the environment by every call)
    monkeypatch.setenv('MTS_PIPE_BYTES', str(20000))
    monkeypatch.setenv('MTS_RESIDUAL_SLAB_BYTES', str(7 * 80))
    monkeypatch.setenv('MTS_TMATCH_SLAB_BYTES', str(200 * 80))
    check(one)
    assert events(one) == wev
    monkeypatch.setenv('MTS_RESIDUAL_SLAB_BYTES', '1')                   # a slab per row
    monkeypatch.setenv('MTS_TMATCH_SLAB_BYTES', '1')
    check(one, 1930, 2070)
    sel = (np.frombuffer(wev[0], np.int64) >= 1930) & (np.frombuffer(wev[0], np.int64) < 2070)
    assert events(one, 1930, 2070) == tuple(np.frombuffer(w, t)[sel].tobytes() for w, t in zip(wev, (np.int64, np.int64, np.float32)))
    for name in ('MTS_PIPE_BYTES', 'MTS_RESIDUAL_SLAB_BYTES', 'MTS_TMATCH_SLAB_BYTES'):
        monkeypatch.delenv(name)
    # resident == cold, and neither call inserts anything
    keys = list(range(one.n_chunks))
    one[:]
    for c in range(one.n_chunks):
        one[one.chunk_bounds[c]:one.chunk_bounds[c] + 1]
    cache = one._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 20 for b in before) >= len(keys) // 2
    check(one)
    assert events(one) == wev
    assert hip.cache_query(cache, keys).tolist() == before
    one.close()
    two.close()


def test_exact_peel_on_the_device(tmp_cfg):
    k = np.zeros((2, 7, 4))
    k[0, :, 0] = k[0, :, 1] = [1, 3, 6, 9, 6, 3, 1]                     # |K0|^2 = 346
    k[1, :, 2] = k[1, :, 3] = [1, 2, 4, 6, 4, 2, 1]                     # |K1|^2 = 156
    t0 = 997
    x = np.zeros((3000, 4), np.int16)
    x[t0 - 3:t0 + 4] += k[0].astype(np.int16)
    x[t0 + 2:t0 + 9] += k[1].astype(np.int16)
    r = _make(tmp_cfg, x, 1000)
    ev = r.match_templates(k, 78.0, before=3)
    assert (ev.sample.tolist(), ev.template.tolist(), ev.score.tolist(), ev.exclude) == ([t0], [0], [346.0], 6)
    amp = api.template_amplitudes(ev.score, ev.template, k)
    assert amp.tolist() == [1.0]
    ev2 = r.match_templates(k, 78.0, before=3, subtract=(ev.sample, ev.template, amp))
    assert (ev2.sample.tolist(), ev2.template.tolist(), ev2.score.tolist()) == ([t0 + 5], [1], [156.0])
    both = (np.concatenate([ev2.sample, ev.sample]), np.concatenate([ev2.template, ev.template]),
            np.concatenate([api.template_amplitudes(ev2.score, ev2.template, k), amp]))
    assert r.residual(*both, k, before=3).tobytes() == bytes(4 * 4 * 3000)         # +0 everywhere
    assert r.match_templates(k, 78.0, before=3, subtract=both).sample.size == 0
    r.close()


def test_argument_errors_name_the_entry():
    x = (np.arange(400, dtype=np.int16).reshape(100, 4) * 37 % 101).astype(np.int16)
    ck = Chunks(x, 100)
    L = hip.lib()
    k = np.ones((2, 3, 2), np.float32)
    ip = C.POINTER(C.c_int)
    d_out = hip.DevBuffer(1 << 16)

    def call(dev, match, s=(10, 20), t=(0, 1), a=(1.0, 2.0), n_sub=None, null=False):
        ev = (np.asarray(s, np.int64), np.asarray(t, np.int32), np.asarray(a, np.float32))
        head, n, status = hip._dev_chunks(*ck.dev()) if dev else hip._host_chunks(0, *ck.host())
        status[:] = 99
        if match:
            mid, cap, n_ev, keep = hip._tm_args(0, 100, 10, 90, [1.0, 0.5], [0, 1], 0, 1, k, -3e38, 0, 8)
        else:
            mid, shape, keep = hip._cor_args(0, 100, 10, 90, [1.0, 0.5], [0, 1], 0, 1, k)
        sub, keep_sub = hip._sub_args(*ev)
        sub = (sub[0] if n_sub is None else n_sub,) + ((None,) * 3 if null else sub[1:])
        out = np.full(80 * 2, -5, np.float32)
        res = (np.full(8, -5, np.int64), np.full(8, -5, np.int32), np.full(8, -5, np.float32))
        n_ev = np.full(1, -7, np.int64)
        if match:
            outs = [d_out.at(0), d_out.at(4096), d_out.at(8192)] if dev else [hip._ptr(v) for v in res]
            rc = getattr(L, 'mts_dev_match_residual' if dev else 'mts_match_residual')(*head, *mid, *sub, *outs, hip._lp(n_ev), status.ctypes.data_as(ip))
        else:
            rc = getattr(L, 'mts_dev_residual' if dev else 'mts_residual')(*head, *mid, *sub, d_out.at(0) if dev else hip._ptr(out),
                                                                          status.ctypes.data_as(ip))
        untouched = int(status[0]) == 99 and (out == -5).all() and all((v == -5).all() for v in res) and int(n_ev[0]) == -7
        return rc, untouched, L.mts_last_error().decode()
    for dev in (False, True):
        for match in (False, True):
            assert call(dev, match)[0] == 0
            assert call(dev, match, s=(), t=(), a=())[0] == 0 and call(dev, match, s=(), t=(), a=(), null=True)[0] == 0
            assert call(dev, match, s=(0, 99), a=(0.0, -3e38))[0] == 0
            for bad, word in ((dict(s=(20, 10)), 'event 1'), (dict(s=(10, 20, 15), t=(0, 0, 0), a=(1, 1, 1)), 'event 2'),
                              (dict(s=(-1, 20)), 'event 0'), (dict(s=(10, 100)), 'event 1'), (dict(t=(0, 2)), 'event 1'),
                              (dict(t=(-1, 0)), 'event 0'), (dict(a=(1.0, np.nan)), 'event 1'), (dict(a=(np.inf, 1.0)), 'event 0'),
                              (dict(n_sub=(1 << 30) + 1), 'events'), (dict(n_sub=-1), 'events'), (dict(null=True), 'events')):
                rc, untouched, msg = call(dev, match, **bad)
                assert rc == -1 and untouched and word in msg, (dev, match, bad, msg)       # MTS_E_ARG before anything ran
    d_out.free()
    ck.free()
