"""Reader.match_templates and mts_match_templates / mts_dev_match_templates on the MI355X: the kernels against the numpy restatement
of the definition (tests/tmatch_oracle.py) over the oracle's decode, for exact equality of every byte: templates across lanes and
waves, exclusion radii and bitmap words, plateaus, special values, dense events and the short buffer, the top of the file,
bit-identity across the cache, lanes, calls, slabs, pieces and the two entry points, cross-checks against correlate and detect,
argument errors and a damaged chunk."""
import ctypes as C

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.correlate_oracle import correlate
from tests.tmatch_oracle import events_of_scores, match_templates
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


def _scores(dec, k, before, channels=slice(None), taps=None, reference=None):
    """The oracle's scores of the whole file: computed once per case and shared by its checks."""
    cols = np.arange(dec.shape[1])[channels] if isinstance(channels, slice) else np.asarray(channels)
    return correlate(dec[:, cols], 0, 0, dec.shape[0], 0, dec.shape[0], [1.0] if taps is None else taps, 1 if reference else 0, before, k)


def _p90(score):
    return np.percentile(score, 90, axis=0).astype(np.float32)


def _bytes(ev):
    return tuple(np.ascontiguousarray(a).tobytes() for a in ev)


def _check(r, score, k, thr, i0, i1, before, R, channels=slice(None), taps=None, reference=None):
    """Reader.match_templates on rows [i0, i1) against the definition over the whole file's scores.  -> the oracle's events."""
    got = r.match_templates(k, thr, i0, i1, channels=channels, before=before, taps=taps, reference=reference, exclude=R)
    want = events_of_scores(score, 0, i0, i1, thr, R)
    assert (got.sample.dtype, got.template.dtype, got.score.dtype) == (np.int64, np.int64, np.float32)
    assert (got.start, got.stop, got.exclude) == (i0, i1, R)
    assert _bytes((got.sample, got.template, got.score)) == _bytes(want), (got.sample[:8], want[0][:8], got.template[:8], want[1][:8])
    return want


TAPS65 = api.highpass_taps(300, 5000, 65)
TAPS9 = np.random.RandomState(1).randn(9)


@pytest.mark.parametrize('n_out', [1, 2, 63, 64, 65, 130])
def test_templates_across_lanes_and_waves(tmp_cfg, n_out):
    x = synth_int16(0, 300, 6, 5)
    r, dec = _make(tmp_cfg, x, 100)                                     # three chunks of 100 rows
    k = np.random.RandomState(n_out).randn(n_out, 7, 6)
    k[n_out - 1] = k[0]                                                 # identical templates: the lower index wins everywhere
    if n_out >= 5:
        k[3] = k[1]
    score = _scores(dec, k, 3, taps=TAPS9)
    thr = _p90(score)
    n0 = 0
    for R in (0, 2):
        row, tpl, _ = _check(r, score, k, thr, 0, 300, 3, R, taps=TAPS9)
        assert row.size > 0 and (R == 0 or row.size < n0)
        assert n_out == 1 or n_out - 1 not in tpl
        assert n_out < 5 or 3 not in tpl
        n0 = row.size
    r.close()


@pytest.mark.parametrize('R', [0, 1, 2, 63, 64, 255])
def test_exclusion_radii_and_bitmap_words(tmp_cfg, R):
    x = synth_int16(0, 700, 5, 2)
    r, dec = _make(tmp_cfg, x, 100)                                     # seven chunks
    assert r.n_chunks == 7
    k = np.random.RandomState(9).randn(5, 7, 5)
    score = _scores(dec, k, 3, taps=TAPS9, reference='median')
    thr = _p90(score)
    n0 = events_of_scores(score, 0, 0, 700, thr, 0)[0].size
    n = _check(r, score, k, thr, 0, 700, 3, R, taps=TAPS9, reference='median')[0].size
    assert n > 0 and (R == 0 or n < n0)
    for i0, i1 in ((70, 201), (0, 1), (699, 700), (1, 66), (630, 700), (1, 64), (1, 65), (64, 193)):     # stitching, starts off a word
        _check(r, score, k, thr, i0, i1, 3, R, taps=TAPS9, reference='median')
    r.close()


def test_plateaus(tmp_cfg):
    ones = np.ones((1, 5, 3))
    ramp = np.repeat(np.arange(300, dtype=np.int16)[:, None], 3, axis=1)
    for x, thr, first in ((np.full((300, 3), 7, np.int16), 1.0, 2), (np.zeros((300, 3), np.int16), -1.0, 0), (ramp, 1.0, None),
                          (ramp[::-1].copy(), 1.0, None)):
        r, dec = _make(tmp_cfg, x, 100)
        score = _scores(dec, ones, 2)
        for R in (1, 4, 255):
            row, tpl, _ = _check(r, score, ones, thr, 0, 300, 2, R)
            assert row.size >= 1
            if first is not None:                                       # one event: the plateau's first row
                assert row.tolist() == [first] and tpl.tolist() == [0]
            _check(r, score, ones, thr, 0, 150, 2, R)                   # in two halves
            _check(r, score, ones, thr, 150, 300, 2, R)
        r.close()


def test_special_values(tmp_cfg):
    rows, nc = 300, 4
    rs = np.random.RandomState(1)
    x = (rs.randn(rows, nc) * 10).astype(np.float32)
    x[120, 1] = np.nan                                                  # poisons the scores of rows 118 .. 122 (T = 5, before = 2)
    x[200, 0] = np.inf
    r, dec = _make(tmp_cfg, x, 100)
    k = np.abs(rs.randn(3, 5, nc)) + 0.5                                # all positive: inf gives +inf, never inf - inf
    score = _scores(dec, k, 2)
    assert np.isnan(score[118:123]).all() and not np.isnan(score[:118]).any() and np.isposinf(score[198:203]).all()
    for R in (0, 1, 4, 20):
        row, tpl, val = _check(r, score, k, -3e38, 0, rows, 2, R)
        assert not np.isin(row, np.arange(118, 123)).any()              # a NaN score is no event ...
        near = row[(row >= 118 - max(R, 1) - 2) & (row <= 122 + max(R, 1) + 2)]
        assert near.size > 0                                            # ... and beats nothing: its neighbours have theirs
        inf = row[np.isposinf(val)]
        assert inf.tolist() == (list(range(198, 203)) if R == 0 else [198])        # a +inf score is an event; of equal ones the earlier
        assert tpl[row == 198].tolist() == [0]                          # ... (row, template) wins
    r.close()
    # -0 against +0: products that underflow give -0 scores beside +0 ones -- one plateau
    x = np.zeros((300, nc), np.float32)
    x[rs.rand(300) < 0.8] = -1e-30
    r, dec = _make(tmp_cfg, x, 100)
    k = np.full((3, 5, nc), 1e-30)
    score = _scores(dec, k, 2)
    assert (score == 0).all() and np.signbit(score).any() and not np.signbit(score).all()
    row, tpl, _ = _check(r, score, k, -1.0, 0, rows, 2, 0)
    assert row.tolist() == list(range(rows)) and not tpl.any()
    for R in (1, 7):
        row, tpl, _ = _check(r, score, k, -1.0, 0, rows, 2, R)
        assert row.tolist() == [0] and tpl.tolist() == [0]
        assert _check(r, score, k, 0.0, 0, rows, 2, R)[0].size == 0
    r.close()


def test_dense_events_go_through_the_second_call(tmp_cfg, monkeypatch):
    x = synth_int16(0, 300, 6, 5)
    r, dec = _make(tmp_cfg, x, 100)
    k = np.random.RandomState(3).randn(5, 7, 6)
    score = _scores(dec, k, 3, taps=TAPS9)
    monkeypatch.setattr(api, 'TMATCH_GUESS_MIN', 16)
    calls = []
    real = r.codec.match_templates
    monkeypatch.setattr(r.codec, 'match_templates', lambda *a, **kw: calls.append(a[-1]) or real(*a, **kw), raising=False)
    row, _, _ = _check(r, score, k, -3e38, 0, 300, 3, 0, taps=TAPS9)
    assert row.tolist() == list(range(300)) and calls == [16, 300]      # the guess, then room for all
    r.close()


def test_top_of_file(tmp_cfg):
    x = synth_int16(0, 300, 6, 5)
    r, dec = _make(tmp_cfg, x, 100)
    k = np.random.RandomState(3).randn(2, 7, 6)
    # before = T: row 0 reads nothing of the recording and scores +0 -- a call without chunks
    top = r.match_templates(k, -1.0, 0, 1, before=7, exclude=0)
    assert (top.sample.tolist(), top.template.tolist(), top.score.tobytes()) == ([0], [0], np.zeros(1, np.float32).tobytes())
    assert r.match_templates(k, 1.0, 0, 1, before=7, exclude=0).sample.size == 0
    score = _scores(dec, k, 7)
    for R in (0, 3):
        _check(r, score, k, -1.0, 0, 1, 7, R)                           # (with R = 3 the rows 1 .. 3 are read, and may beat it)
        _check(r, score, k, 1.0, 0, 1, 7, R)
        _check(r, score, k, _p90(score), 0, 300, 7, R)
    st, n, row, tpl, val = hip.match_templates(0, [], [], b'', [], [], [], 6, np.int16, r._flags(), 0, 300, 0, 1, [1.0], np.arange(6), 0, 7, k,
                                               -1.0, 0, 4)
    assert (st, n, row.tolist(), tpl.tolist(), val.tobytes()) == ([], 1, [0], [0], np.zeros(1, np.float32).tobytes())
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
    k[9] = k[0]
    score = _scores(dec, k, 20, taps=TAPS65, reference='median')
    thr = _p90(score)
    kw = dict(before=20, taps=TAPS65, reference='median', exclude=30)
    want = _bytes(_check(one, score, k, thr, 0, 3000, 20, 30, taps=TAPS65, reference='median'))     # cold, one lane, one call, one slab
    assert len(want[0]) >= 8 * 10

    def ev(r, *rng):
        got = r.match_templates(k, thr, *rng, **kw)
        return _bytes((got.sample, got.template, got.score))

    def part(a, c):
        sel = (np.frombuffer(want[0], np.int64) >= a) & (np.frombuffer(want[0], np.int64) < c)
        return _bytes(np.frombuffer(w, t)[sel] for w, t in zip(want, (np.int64, np.int64, np.float32)))
    assert ev(one) == want                                              # the same call twice
    assert ev(two) == want                                              # one lane == two
    for a, b, c in ((0, 1500, 3000), (0, 1, 3000), (0, 1777, 2999)):    # the whole range == two halves
        assert tuple(p + q for p, q in zip(ev(one, a, b), ev(one, b, c))) == part(a, c)
    monkeypatch.setattr(api, 'TMATCH_CALL_BYTES', 1)                    # a call per chunk
    assert ev(one) == want
    monkeypatch.setattr(api, 'TMATCH_CALL_BYTES', 1 << 30)
    # slabs and pieces (both are read from the environment by every call): 720 rows of 80 bytes hold 600 owned rows, 30 either side
    # and their 60 neighbours -- five slabs of the one piece; with pieces of one chunk, every piece its own slabs; a bound of one
    # byte: a slab per row
    monkeypatch.setenv('MTS_TMATCH_SLAB_BYTES', str(720 * 80))
    assert ev(one) == want
    monkeypatch.setenv('MTS_PIPE_BYTES', str(20000))
    assert ev(one) == want
    monkeypatch.setenv('MTS_TMATCH_SLAB_BYTES', str(200 * 80))
    assert ev(one) == want
    monkeypatch.setenv('MTS_TMATCH_SLAB_BYTES', '1')
    assert ev(one, 1930, 2070) == part(1930, 2070)
    monkeypatch.delenv('MTS_TMATCH_SLAB_BYTES')
    monkeypatch.delenv('MTS_PIPE_BYTES')
    # resident == cold, and a scan inserts nothing
    keys = list(range(one.n_chunks))
    one[:]
    for c in range(one.n_chunks):
        one[one.chunk_bounds[c]:one.chunk_bounds[c] + 1]
    cache = one._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 20 for b in before) >= len(keys) // 2
    assert ev(one) == want
    assert hip.cache_query(cache, keys).tolist() == before
    # mts_match_templates == mts_dev_match_templates, on the file's chunks in host and in device memory
    data = (tmp_cfg / 'd.cbin').read_bytes()
    offs, bounds = np.asarray(one.chunk_offsets, np.int64), np.asarray(one.chunk_bounds, np.int64)
    args = (20, np.int16, one._flags(), 0, 3000, 40, 2950, TAPS65, np.arange(20), 1, 20, k, thr, 30, 4096)
    st, n, row, tpl, val = hip.match_templates(0, keys, bounds[:-1], data, offs[:-1], np.diff(offs), np.diff(bounds), *args)
    assert st == [0] * one.n_chunks and n == row.size and _bytes((row, tpl.astype(np.int64), val)) == part(40, 2950)
    cbuf = _upload(data)
    st, n_dev, res, out = hip.dev_match_templates(cbuf, offs[:-1], np.diff(offs), bounds[:-1], np.diff(bounds), *args)
    assert st == [0] * one.n_chunks and n_dev == n and _bytes(res) == _bytes((row, tpl, val))
    out.free()
    cbuf.free()
    one.close()
    two.close()


def test_cross_checks_against_correlate_and_detect(tmp_cfg):
    x = synth_int16(0, 1500, 24, 4)
    r, dec = _make(tmp_cfg, x, 500)
    k = np.random.RandomState(6).randn(7, 9, 24)
    kw = dict(before=4, taps=TAPS65, reference='median')
    score = r.correlate(k, **kw)                                        # the device's own scores
    thr = _p90(score)
    for (i0, i1), R in (((0, 1500), 8), ((7, 1400), 0), ((490, 1011), 40)):
        ev = r.match_templates(k, thr, i0, i1, exclude=R, **kw)
        assert ev.sample.size > 0
        assert ev.score.tobytes() == np.ascontiguousarray(r.correlate(k, i0, i1, **kw)[ev.sample - i0, ev.template]).tobytes()
        assert _bytes((ev.sample, ev.template, ev.score)) == _bytes(events_of_scores(score, 0, i0, i1, thr, R))   # numpy's peak pick
    # template j is 1 at (before, j): the events are detect's, with every column a neighbour
    hot = np.zeros((24, 5, 24))
    hot[np.arange(24), 2, np.arange(24)] = 1.0
    for reference in (None, 'median'):
        for R in (0, 7):
            det = r.detect(12.0, taps=TAPS65, sign='pos', reference=reference, exclude=R, spread=32)
            ev = r.match_templates(hot, 12.0, before=2, taps=TAPS65, reference=reference, exclude=R)
            assert det.sample.size >= 20
            assert np.array_equal(ev.sample, det.sample) and np.array_equal(ev.template, det.channel) and np.array_equal(ev.score, det.amplitude)
    r.close()


def test_production_width(tmp_cfg):
    x = synth_int16(0, 200, 385, 3)
    r, dec = _make(tmp_cfg, x, 100)
    k = np.random.RandomState(0).randn(3, 61, 385)
    score = _scores(dec, k, 20, taps=TAPS9, reference='median')
    thr = _p90(score)
    n0 = _check(r, score, k, thr, 0, 200, 20, 0, taps=TAPS9, reference='median')[0].size
    n = _check(r, score, k, thr, 0, 200, 20, 60, taps=TAPS9, reference='median')[0].size
    assert 0 < n < n0
    r.close()


@pytest.mark.parametrize('dtype', ['uint16', 'float64'])
def test_item_types(tmp_cfg, dtype):
    rows, nc = 400, 7
    rs = np.random.RandomState(3)
    x = (rs.randn(rows, nc) * 100).astype(dtype) if dtype == 'float64' else rs.randint(0, 65536, size=(rows, nc)).astype(dtype)
    r, dec = _make(tmp_cfg, x, 100)
    k = rs.randn(3, 5, nc)
    score = _scores(dec, k, 2, taps=TAPS9, reference='median')
    thr = _p90(score)
    n0 = _check(r, score, k, thr, 0, rows, 2, 0, taps=TAPS9, reference='median')[0].size
    n = _check(r, score, k, thr, 3, rows - 2, 2, 4, taps=TAPS9, reference='median')[0].size
    assert 0 < n < n0
    r.close()


def test_c_abi_short_buffer_and_argument_errors():
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = (np.arange(400, dtype=np.int16).reshape(100, nc) * 37 % 101).astype(np.int16)
    z = hip.compress_chunks(x, [0, 100], hip.make_flags(), 6)[0]
    data = np.frombuffer(z + b'\0' * 16, dtype=np.uint8)
    cbuf = _upload(z)
    d_out = hip.DevBuffer(1 << 16)
    keep = []

    def call(dev=False, row0=0, rows=100, taps=(1.0, 0.5), vb=0, ve=100, rb=10, re=90, cols=(0, 1), ref=0, before=1, T=3, K=2, tpl=None,
             itemsize=2, flags=hip.make_flags(), outs=True, templates=True, thr=(-3e38, -3e38), R=0, cap=10, n_ev=True):
        a = [np.array(v, dtype=np.int64) for v in ([0], [row0], [0], [len(z)], [rows])]
        c, t = np.array(cols, dtype=np.int32), np.array(taps, dtype=np.float64)
        k = np.ones((max(K, 1), max(T, 1), max(len(c), 1)), np.float32) if tpl is None else np.asarray(tpl, np.float32)
        th = None if thr is None else np.array(thr, dtype=np.float32)
        o = (np.full(64, -5, np.int64), np.full(64, -5, np.int32), np.full(64, -5, np.float32))
        n = np.full(1, -7, np.int64)
        st = np.full(1, 99, np.int32)
        keep.append((a, c, t, k, th, o, n, st))
        lp = [v.ctypes.data_as(C.POINTER(C.c_long)) for v in a]
        mid = (vb, ve, rb, re, len(t), t.ctypes.data_as(C.POINTER(C.c_double)), len(c), c.ctypes.data_as(C.POINTER(C.c_int)), ref, before, T, K,
               k.ctypes.data_as(C.POINTER(C.c_float)) if templates else None, None if th is None else th.ctypes.data_as(C.POINTER(C.c_float)),
               R, cap)
        stp, np_ = st.ctypes.data_as(C.POINTER(C.c_int)), n.ctypes.data_as(C.POINTER(C.c_long)) if n_ev else None
        if dev:
            outs_ = [d_out.at(0), d_out.at(4096), d_out.at(8192)] if outs else [None] * 3
            rc = L.mts_dev_match_templates(0, None, cbuf.at(), lp[2], lp[3], lp[1], lp[4], 1, nc, itemsize, flags, *mid, *outs_, np_, stp)
        else:
            outs_ = [hip._ptr(v) for v in o] if outs else [None] * 3
            rc = L.mts_match_templates(0, 0, 1, lp[0], lp[1], data.ctypes.data_as(C.c_void_p), lp[2], lp[3], lp[4], nc, itemsize, flags, *mid,
                                       *outs_, np_, stp)
        return rc, int(st[0]), int(n[0]), o
    want = match_templates(x[:, :2], 0, 0, 100, 10, 90, [1.0, 0.5], 0, 1, np.ones((2, 3, 2), np.float32), -3e38, 0)
    assert want[0].tolist() == list(range(10, 90))
    want255 = match_templates(x[:, :2], 0, 0, 100, 10, 90, [1.0, 0.5], 0, 1, np.ones((2, 3, 2), np.float32), -3e38, 255)[0].size
    for dev in (False, True):
        # max_events 10 against 80 events: the full count, ten entries, the sentinel behind them intact
        rc, st, n, o = call(dev=dev)
        assert (rc, st, n) == (0, 0, 80)
        if not dev:
            assert _bytes(v[:10] for v in o) == _bytes((want[0][:10], want[1][:10].astype(np.int32), want[2][:10]))
            assert all((v[10:] == -5).all() for v in o)
        assert call(dev=dev, cap=0, outs=False)[:3] == (0, 0, 80)       # max_events 0: a count, the outputs may be null
        assert call(dev=dev, rb=40, re=40)[:3] == (0, 0, 0)             # no rows: MTS_OK, no events
        assert call(dev=dev, before=0, T=1)[:2] == (0, 0) and call(dev=dev, before=256, T=256)[:2] == (0, 0)
        assert call(dev=dev, R=255, cap=64)[:3] == (0, 0, want255)
        others = (dict(outs=False), dict(taps=(np.inf, 1.0)), dict(cols=(0, 4)), dict(cols=(-1,)), dict(row0=10),
                  dict(rows=50), dict(rb=-1), dict(re=101), dict(rb=50, re=40), dict(itemsize=3), dict(flags=hip.FLAG_FLOAT, itemsize=2),
                  dict(thr=None), dict(thr=(1.0, np.nan)), dict(thr=(np.inf, 1.0)), dict(R=-1), dict(R=256), dict(cap=-1), dict(n_ev=False))
        # (a shared argument, one bad at a time: the text is the one the library gave before the five ops shared their checks)
        for bad, text in [(b, None) for b in others] + filter_errors('match_templates') + template_errors('match_templates'):
            rc, st, n, o = call(dev=dev, **bad)
            assert rc == -1, bad                                       # MTS_E_ARG ...
            assert st == 99 and n == -7 and all((v == -5).all() for v in o), bad      # ... before anything ran
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
    st = hip.match_templates(0, list(range(5)), bounds[:-1], bytes(data), offs[:-1], np.diff(offs), np.diff(bounds), 8, np.int16, flags, 0, 2500,
                             0, 2500, TAPS65, np.arange(8), 1, 20, k, 1e9, 10, 16)[0]
    assert st[2] != hip.CHUNK_OK and [s for i, s in enumerate(st) if i != 2] == [hip.CHUNK_OK] * 4
    r = _open(tmp_cfg)
    kw = dict(before=20, taps=TAPS65, reference='median', exclude=10)
    with pytest.raises(IOError, match='#2'):
        r.match_templates(k, 1e9, 0, b[2] - 81, **kw)                   # rows of chunks 0 and 1 only; row + 10 + 40 + 32 reaches chunk 2
    with pytest.raises(IOError, match='#2'):
        r.match_templates(k, 1e9, b[3] + 61, b[4], **kw)                # ... and from above: row - 10 - 20 + 32 - 64
    r.match_templates(k, 1e9, 0, b[2] - 82, **kw)
    r.match_templates(k, 1e9, b[3] + 62, b[4], **kw)
    r.close()
