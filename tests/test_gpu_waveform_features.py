"""mts_waveform_features / mts_dev_waveform_features and the Reader on top of them on the MI355X: k_waveform_features against the
numpy restatement of the definition (tests/features_oracle.py), for equality of every byte: lane, workgroup and event-batch seams of
the flat (event, position) index, component blocks and their remainders, basis images up to the LDS limit, clipping at every edge,
special values, every seam of the host side (chunks, pieces, slabs, gaps, residency), the chain on mts_dev_waveforms' own snippets,
the Reader, argument errors."""
import ctypes as C

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.features_oracle import chain, features

pytestmark = pytest.mark.gpu

TAPS9 = np.random.RandomState(1).randn(9)
TAPS65 = api.highpass_taps(300, 5000, 65)
PB = 8                                                                 # FEAT_PB (csrc/common.h): components of a register block
GROUP = 256                                                            # FEAT_THREADS (csrc/features.hip): pairs, and at most events, of a workgroup


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

    def feat(self, dev, *args):
        """The features of mts_dev_waveform_features / mts_waveform_features for the op's own arguments."""
        if dev:
            st, res, buf = hip.dev_waveform_features(*self.dev(), *args)
            buf.free()
        else:
            st, res = hip.waveform_features(*self.host(), *args)
        assert st == [0] * len(self.keys)
        return res

    def waveforms(self, *args):
        st, res, buf = hip.dev_waveforms(*self.dev(), *args)
        buf.free()
        assert st == [0] * len(self.keys)
        return res[0]

    def free(self):
        if self.cbuf is not None:
            self.cbuf.free()


def _same(got, want, what=None):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())


def _both(ck, args, want, what=None):
    for dev in (False, True):
        _same(ck.feat(dev, *args), want, (what, dev))


def _basis(rs, P, T):
    b = rs.standard_normal((P, T)).astype(np.float32)
    b[rs.rand(P, T) < 0.1] = 0.0                                       # zero entries are not skipped
    return b


def _events(rs, rows, n_cols, width, n, before, after):
    """n events by ascending row: a few at both ends of the recording (clipped: NaN throughout), repeats, the rest inside; first
    positions from left of the columns to right of them."""
    fixed = [0, before - 1 if before else 0, rows - 1, rows // 2, rows // 2][:min(n, 5)]
    row = np.sort(np.concatenate((fixed, rs.randint(before, rows - after + 1, n - len(fixed))))).astype(np.int64)
    col0 = rs.randint(-width, n_cols + 1, n)
    col0[:4] = [0, -width + 1, n_cols - 1, max(0, n_cols - width)][:min(n, 4)]
    return row, col0.astype(np.int64)


def _counts(W):
    """Event counts of one slab that put the last workgroup of the flat index at one pair and at a full one, and the event-batch
    seams: a workgroup stages the events of its GROUP pairs, GROUP of them when W is 1."""
    ns = {next(n for n in range(1, 400) if n * W % GROUP == 0)}
    ns |= {n for n in range(1, 300) if n * W % GROUP == 1 and n * W > GROUP}
    if W == 1:
        ns |= {GROUP - 1, GROUP, GROUP + 1}
    return sorted(ns)


def test_counts_reach_the_seams():
    assert _counts(1) == [255, 256, 257] and _counts(17) == [241, 256] and _counts(5) == [205, 256] and _counts(16) == [16]
    assert _counts(33) == [225, 256] and _counts(64) == [4] and _counts(65) == [193, 256] and _counts(70) == [128]


@pytest.mark.parametrize('W', [1, 5, 16, 17, 33, 64, 65, 70])
def test_lane_and_workgroup_seams_of_the_flat_index(W):
    rs = np.random.RandomState(W)
    rows, nc, T, P = 1500, 70, 5, 3
    case = W
    for dtype in (np.int16, np.float32):
        x = synth_int16(0, rows, nc, W) if dtype == np.int16 else (rs.randn(rows, nc) * 300).astype(np.float32)
        ck = Chunks(x, 600)
        for n in _counts(W):
            row, col0 = _events(rs, rows, nc, W, n, 2, 3)
            if W == nc:
                col0[::2] = 0
            ref, taps = case % 2, (TAPS9 if case % 3 else [1.0])
            case += 1
            args = (0, rows, taps, np.arange(nc), ref, row, col0, 2, 3, W, _basis(rs, P, T))
            want = features(x, 0, *args[:3], *args[4:])
            nan = np.isnan(want)
            assert nan.any() and not nan.all()
            _both(ck, args, want, (dtype, n, ref))
            assert hip.waveforms_last_plan(0)['slabs'] == 1              # the flat index runs over the events of a slab: all of them
        ck.free()


@pytest.mark.parametrize('P', [1, 2, 3, 4, 5, 6, PB - 1, PB, PB + 1, 2 * PB, 2 * PB + 5, 32])
def test_component_blocks_and_their_remainders(P):
    rs = np.random.RandomState(100 + P)
    rows, nc, T, W = 1200, 12, 7, 5
    x = synth_int16(0, rows, nc, P)
    ck = Chunks(x, 500)
    row, col0 = _events(rs, rows, nc, W, 70, 3, 4)
    # every component its own numbers: a component read from a neighbour's place in the image shows
    args = (0, rows, TAPS9, np.arange(nc), P % 2, row, col0, 3, 4, W, _basis(rs, P, T))
    want = features(x, 0, *args[:3], *args[4:])
    ok = ~np.isnan(want).any(axis=(1, 2))
    assert ok.sum() > 10 and len({want[ok][:, p].tobytes() for p in range(P)}) == P
    _both(ck, args, want, P)
    ck.free()


# T alone, then the largest images: P * T = 8192 entries, 32 KiB of LDS, as one remainder block of 2 and as four blocks of PB
@pytest.mark.parametrize('T,P', [(1, 1), (1, 9), (2, 3), (61, 3), (61, 6), (256, 3), (4096, 2), (256, 32), (4096, 1)])
def test_basis_images_up_to_the_limit(T, P):
    rs = np.random.RandomState(T + P)
    rows, nc, W = 5000, 6, 3
    assert P * T <= hip.FEATURES_MAX_BASIS and ((T, P) not in ((4096, 2), (256, 32)) or P * T == hip.FEATURES_MAX_BASIS)
    x = (rs.randn(rows, nc) * 100).astype(np.float32)
    ck = Chunks(x, 2000)
    before = T // 2
    n = 12 if T > 1000 else 60
    row, col0 = _events(rs, rows, nc, W, n, before, T - before)
    args = (0, rows, [1.0], np.arange(nc), 0, row, col0, before, T - before, W, _basis(rs, P, T))
    want = features(x, 0, *args[:3], *args[4:])
    nan = np.isnan(want)
    assert nan.any() and not nan.all()
    _both(ck, args, want, (T, P))
    ck.free()


def test_clipping_at_every_edge():
    rows, nc, W, before, after, P = 900, 10, 6, 4, 5, 3
    rs = np.random.RandomState(2)
    x = synth_int16(0, rows, nc, 2)
    ck = Chunks(x, 250)
    basis = _basis(rs, P, before + after)
    # the rows: the first and the last that are whole, and their neighbours
    edge_rows = [0, 1, before - 1, before, rows - after, rows - after + 1, rows - 1]
    whole = [False, False, False, True, True, False, False]
    row = np.repeat(edge_rows, 3).astype(np.int64)
    col0 = np.tile([0, -2, nc - W + 1], len(edge_rows)).astype(np.int64)
    args = (0, rows, TAPS9, np.arange(nc), 1, row, col0, before, after, W, basis)
    want = features(x, 0, *args[:3], *args[4:])
    nan = np.isnan(want)
    assert nan.any() and not nan.all() and (nan.all(axis=1) == nan.any(axis=1)).all()
    for k, w in enumerate(whole):                                      # a clipped row: the whole event; else the positions outside
        assert nan[3 * k].all() != w and (not w or (nan[3 * k + 1, :, :2].all() and not nan[3 * k + 1, :, 2:].any()))
        assert not w or (nan[3 * k + 2, :, -1].all() and not nan[3 * k + 2, :, :-1].any())
    _both(ck, args, want, 'rows')
    # the first positions from -W to n_cols: from all outside over some to none and back
    col0 = np.arange(-W, nc + 1).astype(np.int64)
    row = np.full(col0.size, 450, np.int64)
    args = (0, rows, [1.0], np.arange(nc), 0, row, col0, before, after, W, basis)
    want = features(x, 0, *args[:3], *args[4:])
    outside = np.isnan(want).all(axis=1).sum(axis=1)
    assert outside.tolist() == [max(0, -c) + max(0, c + W - nc) for c in col0.tolist()] and outside[0] == W and outside[-1] == W
    assert ((outside > 0) & (outside < W)).sum() >= 2 * (W - 1) and (outside == 0).any()      # events with some but not all positions NaN
    _both(ck, args, want, 'positions')
    # the recording a window of the chunks' rows: the valid range clips as the file's ends do
    row = np.array([200, 200 + before - 1, 200 + before, 450, 700 - after, 700 - after + 1, 699], np.int64)
    args = (200, 700, TAPS9, np.arange(nc), 1, row, np.array([0, 1, -1, 5, 2, 3, 4]), before, after, W, basis)
    want = features(x[200:700], 200, *args[:3], *args[4:])
    assert np.isnan(want).all(axis=(1, 2)).tolist() == [True, True, False, False, False, True, True]
    assert np.isnan(want[2, :, 0]).all() and not np.isnan(want[2, :, 1:]).any() and np.isnan(want[3, :, -1]).all()
    _both(ck, args, want, 'window')
    ck.free()


def test_special_values():
    rs = np.random.RandomState(5)
    rows, nc, T = 800, 8, 4
    x = rs.randn(rows, nc).astype(np.float32)
    x[100, 0], x[110, 1], x[120, 2] = np.nan, np.inf, -np.inf
    x[130, 3], x[131, 3], x[132, 3], x[133, 3] = 1e-42, -3e-45, 1e-43, 2e-44     # denormals: so is their sum
    x[140, 4], x[141, 4] = 0.0, -0.0
    x[150:154, 5] = -0.0
    x[160, 6], x[161, 6] = 3e38, 3e38                                  # sums that overflow
    x[300:302] = np.nan                                                # whole rows
    ck = Chunks(x, 300)
    basis = np.array([[1.0, 1.0, 1.0, 1.0],
                      [0.0, 1.0, 0.0, 1.0],                            # inf * 0 is NaN, and so is inf - inf
                      [-1.0, 0.5, -0.0, 2.0],
                      [1e-40, 1e-40, -1e-40, 1e-40],                    # a denormal basis
                      [1e20, -1e20, 1e20, 1e20],
                      [0.0, 0.0, 0.0, 0.0],
                      [1.0, -1.0, 1.0, -1.0],
                      [2.0 ** -100, 2.0 ** -126, 2.0 ** -149, 2.0 ** -140],
                      [3e38, 3e38, 3e38, 3e38]], np.float32)
    assert basis.shape[0] == PB + 1                                    # (a full block and a remainder)
    planted = [100, 110, 120, 130, 131, 132, 133, 140, 141, 150, 151, 152, 153, 160, 161, 300, 301]
    row = np.sort(np.concatenate([np.array(planted) + d for d in (-1, 0, 1, 2)] + [rs.randint(2, rows - 2, 40)])).astype(np.int64)
    args = (0, rows, [1.0], np.arange(nc), 0, row, np.zeros(row.size, np.int64), 2, 2, nc, basis)
    want = features(x, 0, *args[:3], *args[4:])
    wave = ck.waveforms(0, rows, [1.0], np.arange(nc), 0, row, np.zeros(row.size, np.int64), 2, 2, nc)
    _same(want, chain(wave, basis), 'oracle')
    e = int(np.searchsorted(row, 109))                                 # the event at row 109 holds x[110, 1] = inf at tau 3
    assert row[e] == 109 and want[e, 0, 1] == np.inf and np.isnan(want[e, 5, 1]) and want[e, 1, 1] == np.inf and want[e, 6, 1] == -np.inf
    e = int(np.searchsorted(row, 111))                                 # ... and this one at tau 1
    assert want[e, 0, 1] == np.inf and np.isnan(want[e, 5, 1]) and want[e, 1, 1] == np.inf
    e = int(np.searchsorted(row, 112))                                 # at tau 0: component 1 has a zero there
    assert np.isnan(want[e, 1, 1]) and want[e, 2, 1] == -np.inf
    tiny = np.finfo(np.float32).tiny
    sub = (np.abs(want) > 0) & (np.abs(want) < tiny)
    assert sub.sum() >= 20 and sub[:, 0].any() and sub[:, 3].any() and sub[:, 7].any()       # denormal results are kept, not flushed
    assert np.isinf(want[:, 8]).any() and np.isinf(want[:, 0, 6]).any() and not (want.view(np.uint32) == 0x80000000).any()
    assert (want[:, 5].view(np.uint32)[~np.isnan(want[:, 5])] == 0).all()                    # finite * 0 from +0: +0
    assert (want.view(np.uint32)[np.isnan(want)] == 0x7fc00000).all()
    _both(ck, args, want)
    ck.free()


def test_host_seams_and_the_snippets_of_dev_waveforms(monkeypatch):
    rs = np.random.RandomState(6)
    rows, nc = 6000, 16
    x = synth_int16(0, rows, nc, 11)
    row = rs.randint(0, rows, 260)
    row = np.sort(row[((row < 1200) | (row >= 1800)) & ((row < 4300) | (row >= 4800))]).astype(np.int64)      # two stretches without events, each inside a chunk
    n = row.size
    col0 = rs.randint(-3, nc, n).astype(np.int64)
    basis = _basis(rs, 6, 61)
    args = (0, rows, TAPS65, np.arange(nc), 1, row, col0, 20, 41, 7, basis)
    want = features(x, 0, *args[:3], *args[4:])
    knobs = ('MTS_PIPE_BYTES', 'MTS_WAVEFORMS_SLAB_BYTES', 'MTS_WAVEFORMS_GAP_ROWS')
    plans = []
    for chunk, pipe, slab, gap in ((1000, None, None, None), (1000, 40000, 20000, 100), (700, 40000, None, -1), (6000, None, 1, 0),
                                   (1000, None, 30000, None)):
        ck = Chunks(x, chunk)
        for name, v in zip(knobs, (pipe, slab, gap)):
            monkeypatch.delenv(name, raising=False)
            if v is not None:
                monkeypatch.setenv(name, str(v))
        _same(ck.feat(False, *args), want, (chunk, pipe, slab, gap))
        plans.append(hip.waveforms_last_plan(0))
        _same(ck.feat(True, *args), want, (chunk, pipe, slab, gap, 'dev'))
        ck.free()
    for name in knobs:
        monkeypatch.delenv(name, raising=False)
    print(plans)
    # chunks of 32 000 bytes: pieces of one chunk; slabs of 312 rows; the two empty stretches are gaps at 100 rows
    assert plans[1]['pieces'] >= 3 and plans[1]['slabs'] > plans[0]['slabs'] and plans[1]['gap_cuts'] >= 2, plans
    assert plans[2]['pieces'] >= 3 and plans[2]['gap_cuts'] == 0, plans
    assert plans[3]['slabs'] >= 100 and plans[4]['slabs'] >= 3, plans    # (a cap of one row: T rows, nearly a slab per event)
    assert all(p['gather_us'] == 0 for p in plans)
    # the gather's microseconds are reported for this call too
    ck = Chunks(x, 1000)
    monkeypatch.setenv('MTS_WAVEFORMS_TIME', '1')
    _same(ck.feat(True, *args), want, 'timed')
    assert hip.waveforms_last_plan(0)['gather_us'] > 0
    monkeypatch.delenv('MTS_WAVEFORMS_TIME')
    # identity on the device: the chain on mts_dev_waveforms' own snippets of the same events
    w = ck.waveforms(0, rows, TAPS65, np.arange(nc), 1, row, col0, 20, 41, 7)
    assert np.isnan(w).any() and not np.isnan(w).all()
    assert chain(w, basis).tobytes() == want.tobytes()
    ck.free()


def test_reader_on_detects_events_shuffled_resident_cold_and_lanes(tmp_cfg, monkeypatch):
    x = synth_int16(0, 5000, 40, 4)
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=1000., n_channels=40, dtype=x.dtype, check_after_compress=False)
    one = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, codec=api.HipCodec(devices=[0]))
    two = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, codec=api.HipCodec(devices=[0, 0]))
    assert one.n_chunks >= 4
    ev = one.detect(14.0, taps=TAPS65, sign='both', reference='median', exclude=30, spread=5)
    assert 50 <= ev.sample.size <= 400
    kw = dict(neighbours=8, taps=TAPS65, reference='median')
    snip = one.waveforms(ev.sample, ev.channel, **kw).waveforms
    basis = api.waveform_basis(snip, 3)
    # a shuffled sample with repeats
    rs = np.random.RandomState(8)
    pick = np.concatenate((rs.permutation(ev.sample.size), rs.randint(0, ev.sample.size, 30)))
    sample, channel = ev.sample[pick], ev.channel[pick]
    cold = one.waveform_features(sample, basis, channel, **kw)
    want = features(x, 0, 0, 5000, TAPS65, 1, sample, channel - 8, 20, 41, 17, basis)
    assert cold.features.shape == (pick.size, 3, 17) and np.isnan(want).any() and not np.isnan(want).all()
    _same(cold.features, want)
    _same(cold.features, chain(snip, basis)[pick])                      # the chain on Reader.waveforms' own snippets
    _same(two.waveform_features(sample, basis, channel, **kw).features, want)                      # one device == two lanes
    _same(one.waveform_features(sample, basis[1], channel, **kw).features, want[:, 1])             # a 1-D basis
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1)
    _same(one.waveform_features(sample, basis, channel, **kw).features, want)
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1 << 30)
    monkeypatch.setattr(api, 'WAVEFORMS_OUT_BYTES', 7 * 4 * 3 * 17)                                # 7 events per call
    _same(one.waveform_features(sample, basis, channel, **kw).features, want)
    monkeypatch.setattr(api, 'WAVEFORMS_OUT_BYTES', 1 << 30)
    keys = list(range(one.n_chunks))
    one[:]                                                                                         # (read-ahead makes chunks resident)
    for k in range(one.n_chunks):
        one[one.chunk_bounds[k]:one.chunk_bounds[k] + 1]
    cache = one._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 40 for b in before) >= len(keys) // 2
    _same(one.waveform_features(sample, basis, channel, **kw).features, want)                      # resident == cold
    assert hip.cache_query(cache, keys).tolist() == before                                         # the projection inserted nothing
    # full width
    full = one.waveform_features(sample, _basis(rs, 9, 61), taps=TAPS65)
    _same(full.features, features(x, 0, 0, 5000, TAPS65, 0, sample, np.zeros(pick.size, int), 20, 41, 40, full.basis))
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
    b5 = np.arange(10, dtype=np.float32).reshape(2, 5) - 3

    def call(dev=False, row0=0, rows=100, taps=(1.0, 0.5), vb=0, ve=100, cols=(0, 1), ref=0, ev=(10, 10, 50), col0=(0, -1, 1), n_ev=None,
             before=2, after=3, width=2, basis=b5, P=None, itemsize=2, flags=hip.make_flags(), out=True, events=True):
        a = [np.array(v, dtype=np.int64) for v in ([0], [row0], [0], [len(z)], [rows])]
        c, t = np.array(cols, dtype=np.int32), np.array(taps, dtype=np.float64)
        er, ec = np.array(ev, dtype=np.int64), np.array(col0, dtype=np.int32)
        bs = None if basis is None else np.ascontiguousarray(basis, dtype=np.float32)
        o = np.full(4096, 5, np.float32)
        st = np.full(1, 99, np.int32)
        keep.append((a, c, t, er, ec, bs, o, st))
        lp = [v.ctypes.data_as(C.POINTER(C.c_long)) for v in a]
        n = len(er) if n_ev is None else n_ev
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        mid = (vb, ve, len(t), t.ctypes.data_as(C.POINTER(C.c_double)), len(c), c.ctypes.data_as(ip), ref, n,
               er.ctypes.data_as(C.POINTER(C.c_long)) if events else None, ec.ctypes.data_as(ip) if events else None, before, after, width,
               (bs.shape[0] if bs is not None else 2) if P is None else P, None if bs is None else bs.ctypes.data_as(fp))
        stp = st.ctypes.data_as(ip)
        po = (d_out.at() if dev else hip._ptr(o)) if out else None
        if dev:
            rc = L.mts_dev_waveform_features(0, None, cbuf.at(), lp[2], lp[3], lp[1], lp[4], 1, nc, itemsize, flags, *mid, po, stp)
        else:
            rc = L.mts_waveform_features(0, 0, 1, lp[0], lp[1], data.ctypes.data_as(C.c_void_p), lp[2], lp[3], lp[4], nc, itemsize, flags, *mid, po, stp)
        return rc, int(st[0]), o
    said = {}
    for dev in (False, True):
        rc, st, o = call(dev=dev)
        assert (rc, st) == (0, 0)
        if not dev:
            want = features(x[:, :2], 0, 0, 100, [1.0, 0.5], 0, [10, 10, 50], [0, -1, 1], 2, 3, 2, b5)
            assert o[:12].tobytes() == want.tobytes() and o[12] == 5 and np.isnan(want).any() and not np.isnan(want).all()
            rc, st, o = call(ev=(), col0=())                            # no events: nothing launched, nothing written
            assert (rc, st) == (0, 0) and (o == 5).all()
        assert call(dev=dev, n_ev=0, events=False)[:2] == (0, 0)
        assert call(dev=dev, before=0, after=1, width=1, basis=[[2.0]])[:2] == (0, 0)
        assert call(dev=dev, basis=np.ones((32, 5)))[:2] == (0, 0)
        assert call(dev=dev, ev=(50,), col0=(0,), before=2048, after=2048, basis=np.ones((2, 4096)))[:2] == (0, 0)     # 8192 entries
        nan, inf = np.full((2, 5), 1.0), np.full((2, 5), 1.0)
        nan[1, 2], inf[0, 4] = np.nan, -np.inf
        for bad in (dict(ev=(10, 9, 50)), dict(ev=(10, 10, 100)), dict(ev=(-1, 10, 50)), dict(vb=20), dict(ve=40),
                    dict(before=-1), dict(after=-1), dict(before=0, after=0), dict(before=4096, after=1), dict(width=0), dict(width=1025),
                    dict(n_ev=-1), dict(events=False),
                    dict(P=0), dict(P=-1), dict(P=33, basis=np.ones((33, 5))), dict(before=128, after=129, basis=np.ones((32, 257))),
                    dict(before=2048, after=2049, basis=np.ones((2, 4097))), dict(before=1000, after=1000, basis=np.ones((5, 2000))),
                    dict(basis=None), dict(out=False), dict(basis=nan), dict(basis=inf),
                    dict(taps=(np.inf, 1.0)), dict(taps=()), dict(cols=(0, 4)), dict(cols=(-1,)), dict(cols=()), dict(ref=2), dict(row0=10),
                    dict(rows=50), dict(itemsize=3), dict(flags=hip.FLAG_FLOAT, itemsize=2)):
            rc, st, o = call(dev=dev, **bad)
            assert rc == -1, bad                                       # MTS_E_ARG ...
            assert st == 99 and (dev or (o == 5).all()), bad           # ... before anything ran
            msg = hip.lib().mts_last_error().decode()
            assert msg, bad
            if set(bad) & {'P', 'basis', 'out', 'before', 'after', 'width', 'ev', 'n_ev', 'events', 'vb', 've'}:
                assert msg.startswith('waveform_features:'), (bad, msg)
            said[str(sorted(bad))] = msg
    assert said["['P']"] == 'waveform_features: -1 components (1 .. 32)'
    assert said["['P', 'basis']"] == 'waveform_features: 33 components (1 .. 32)'
    assert said["['after', 'basis', 'before']"] == 'waveform_features: 5 components x 2000 rows (<= 8192 entries in all)'
    assert said["['basis']"] == 'waveform_features: basis[0, 4] is not finite'
    assert said["['out']"] == 'waveform_features: no output buffer'
    assert call(basis=None)[0] == -1 and hip.lib().mts_last_error().decode() == 'waveform_features: no basis'
    assert call(basis=nan)[0] == -1 and hip.lib().mts_last_error().decode() == 'waveform_features: basis[1, 2] is not finite'
    assert call(width=0)[0] == -1 and hip.lib().mts_last_error().decode() == 'waveform_features: width 0 (1 .. 1024)'
    assert call(ev=(10, 9, 50))[0] == -1 and hip.lib().mts_last_error().decode() == 'waveform_features: event 1: the rows must ascend'
    d_out.free()
    cbuf.free()
