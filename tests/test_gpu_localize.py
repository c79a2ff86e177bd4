"""mts_localize / mts_dev_localize and the Reader on top of them on the MI355X: k_localize against the numpy restatement of the
definition (tests/localize_oracle.py), for equality of every byte of amplitude, weight, moment and best: widths either side of every
seam of the event-to-workgroup mapping, snippet lengths, dimensions and modes, clipping at every edge, special values, every seam of
the host side (chunks, pieces, slabs, gaps, residency), the definition on mts_dev_waveforms' own snippets, the Reader, argument
errors."""
import ctypes as C

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.localize_oracle import MODES, localize, location, reduce_snippets

pytestmark = pytest.mark.gpu

TAPS9 = np.random.RandomState(1).randn(9)
TAPS65 = api.highpass_taps(300, 5000, 65)
THREADS = 256                                                          # LOC_THREADS (csrc/localize.hip): threads of a workgroup
FILL_BITS = 0x7fc00000


def group(W):
    """Events of a workgroup (launch_localize): THREADS / W whole events for W <= THREADS, one event whose positions the threads stride
    over beyond; the LDS stride of an event is W | 1."""
    return THREADS // W if W <= THREADS else 1


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

    def loc(self, dev, *args, want_amp=True):
        """(amplitude, weight, moment, best) of mts_dev_localize / mts_localize for the op's own arguments."""
        if dev:
            st, res, buf = hip.dev_localize(*self.dev(), *args, want_amp=want_amp)
            buf.free()
        else:
            st, *res = hip.localize(*self.host(), *args, want_amp=want_amp)
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
    """got: (amplitude or None, weight, moment, best int32) of the device; want: the oracle's four (best int64)."""
    assert len(got) == 4 and got[3].dtype == np.int32, what
    for name, g, w in zip(('amplitude', 'weight', 'moment', 'best'), got, want[:3] + (want[3].astype(np.int32),)):
        if g is None:
            assert name == 'amplitude'
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:4].tolist())


def _both(ck, args, want, what=None):
    for dev in (False, True):
        _same(ck.loc(dev, *args), want, (what, dev))


def _want(x, args, x_row0=0):
    return localize(x, x_row0, *args[:3], *args[4:])


def _positions(rs, n_cols, D):
    p = (rs.standard_normal((n_cols, D)) * 100).astype(np.float32)
    p[rs.rand(n_cols, D) < 0.05] = 0.0
    return p


def _events(rs, rows, n_cols, width, n, before, after):
    """n events by ascending row: a few at both ends of the recording (clipped: fewer rows), repeats, the rest inside; first positions
    from left of the columns to right of them."""
    fixed = [0, before - 1 if before else 0, rows - 1, rows // 2, rows // 2][:min(n, 5)]
    row = np.sort(np.concatenate((fixed, rs.randint(before, rows - after + 1, n - len(fixed))))).astype(np.int64)
    col0 = rs.randint(-width, n_cols + 1, n)
    col0[:4] = [0, -width + 1, n_cols - 1, max(0, n_cols - width)][:min(n, 4)]
    return row, col0.astype(np.int64)


def _counts(W):
    """Event counts of one slab that put the last workgroup at one event and at a full complement, with more than one workgroup."""
    G = group(W)
    return [3 * G, 2 * G + 1] if G > 1 else [1, 3]


def test_counts_reach_the_seams():
    assert [group(W) for W in (1, 5, 16, 17, 33, 64, 65, 127, 128, 129, 255, 256, 257, 385, 1024)] == [256, 51, 16, 15, 7, 4, 3, 2, 2, 1, 1, 1, 1, 1, 1]
    assert _counts(1) == [768, 513] and _counts(17) == [45, 31] and _counts(128) == [6, 5] and _counts(129) == [1, 3]
    for W in range(1, 1025):                                           # the workgroup's amplitudes fit the kernel's LDS array of 1025 floats
        assert group(W) * (W | 1) <= 1025 and group(W) * W <= max(THREADS, W)


@pytest.mark.parametrize('W', [1, 5, 16, 17, 33, 64, 65, 127, 128, 129, 255, 256, 257, 385, 1024])
def test_widths_either_side_of_every_seam_of_the_event_mapping(W):
    rs = np.random.RandomState(W)
    rows, nc = (1500, 70) if W <= 70 else (300, 1024)
    case = W
    for dtype in (np.int16, np.float32):
        x = synth_int16(0, rows, nc, W) if dtype == np.int16 else (rs.randn(rows, nc) * 300).astype(np.float32)
        ck = Chunks(x, 600)
        for n in _counts(W):
            row, col0 = _events(rs, rows, nc, W, n, 2, 3)
            if W >= nc:
                col0[::2] = 0
            ref, taps = case % 2, (TAPS9 if case % 3 else [1.0])
            mode, D = case % 4, 1 + (case // 2) % 4
            case += 1
            args = (0, rows, taps, np.arange(nc), ref, row, col0, 2, 3, W, mode, _positions(rs, nc, D))
            want = _want(x, args)
            nan = np.isnan(want[0])
            assert (nan.any() or n < 3) and not nan.all() and (want[1] > 0).any()
            _both(ck, args, want, (dtype, n, ref, mode, D))
            assert hip.waveforms_last_plan(0)['slabs'] == 1              # the workgroups run over the events of a slab: all of them
        ck.free()


@pytest.mark.parametrize('T', [1, 2, 61, 4096])
def test_snippet_lengths_with_no_rows_before_and_none_after(T):
    rs = np.random.RandomState(T)
    rows, nc, W = 9000, 6, 3
    x = (rs.randn(rows, nc) * 100).astype(np.float32)
    ck = Chunks(x, 4000)
    n = 12 if T > 1000 else 60
    for before, after in ((0, T), (T, 0)):
        row, col0 = _events(rs, rows, nc, W, n, before, after)
        for mode in (0, 3):
            args = (0, rows, [1.0], np.arange(nc), 0, row, col0, before, after, W, mode, _positions(rs, nc, 2))
            want = _want(x, args)
            assert np.isnan(want[0]).any() and not np.isnan(want[0]).all()
            if T == 1 and mode == 0:                                     # one entry: hi - lo = +0, and no weight
                assert not want[0].view(np.uint32)[~np.isnan(want[0])].any() and not want[1].view(np.uint32).any()
            _both(ck, args, want, (T, before, mode))
    ck.free()


@pytest.mark.parametrize('D', [1, 2, 3, 4])
def test_dimensions_and_modes(D):
    rs = np.random.RandomState(40 + D)
    rows, nc, W = 1200, 12, 5
    x = synth_int16(0, rows, nc, D)
    ck = Chunks(x, 500)
    row, col0 = _events(rs, rows, nc, W, 70, 3, 4)
    pos = _positions(rs, nc, D)
    seen = set()
    for name, mode in MODES.items():
        args = (0, rows, TAPS9, np.arange(nc), D % 2, row, col0, 3, 4, W, mode, pos)
        want = _want(x, args)
        seen.add(want[0].tobytes())
        # every coordinate its own numbers: a moment read from a neighbour's place shows
        assert len({want[2][:, d].tobytes() for d in range(D)}) == D and want[2].shape == (70, D)
        _both(ck, args, want, (name, D))
        _same(ck.loc(True, *args, want_amp=False), want, 'no amplitudes')      # out_amp null: everything else is the same bytes
        _same(ck.loc(False, *args, want_amp=False), want, 'no amplitudes')
    assert len(seen) == 4
    ck.free()


def test_clipping_at_every_edge():
    rows, nc, W, before, after = 900, 10, 6, 4, 5
    rs = np.random.RandomState(2)
    x = synth_int16(0, rows, nc, 2)
    ck = Chunks(x, 250)
    pos = _positions(rs, nc, 3)
    # events at the rows 0, before - 1 and N - 1 and their neighbours: fewer rows, never none
    edge_rows = [0, 1, before - 1, before, rows - after, rows - after + 1, rows - 1]
    row = np.repeat(edge_rows, 3).astype(np.int64)
    col0 = np.tile([0, -2, nc - W + 1], len(edge_rows)).astype(np.int64)
    for mode in range(4):
        args = (0, rows, TAPS9, np.arange(nc), 1, row, col0, before, after, W, mode, pos)
        want = _want(x, args)
        nan = np.isnan(want[0])
        assert not nan[0::3].any() and nan[1::3, :2].all() and not nan[1::3, 2:].any() and nan[2::3, -1].all() and not nan[2::3, :-1].any()
        _both(ck, args, want, ('rows', mode))
    # the first positions from -W to n_cols: from all outside over some to none and back
    col0 = np.arange(-W, nc + 1).astype(np.int64)
    row = np.full(col0.size, 450, np.int64)
    args = (0, rows, [1.0], np.arange(nc), 0, row, col0, before, after, W, 0, pos)
    want = _want(x, args)
    outside = np.isnan(want[0]).sum(axis=1)
    assert outside.tolist() == [max(0, -c) + max(0, c + W - nc) for c in col0.tolist()] and outside[0] == W and outside[-1] == W
    for e in (0, -1):                                                  # every position outside: NaN amplitudes, weight and moment +0, no best
        assert (want[0][e].view(np.uint32) == FILL_BITS).all() and want[1].view(np.uint32)[e] == 0 and not want[2][e].view(np.uint32).any()
        assert want[3][e] == -1
    assert (want[3][1:-1] >= 0).all()
    _both(ck, args, want, 'positions')
    # the recording a window of the chunks' rows: the valid range clips as the file's ends do
    row = np.array([200, 200 + before - 1, 200 + before, 450, 700 - after, 700 - after + 1, 699], np.int64)
    args = (200, 700, TAPS9, np.arange(nc), 1, row, np.array([0, 1, -1, 5, 2, 3, 4]), before, after, W, 1, pos)
    want = _want(x[200:700], args, 200)
    assert not np.isnan(want[0][0]).any() and np.isnan(want[0][2, 0]) and not np.isnan(want[0][2, 1:]).any() and np.isnan(want[0][3, -1])
    whole = _want(x, (0, rows) + args[2:])                              # (the rows beyond the window are not read: other amplitudes)
    assert whole[0][0].tobytes() != want[0][0].tobytes() and whole[0][3].tobytes() == want[0][3].tobytes()
    _both(ck, args, want, 'window')
    # (an event whose every row lies outside the recording cannot be given: its own row is inside; all-NaN rows stand in for it in
    # test_special_values)
    ck.free()


def test_special_values():
    rs = np.random.RandomState(5)
    rows, nc = 800, 12
    x = rs.randn(rows, nc).astype(np.float32)
    x[100, 0], x[110, 1], x[120, 2], x[121, 2] = np.nan, np.inf, -np.inf, np.inf
    x[130, 3], x[131, 3], x[132, 3], x[133, 3] = 1e-42, -3e-45, 1e-43, 2e-44     # denormals: so are their amplitudes
    x[128:136, 4] = 0.0
    x[140:150, 4], x[141, 4], x[143, 4] = 0.0, -0.0, -0.0              # zeros of both signs
    x[150:160, 5] = [-3.0, 2.0, -3.0, 2.0, 0.0, 2.0, -3.0, 0.0, -3.0, 2.0]      # equal extrema at several taus ...
    x[150:160, 6] = x[150:160, 5]                                      # ... and equal amplitudes at several positions
    x[150:160, 8] = x[150:160, 5]
    x[160, 7], x[161, 7] = 3e38, -3e38                                 # an amplitude that overflows to +inf
    x[150:154, 7] = 0.5                                                # (between the tied columns: a smaller amplitude in every mode)
    x[:, 9] = np.nan                                                   # a column that is NaN throughout
    x[300:302] = np.nan                                                # whole rows
    x[400:420] = np.nan                                                # whole snippets
    x[500:504, 10] = [1e-42, 1e-42, 1e-42, 1e-42]
    ck = Chunks(x, 300)
    pos = _positions(rs, nc, 4)
    pos[7] = [0.0, 5.0, -5.0, 3e38]                                    # inf * 0 is NaN; inf * 5 is inf
    pos[3] = [1e-40, 2.0 ** -126, -1.0, 1.0]
    planted = [100, 110, 120, 130, 131, 132, 133, 141, 143, 150, 155, 159, 160, 161, 300, 301, 405, 410, 501]
    row = np.sort(np.concatenate([np.array(planted) + d for d in (-1, 0, 1, 2)] + [rs.randint(2, rows - 2, 40)])).astype(np.int64)
    tiny = np.finfo(np.float32).tiny
    for name, mode in MODES.items():
        args = (0, rows, [1.0], np.arange(nc), 0, row, np.zeros(row.size, np.int64), 2, 2, nc, mode, pos)
        want = _want(x, args)
        wave = ck.waveforms(0, rows, [1.0], np.arange(nc), 0, row, np.zeros(row.size, np.int64), 2, 2, nc)
        _same(tuple(a if a.dtype != np.int64 else a.astype(np.int32) for a in reduce_snippets(wave, np.zeros(row.size, np.int64), pos, mode)),
              want, 'oracle')
        amp, weight, moment, best = want
        assert (amp[:, 9].view(np.uint32) == FILL_BITS).all()
        e = int(np.searchsorted(row, 160))                             # rows 158 .. 161: both 3e38 and -3e38
        assert row[e] == 160
        assert np.isfinite(amp[e, 7]) == (name != 'ptp')
        if name == 'ptp':
            assert amp[e, 7] == np.inf and weight[e] == np.inf and moment.view(np.uint32)[e, 0] == FILL_BITS and moment[e, 1] == np.inf
            assert moment[e, 2] == -np.inf
            sub = (amp > 0) & (amp < tiny)
            assert sub[:, 3].any() and sub[:, 10].sum() == 0 and (amp[:, 10].view(np.uint32) == 0).any()
            e5 = int(np.searchsorted(row, 152))
            assert amp[e5, 5] == 5.0 and amp[e5, 5] == amp[e5, 6] == amp[e5, 8]
        e4 = int(np.searchsorted(row, 405))                            # every row NaN: no amplitude, no weight, no best
        assert (amp[e4].view(np.uint32) == FILL_BITS).all() and weight.view(np.uint32)[e4] == 0 and best[e4] == -1
        assert not moment[e4].view(np.uint32).any()
        for a in (amp, weight, moment):
            assert (a.view(np.uint32)[np.isnan(a)] == FILL_BITS).all()
        assert not (weight.view(np.uint32) == 0x80000000).any() and not (moment.view(np.uint32) == 0x80000000).any()
        _both(ck, args, want, name)
    # a narrow snippet on the tied columns: best is the lowest of the equal amplitudes
    row = np.array([152, 152, 155], np.int64)
    col0 = np.array([5, 4, 5], np.int64)
    for mode in range(4):
        args = (0, rows, [1.0], np.arange(nc), 0, row, col0, 2, 2, 4, mode, pos)
        want = _want(x, args)
        assert want[3][0] == 0 and want[0][0, 0] == want[0][0, 1] == want[0][0, 3] and want[3][1] == 1
        _both(ck, args, want, ('ties', mode))
    ck.free()


def test_host_seams_and_the_snippets_of_dev_waveforms(monkeypatch):
    rs = np.random.RandomState(6)
    rows, nc = 6000, 16
    x = synth_int16(0, rows, nc, 11)
    row = rs.randint(0, rows, 260)
    row = np.sort(row[((row < 1200) | (row >= 1800)) & ((row < 4300) | (row >= 4800))]).astype(np.int64)      # two stretches without events, each inside a chunk
    n = row.size
    col0 = rs.randint(-3, nc, n).astype(np.int64)
    pos = _positions(rs, nc, 3)
    args = (0, rows, TAPS65, np.arange(nc), 1, row, col0, 20, 41, 7, 0, pos)
    want = _want(x, args)
    knobs = ('MTS_PIPE_BYTES', 'MTS_WAVEFORMS_SLAB_BYTES', 'MTS_WAVEFORMS_GAP_ROWS')
    plans = []
    for chunk, pipe, slab, gap in ((1000, None, None, None), (1000, 40000, 20000, 100), (700, 40000, None, -1), (6000, None, 1, 0),
                                   (1000, None, 30000, None), (600, None, None, None)):
        ck = Chunks(x, chunk)
        for name, v in zip(knobs, (pipe, slab, gap)):
            monkeypatch.delenv(name, raising=False)
            if v is not None:
                monkeypatch.setenv(name, str(v))
        _same(ck.loc(False, *args), want, (chunk, pipe, slab, gap))
        plans.append(hip.waveforms_last_plan(0))
        _same(ck.loc(True, *args), want, (chunk, pipe, slab, gap, 'dev'))
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
    _same(ck.loc(True, *args), want, 'timed')
    assert hip.waveforms_last_plan(0)['gather_us'] > 0
    monkeypatch.delenv('MTS_WAVEFORMS_TIME')
    # identity on the device: the definition on mts_dev_waveforms' own snippets of the same events
    w = ck.waveforms(0, rows, TAPS65, np.arange(nc), 1, row, col0, 20, 41, 7)
    assert np.isnan(w).any() and not np.isnan(w).all()
    for a, b in zip(reduce_snippets(w, col0, pos, 0), want):
        assert a.tobytes() == b.tobytes()
    ck.free()


def test_resident_against_cold_chunks(tmp_cfg):
    x = synth_int16(0, 5000, 20, 3)
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=1000., n_channels=20, dtype=x.dtype, check_after_compress=False)
    r = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, codec=api.HipCodec(devices=[0]))
    rs = np.random.RandomState(3)
    sample, channel = rs.randint(0, 5000, 200), rs.randint(0, 20, 200)
    pos = _positions(rs, 20, 2)
    kw = dict(neighbours=4, taps=TAPS65, reference='median', amplitude='neg')
    cold = r.localize(sample, pos, channel, **kw)
    keys = list(range(r.n_chunks))
    cache = r._cache_for(0)
    assert not any(hip.cache_query(cache, keys).tolist())              # a localization inserts nothing
    r[:]
    for k in range(r.n_chunks):
        r[r.chunk_bounds[k]:r.chunk_bounds[k] + 1]
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 20 for b in before) >= len(keys) // 2
    warm = r.localize(sample, pos, channel, **kw)
    assert hip.cache_query(cache, keys).tolist() == before
    want = localize(x, 0, 0, 5000, TAPS65, 1, sample, channel - 4, 20, 41, 9, MODES['neg'], pos)
    for g in (cold, warm):
        _same((g.amplitude, g.weight, g.moment, g.best.astype(np.int32)), want)
    r.close()


def test_reader_on_detects_events_shuffled_resident_cold_and_lanes(tmp_cfg, monkeypatch):
    x = synth_int16(0, 5000, 40, 4)
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=1000., n_channels=40, dtype=x.dtype, check_after_compress=False)
    one = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, codec=api.HipCodec(devices=[0]))
    two = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False, codec=api.HipCodec(devices=[0, 0]))
    assert one.n_chunks >= 4
    ev = one.detect(14.0, taps=TAPS65, sign='neg', reference='median', exclude=30, spread=5)
    assert 30 <= ev.sample.size <= 400
    kw = dict(neighbours=8, taps=TAPS65, reference='median')
    k = np.arange(40)
    pos = np.stack([np.where(k % 2, 43.0, 11.0), 20.0 * (k // 2)], axis=1)
    # a shuffled sample with repeats
    rs = np.random.RandomState(8)
    pick = np.concatenate((rs.permutation(ev.sample.size), rs.randint(0, ev.sample.size, 30)))
    sample, channel = ev.sample[pick], ev.channel[pick]

    def check(g, want, flat=False):
        amp, weight, moment, best = want
        loc = location(moment, weight)
        chan = np.where(best >= 0, np.where(best >= 0, g.position + best, 0), -1)       # (channels is 0 .. 39: the position is the channel)
        for name, w in (('amplitude', amp), ('weight', weight), ('moment', moment[:, 0] if flat else moment), ('best', best),
                        ('location', loc[:, 0] if flat else loc), ('channel', chan)):
            assert g[name].dtype == w.dtype and g[name].shape == w.shape and g[name].tobytes() == w.tobytes(), name
    for mode in MODES:
        want = localize(x, 0, 0, 5000, TAPS65, 1, sample, channel - 8, 20, 41, 17, MODES[mode], pos)
        assert np.isnan(want[0]).any() and not np.isnan(want[0]).all()
        cold = one.localize(sample, pos, channel, amplitude=mode, **kw)
        check(cold, want)
        check(two.localize(sample, pos, channel, amplitude=mode, **kw), want)                      # one device == two lanes
    # the identities on the device: the trough and the peak of Reader.waveforms, and detect's amplitude
    w = one.waveforms(ev.sample, ev.channel, **kw)
    neg = one.localize(ev.sample, pos, ev.channel, amplitude='neg', **kw)
    assert np.nanmax(neg.amplitude, axis=1).tobytes() == (-w.trough.value).tobytes()
    assert np.nanmax(one.localize(ev.sample, pos, ev.channel, amplitude='pos', **kw).amplitude, axis=1).tobytes() == w.peak.value.tobytes()
    assert (neg.amplitude[:, 8] >= ev.amplitude).all() and (neg.amplitude[:, 8] >= -ev.amplitude).all()
    for a, b in zip(reduce_snippets(w.waveforms, ev.channel - 8, pos.astype(np.float32), MODES['neg']), (neg.amplitude, neg.weight, neg.moment, neg.best)):
        assert a.tobytes() == b.tobytes()
    want = localize(x, 0, 0, 5000, TAPS65, 1, sample, channel - 8, 20, 41, 17, 0, pos)
    flat = one.localize(sample, pos[:, 1], channel, **kw)                                          # 1-D positions
    want1 = localize(x, 0, 0, 5000, TAPS65, 1, sample, channel - 8, 20, 41, 17, 0, pos[:, 1:2])
    check(flat, want1, flat=True)
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1)
    check(one.localize(sample, pos, channel, **kw), want)
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1 << 30)
    monkeypatch.setattr(api, 'WAVEFORMS_OUT_BYTES', 7 * 4 * (17 + 2 + 2))                          # 7 events per call
    check(one.localize(sample, pos, channel, **kw), want)
    monkeypatch.setattr(api, 'WAVEFORMS_OUT_BYTES', 1 << 30)
    keys = list(range(one.n_chunks))
    one[:]                                                                                         # (read-ahead makes chunks resident)
    for k in range(one.n_chunks):
        one[one.chunk_bounds[k]:one.chunk_bounds[k] + 1]
    cache = one._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 40 for b in before) >= len(keys) // 2
    check(one.localize(sample, pos, channel, **kw), want)                                          # resident == cold
    assert hip.cache_query(cache, keys).tolist() == before                                         # the localization inserted nothing
    bare = one.localize(sample, pos, channel, amplitudes=False, **kw)
    assert bare.amplitude is None and bare.location.tobytes() == location(want[2], want[1]).tobytes()
    # full width
    full = one.localize(sample, pos, taps=TAPS65, amplitude='abs')
    check(full, localize(x, 0, 0, 5000, TAPS65, 0, sample, np.zeros(pick.size, int), 20, 41, 40, MODES['abs'], pos))
    one.close()
    two.close()


def test_c_abi_arguments():
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = np.arange(400, dtype=np.int16).reshape(100, nc)
    x[::7] *= -3
    z = hip.compress_chunks(x, [0, 100], hip.make_flags(), 6)[0]
    data = np.frombuffer(z + b'\0' * 16, dtype=np.uint8)
    cbuf = hip.DevBuffer(len(z) + 256)
    host = np.frombuffer(z + b'\0' * 256, dtype=np.uint8).copy()
    hip._check(L.mts_dev_copy(0, None, cbuf.at(), hip._ptr(host), host.nbytes, 0), 'mts_dev_copy')
    d_out = hip.DevBuffer(1 << 20)
    keep = []
    p2 = np.array([[0.0, 1.0], [2.0, -1.0]], np.float32)

    def call(dev=False, row0=0, rows=100, taps=(1.0, 0.5), vb=0, ve=100, cols=(0, 1), ref=0, ev=(10, 10, 50), col0=(0, -1, 1), n_ev=None,
             before=2, after=3, width=2, mode=0, pos=p2, D=None, itemsize=2, flags=hip.make_flags(), amp=True, weight=True, moment=True,
             best=True, events=True):
        a = [np.array(v, dtype=np.int64) for v in ([0], [row0], [0], [len(z)], [rows])]
        c, t = np.array(cols, dtype=np.int32), np.array(taps, dtype=np.float64)
        er, ec = np.array(ev, dtype=np.int64), np.array(col0, dtype=np.int32)
        ps = None if pos is None else np.ascontiguousarray(pos, dtype=np.float32)
        o = [np.full(64, 5, np.float32), np.full(64, 5, np.float32), np.full(64, 5, np.float32), np.full(64, 5, np.int32)]
        st = np.full(1, 99, np.int32)
        keep.append((a, c, t, er, ec, ps, o, st))
        lp = [v.ctypes.data_as(C.POINTER(C.c_long)) for v in a]
        n = len(er) if n_ev is None else n_ev
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        mid = (vb, ve, len(t), t.ctypes.data_as(C.POINTER(C.c_double)), len(c), c.ctypes.data_as(ip), ref, n,
               er.ctypes.data_as(C.POINTER(C.c_long)) if events else None, ec.ctypes.data_as(ip) if events else None, before, after, width, mode,
               (ps.shape[1] if ps is not None else 2) if D is None else D, None if ps is None else ps.ctypes.data_as(fp))
        stp = st.ctypes.data_as(ip)
        po = [(d_out.at(4096 * k) if dev else hip._ptr(o[k])) if on else None for k, on in enumerate((amp, weight, moment, best))]
        if dev:
            rc = L.mts_dev_localize(0, None, cbuf.at(), lp[2], lp[3], lp[1], lp[4], 1, nc, itemsize, flags, *mid, *po, stp)
        else:
            rc = L.mts_localize(0, 0, 1, lp[0], lp[1], data.ctypes.data_as(C.c_void_p), lp[2], lp[3], lp[4], nc, itemsize, flags, *mid, *po, stp)
        return rc, int(st[0]), o
    said = {}
    for dev in (False, True):
        rc, st, o = call(dev=dev)
        assert (rc, st) == (0, 0)
        if not dev:
            want = localize(x[:, :2], 0, 0, 100, [1.0, 0.5], 0, [10, 10, 50], [0, -1, 1], 2, 3, 2, 0, p2)
            assert o[0][:6].tobytes() == want[0].tobytes() and o[1][:3].tobytes() == want[1].tobytes() and o[2][:6].tobytes() == want[2].tobytes()
            assert o[3][:3].tolist() == want[3].tolist() and o[0][6] == 5 and o[1][3] == 5 and o[2][6] == 5 and o[3][3] == 5
            assert np.isnan(want[0]).any() and not np.isnan(want[0]).all()
            rc, st, o2 = call(amp=False)                                # no amplitudes: the other three are the same bytes
            assert (rc, st) == (0, 0) and (o2[0] == 5).all() and all(o2[k].tobytes() == o[k].tobytes() for k in (1, 2, 3))
            rc, st, o = call(ev=(), col0=())                            # no events: nothing launched, nothing written
            assert (rc, st) == (0, 0) and all((v == 5).all() for v in o)
        assert call(dev=dev, n_ev=0, events=False)[:2] == (0, 0)
        assert call(dev=dev, before=0, after=1, width=1)[:2] == (0, 0)
        assert call(dev=dev, amp=False)[:2] == (0, 0)
        for m in range(4):
            assert call(dev=dev, mode=m, pos=np.ones((2, 4)))[:2] == (0, 0)
        nan, inf = np.full((2, 2), 1.0), np.full((2, 2), 1.0)
        nan[1, 0], inf[0, 1] = np.nan, -np.inf
        for bad in (dict(ev=(10, 9, 50)), dict(ev=(10, 10, 100)), dict(ev=(-1, 10, 50)), dict(vb=20), dict(ve=40),
                    dict(before=-1), dict(after=-1), dict(before=0, after=0), dict(before=4096, after=1), dict(width=0), dict(width=1025),
                    dict(n_ev=-1), dict(events=False),
                    dict(mode=-1), dict(mode=4), dict(D=0), dict(D=-1), dict(D=5, pos=np.ones((2, 5))),
                    dict(pos=None), dict(weight=False), dict(moment=False), dict(best=False), dict(pos=nan), dict(pos=inf),
                    dict(taps=(np.inf, 1.0)), dict(taps=()), dict(cols=(0, 4)), dict(cols=(-1,)), dict(cols=()), dict(ref=2), dict(row0=10),
                    dict(rows=50), dict(itemsize=3), dict(flags=hip.FLAG_FLOAT, itemsize=2)):
            rc, st, o = call(dev=dev, **bad)
            assert rc == -1, bad                                       # MTS_E_ARG ...
            assert st == 99 and (dev or all((v == 5).all() for v in o)), bad           # ... before anything ran
            msg = hip.lib().mts_last_error().decode()
            assert msg, bad
            if set(bad) & {'mode', 'D', 'pos', 'weight', 'moment', 'best', 'before', 'after', 'width', 'ev', 'n_ev', 'events', 'vb', 've'}:
                assert msg.startswith('localize:'), (bad, msg)
            said[str(sorted(bad))] = msg
    assert said["['mode']"] == 'localize: mode 4 (0 .. 3)'
    assert said["['D']"] == 'localize: -1 dimensions (1 .. 4)'
    assert said["['D', 'pos']"] == 'localize: 5 dimensions (1 .. 4)'
    assert said["['pos']"] == 'localize: positions[0, 1] is not finite'
    assert said["['weight']"] == said["['moment']"] == said["['best']"] == 'localize: no weight, moment or best buffer'
    assert call(pos=None)[0] == -1 and hip.lib().mts_last_error().decode() == 'localize: no positions'
    assert call(pos=nan)[0] == -1 and hip.lib().mts_last_error().decode() == 'localize: positions[1, 0] is not finite'
    assert call(mode=-1)[0] == -1 and hip.lib().mts_last_error().decode() == 'localize: mode -1 (0 .. 3)'
    assert call(width=0)[0] == -1 and hip.lib().mts_last_error().decode() == 'localize: width 0 (1 .. 1024)'
    assert call(ev=(10, 9, 50))[0] == -1 and hip.lib().mts_last_error().decode() == 'localize: event 1: the rows must ascend'
    d_out.free()
    cbuf.free()
