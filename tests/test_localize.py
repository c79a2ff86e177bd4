"""Reader.localize, host side: argument handling, any order of the events, the 1-D positions, call cutting, lanes, cache use, the
host's quotient and errors, driven through a numpy restatement of mts_localize (tests/localize_oracle.py).  The kernel:
tests/test_gpu_localize.py."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.localize_oracle import MODES, LocalizeOracleCodec, localize, location, reduce_snippets

TAPS65 = api.highpass_taps(300, 5000, 65)
FILL_BITS = 0x7fc00000
FIELDS = ('location', 'amplitude', 'weight', 'moment', 'best', 'channel')


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _write(tmp, arr, codec, sample_rate=1000.):
    raw = tmp / 'data.bin'
    arr.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'data.cbin', tmp / 'data.ch', sample_rate=sample_rate, n_channels=arr.shape[1], dtype=arr.dtype,
                         codec=codec, check_after_compress=False, do_time_diff=arr.dtype.kind != 'f')
    return mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', codec=codec, check_after_decompress=False)


def _codec(n_lanes=1):
    return LocalizeOracleCodec(n_lanes=n_lanes, capacity_chunks=8)


def _grid(n, D=2):
    """A staggered two-column probe: x alternates, y rises by 20 every second channel; further coordinates are made up."""
    k = np.arange(n)
    cols = [np.where(k % 2, 43.0, 11.0), 20.0 * (k // 2), 0.5 * k - 3.0, np.cos(k)]
    return np.stack(cols[:D], axis=1)


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


def _same_bunch(a, b, index=None):
    for name in FIELDS:
        u, v = a[name], b[name]
        if u is None or v is None:
            assert u is None and v is None
            continue
        _same(u, v if index is None else v[index])


def _want(x, cols, taps, reference, sample, col0, before, after, W, mode, positions):
    """(amplitude, weight, moment, best, location, channel) by the oracle on the whole recording."""
    cols = np.asarray(cols)
    p = np.asarray(positions, dtype=np.float32).reshape(cols.size, -1)
    amp, weight, moment, best = localize(x[:, cols], 0, 0, x.shape[0], [1.0] if taps is None else taps, 1 if reference else 0, sample, col0,
                                         before, after, W, MODES[mode], p)
    chan = np.where(best >= 0, cols[np.where(best >= 0, np.asarray(col0) + best, 0)], -1)
    return amp, weight, moment, best, location(moment, weight), chan


def _check(got, want):
    amp, weight, moment, best, loc, chan = want
    _same(got.amplitude, amp)
    _same(got.weight, weight)
    _same(got.moment, moment)
    _same(got.best, best)
    _same(got.location, loc)
    _same(got.channel, chan)


@pytest.mark.parametrize('reference', [None, 'median'])
def test_detect_then_localize_and_the_three_identities(tmp_cfg, reference):
    x = synth_int16(0, 3000, 70, 4)
    r = _write(tmp_cfg, x, _codec(), sample_rate=700.)
    ev = r.detect(12, taps=TAPS65, sign='neg', reference=reference, exclude=7, spread=3)
    assert ev.sample.size > 300
    pos = _grid(70)
    kw = dict(neighbours=8, taps=TAPS65, reference=reference)
    w = r.waveforms(ev.sample, ev.channel, **kw)
    got = {m: r.localize(ev.sample, pos, ev.channel, amplitude=m, **kw) for m in MODES}
    for m, g in got.items():
        assert g.location.shape == (ev.sample.size, 2) and g.amplitude.shape == (ev.sample.size, 17) and (g.before, g.after, g.mode) == (20, 41, m)
        assert g.positions.dtype == np.float32 and np.array_equal(g.positions, pos.astype(np.float32))
        assert np.array_equal(g.channels, np.arange(70)) and np.array_equal(g.sample, ev.sample) and np.array_equal(g.position, ev.channel - 8)
        # identity 1: the definition run on the host over Reader.waveforms' own snippets
        amp, weight, moment, best = reduce_snippets(w.waveforms, ev.channel - 8, pos.astype(np.float32), MODES[m])
        _same(g.amplitude, amp)
        _same(g.weight, weight)
        _same(g.moment, moment)
        _same(g.best, best)
        _same(g.location, location(moment, weight))
        _check(g, _want(x, np.arange(70), TAPS65, reference, ev.sample, ev.channel - 8, 20, 41, 17, m, pos))
        nan = np.isnan(g.amplitude)
        assert nan.any() and not nan.all()                              # events at the probe's edges; and none is empty
        assert (g.best >= 0).all() and np.array_equal(g.channel, ev.channel - 8 + g.best)
    # identity 2: the largest 'neg' amplitude is minus the trough, the largest 'pos' amplitude the peak
    assert (w.trough.index >= 0).all()
    _same(np.nanmax(got['neg'].amplitude, axis=1), -w.trough.value)
    _same(np.nanmax(got['pos'].amplitude, axis=1), w.peak.value)
    assert np.array_equal(got['neg'].channel, w.trough.channel) and np.array_equal(got['pos'].channel, w.peak.channel)
    # identity 3: the centre sample is one of the column's entries.  detect(sign='neg') returns the sample itself, z < 0, so the
    # amplitude is held to its size -z as well, and meets it where the crossing is the column's trough
    centre = got['neg'].amplitude[:, 8]
    assert (centre >= ev.amplitude).all() and (centre >= -ev.amplitude).all() and (centre == -ev.amplitude).sum() > 100
    # the spikes sit near their channel: the location lies inside the box of the snippet's positions
    g = got['ptp']
    ok = np.isfinite(g.weight) & (g.weight > 0)
    assert ok.all()
    assert (g.location[:, 0] >= 11.0).all() and (g.location[:, 0] <= 43.0).all()
    assert (np.abs(g.location[:, 1] - 20.0 * (ev.channel // 2)) <= 80.0).all()
    r.close()


@pytest.mark.parametrize('mode', sorted(MODES))
def test_location_is_within_the_derived_bound_of_the_float64_weighted_mean(tmp_cfg, mode):
    """|location - sum g p / sum g| <= (2 W + 2) u sum g |p| / sum g with u = 2^-24, wherever weight > 0 and finite.  Derived, not
    measured: the moment is a length-W fmaf chain, so it is off by at most gamma_W sum g |p| (gamma_k = k u / (1 - k u)); the weight is
    a length-W sum of terms >= 0 from +0 (its first step exact), off by at most gamma_(W-1) of itself, which moves the quotient by as
    much relative to |quotient| <= sum g |p| / sum g; the quotient is rounded to float64 and to float32, 2^-53 + u more.  To first
    order that is (2 W + 1) u; the one u left over covers the second-order terms (about (2 W)^2 u^2: 2e-3 u at W = 70) and the float64
    reference's own W 2^-53.  Nothing underflows here: the amplitudes come from int16 data and no position is subnormal."""
    x = synth_int16(0, 3000, 70, 4)
    r = _write(tmp_cfg, x, _codec(), sample_rate=700.)
    ev = r.detect(12, taps=TAPS65, sign='neg', exclude=7, spread=3)
    pos = _grid(70, 4)
    for neighbours, W in ((8, 17), (None, 70)):
        g = r.localize(ev.sample, pos, ev.channel, neighbours=neighbours, taps=TAPS65, amplitude=mode)
        a = g.amplitude.astype(np.float64)
        wgt = np.where(a > 0, a, 0.0)                                    # (NaN compares false)
        c = g.position[:, None] + np.arange(W)[None, :]
        inside = (c >= 0) & (c < 70)
        wgt = np.where(inside, wgt, 0.0)
        p = g.positions.astype(np.float64)[np.clip(c, 0, 69)]           # (n, W, D)
        ok = np.isfinite(g.weight) & (g.weight > 0)
        assert ok.sum() > 300
        num, den, scale = (wgt[:, :, None] * p).sum(axis=1), wgt.sum(axis=1), (wgt[:, :, None] * np.abs(p)).sum(axis=1)
        err = np.abs(g.location[ok].astype(np.float64) - num[ok] / den[ok, None])
        assert (err <= (2 * W + 2) * 2.0 ** -24 * scale[ok] / den[ok, None]).all()
    r.close()


def test_any_order_repeats_one_d_positions_and_full_width(tmp_cfg):
    x = synth_int16(0, 5000, 12, 4)
    codec = _codec()
    r = _write(tmp_cfg, x, codec)
    rs = np.random.RandomState(0)
    sample = rs.randint(0, 5000, 300)
    sample[:40] = sample[40:80]                                        # repeats, shuffled
    sample[[5, 17]] = [0, 4999]
    channel = rs.randint(0, 12, 300)
    pos = _grid(12, 3)
    for reference in (None, 'median'):
        for mode in ('ptp', 'abs'):
            kw = dict(before=7, after=12, taps=TAPS65, reference=reference, amplitude=mode)
            got = r.localize(sample, pos, channel, neighbours=2, **kw)
            assert got.amplitude.shape == (300, 5) and got.moment.shape == (300, 3) and got.best.dtype == np.int64 and got.channel.dtype == np.int64
            _check(got, _want(x, np.arange(12), TAPS65, reference, sample, channel - 2, 7, 12, 5, mode, pos))
            order = rs.permutation(300)
            again = r.localize(sample[order], pos, channel[order], neighbours=2, **kw)
            _same_bunch(again, got, order)
            whole = r.localize(sample, pos, **kw)
            assert whole.amplitude.shape == (300, 12) and not whole.position.any()
            _check(whole, _want(x, np.arange(12), TAPS65, reference, sample, np.zeros(300, int), 7, 12, 12, mode, pos))
            # 1-D positions: no D axis, the same bytes as the one-column positions
            one = r.localize(sample, pos[:, 1], channel, neighbours=2, **kw)
            col = r.localize(sample, pos[:, 1:2], channel, neighbours=2, **kw)
            assert one.location.shape == (300,) and one.moment.shape == (300,) and one.positions.shape == (12, 1) and col.location.shape == (300, 1)
            _same(one.location, col.location[:, 0])
            _same(one.moment, col.moment[:, 0])
            _same(one.amplitude, got.amplitude)
            # without the amplitudes: everything else is the same bytes
            bare = r.localize(sample, pos, channel, neighbours=2, amplitudes=False, **kw)
            assert bare.amplitude is None
            for name in FIELDS:
                if name != 'amplitude':
                    _same(bare[name], got[name])
    # float64 positions are rounded once, and the Bunch holds what was used; ints are taken
    p64 = np.random.RandomState(1).standard_normal((12, 2)) * 1e3 + 1e-7
    assert not np.array_equal(p64.astype(np.float32).astype(np.float64), p64)
    got = r.localize(sample, p64, before=7, after=12)
    assert got.positions.dtype == np.float32 and np.array_equal(got.positions, p64.astype(np.float32))
    _check(got, _want(x, np.arange(12), None, None, sample, np.zeros(300, int), 7, 12, 12, 'ptp', p64.astype(np.float32)))
    r.localize(sample, np.arange(12), before=7, after=12)
    # a shuffled channel list with repeats: positions follow the list, not the file
    cols = [7, 0, 0, 11, 3, 7, 5]
    ch = np.array(cols)[rs.randint(0, 7, 300)]
    first = np.array([cols.index(c) for c in ch])
    pos7 = _grid(7, 2)[::-1].copy()
    got = r.localize(sample, pos7, ch, before=3, after=4, neighbours=1, channels=cols, reference='median', amplitude='neg')
    assert np.array_equal(got.channels, cols)
    _check(got, _want(x, cols, None, 'median', sample, first - 1, 3, 4, 3, 'neg', pos7))
    # no events: no device call
    codec.localize_calls.clear()
    none = r.localize(np.zeros(0, np.int64), _grid(12), np.zeros(0, np.int64), neighbours=3)
    assert none.location.shape == (0, 2) and none.amplitude.shape == (0, 7) and none.amplitude.dtype == np.float32 and not codec.localize_calls
    assert none.weight.shape == (0,) and none.moment.shape == (0, 2) and none.best.shape == (0,) and none.channel.shape == (0,)
    assert r.localize(np.zeros(0, np.int64), np.arange(12.0)).location.shape == (0,)
    r.close()


def test_call_cuts_and_lanes_give_identical_bytes(tmp_cfg, monkeypatch):
    x = synth_int16(0, 9000, 8, 5)
    codec = _codec()
    one = _write(tmp_cfg, x, codec)
    rs = np.random.RandomState(2)
    sample, channel = rs.randint(0, 9000, 400), rs.randint(0, 8, 400)
    pos = _grid(8, 2)
    kw = dict(before=9, after=14, neighbours=3, taps=TAPS65, reference='median')
    whole = one.localize(sample, pos, channel, **kw)
    assert len(codec.localize_calls) == 1 and codec.localize_calls[0][3] == 400
    _check(whole, _want(x, np.arange(8), TAPS65, 'median', sample, channel - 3, 9, 14, 7, 'ptp', pos))
    for n_lanes in (2, 3):
        lc = _codec(n_lanes)
        many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=lc, check_after_decompress=False)
        _same_bunch(many.localize(sample, pos, channel, **kw), whole)
        assert {c[0] for c in lc.localize_calls} == set(range(n_lanes))
        assert sum(c[3] for c in lc.localize_calls) == 400
        for _, keys, _, _ in lc.localize_calls:                        # a lane reads adjacent chunks
            assert keys == list(range(keys[0], keys[-1] + 1))
        many.close()
    codec.localize_calls.clear()
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1)
    _same_bunch(one.localize(sample, pos, channel, **kw), whole)
    assert len(codec.localize_calls) >= 8 and sum(c[3] for c in codec.localize_calls) == 400
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1 << 30)
    codec.localize_calls.clear()
    monkeypatch.setattr(api, 'WAVEFORMS_OUT_BYTES', 30 * 4 * (7 + 2 + 2))    # 4 (W + D + 2) bytes an event: 30 events a call
    _same_bunch(one.localize(sample, pos, channel, **kw), whole)
    assert [c[3] for c in codec.localize_calls] == [30] * 13 + [10]
    one.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    x = synth_int16(0, 6000, 6, 7)
    codec = _codec()
    r = _write(tmp_cfg, x, codec)
    cache = r._cache_for(0)
    sample = np.arange(50, 6000, 97)
    pos = _grid(6)
    cold = r.localize(sample, pos, taps=TAPS65)
    assert not codec.caches[cache]                                     # a localization inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    assert resident
    codec.localize_calls.clear()
    warm = r.localize(sample, pos, taps=TAPS65)
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens, _), = codec.localize_calls
    assert [k for k, n in zip(keys, lens) if n == 0] == resident
    _same_bunch(warm, cold)
    # an entry dropped between the query and the call: E_MISS, then everything is sent once more
    codec.localize_calls.clear()
    codec.miss_next_localize = True
    _same_bunch(r.localize(sample, pos, taps=TAPS65), cold)
    (_, _, lens_a, _), (_, _, lens_b, _) = codec.localize_calls
    assert 0 in lens_a and all(lens_b)
    # a sparse list reads only its chunks
    codec.localize_calls.clear()
    r.localize([5400, 300], pos, taps=TAPS65)
    assert sorted(c[1] for c in codec.localize_calls) == [[0], [5]]
    r.close()


def test_a_spike_at_the_start_of_the_file_keeps_the_amplitudes_of_its_rows(tmp_cfg):
    x = synth_int16(0, 2000, 5, 3)
    r = _write(tmp_cfg, x, _codec())
    got = r.localize([0, 3, 1999], _grid(5), before=20, after=41)
    assert not np.isnan(got.amplitude).any() and (got.weight > 0).all() and np.isfinite(got.location).all()
    one = r.localize([1999], _grid(5), before=0, after=1)             # one row: every 'ptp' amplitude is hi - lo of a single entry
    assert (one.amplitude.view(np.uint32) == 0).all() and one.weight.view(np.uint32)[0] == 0 and (one.location.view(np.uint32) == FILL_BITS).all()
    assert one.best[0] == 0 and one.channel[0] == 0
    r.close()


def test_argument_errors(tmp_cfg):
    x = synth_int16(0, 2000, 5, 9)
    r = _write(tmp_cfg, x, _codec())
    ok = dict(sample=[10, 20], positions=_grid(5), channel=[0, 1], neighbours=1)
    r.localize(**ok)
    for bad in (dict(sample=[-1, 5]), dict(sample=[2000, 5]), dict(sample=[[1, 2]]), dict(sample=[1.0, 2.0]),
                dict(before=-1), dict(before=0, after=0), dict(before=4000, after=97), dict(after=True),
                dict(neighbours=-1), dict(neighbours=512), dict(channel=None), dict(channel=[0]), dict(channel=[0, 5]),
                dict(channels=[0, 2, 3]), dict(channels=[]), dict(reference='mean'), dict(taps=[]), dict(taps=[np.nan])):
        with pytest.raises(ValueError):
            r.localize(**{**ok, **bad})
    shape = r"positions must be a \(5, D\) or \(5,\) array of numbers, one row per selected channel, got shape "
    for bad, text in ((_grid(4), shape + r"\(4, 2\)"), (_grid(5).T, shape + r"\(2, 5\)"), (np.zeros((5, 2, 1)), shape), (np.float32(1.0), shape),
                      (None, shape), (np.zeros((5, 2), complex), shape), ([['a']] * 5, shape), (np.zeros(6), shape + r"\(6,\)"),
                      (np.zeros((5, 0)), "positions must have 1 to 4 coordinates a channel, got 0"),
                      (np.zeros((5, 5)), "positions must have 1 to 4 coordinates a channel, got 5")):
        with pytest.raises(ValueError, match=text):
            r.localize(**{**ok, 'positions': bad})
    # one row per entry of `channels`, not per file channel
    with pytest.raises(ValueError, match=r"positions must be a \(3, D\)"):
        r.localize([10], _grid(5), channels=[0, 2, 3])
    r.localize([10], _grid(3), channels=[0, 2, 3])
    r.localize([10], _grid(5, 4))
    for v in (np.nan, np.inf, -np.inf, 1e39):                           # 1e39 is finite as float64, inf as float32
        p = _grid(5).astype(np.float64)
        p[3, 1] = v
        with pytest.raises(ValueError, match="positions must be finite as float32"):
            r.localize(**{**ok, 'positions': p})
    for bad in ('PTP', 'both', '', None, 0, b'ptp', ['ptp']):
        with pytest.raises(ValueError, match="amplitude must be 'ptp', 'neg', 'pos' or 'abs', got"):
            r.localize(**{**ok, 'amplitude': bad})
    assert hip.LOCALIZE_MAX_DIMS == 4 and hip.LOCALIZE_MODES == MODES == {'ptp': 0, 'neg': 1, 'pos': 2, 'abs': 3}
    r.close()


def test_needs_a_device_codec(tmp_cfg):
    r = _write(tmp_cfg, synth_int16(0, 2000, 3, 0), OracleCodec())
    with pytest.raises(NotImplementedError):
        r.localize([10], _grid(3))
    r.close()


def test_exports_are_listed():
    assert {'mts_localize', 'mts_dev_localize'} <= set(hip.EXPORTS)
    assert callable(api.HipCodec.localize) and callable(hip.localize) and callable(hip.dev_localize)
