"""Reader.waveforms, host side: argument handling, the caller's order, neighbourhoods, call cutting, lanes, cache use and errors,
driven through a numpy restatement of mts_waveforms (tests/waveforms_oracle.py).  The kernel: tests/test_gpu_waveforms.py."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.waveforms_oracle import BASE_COUNTS, FILL, WaveformsOracleCodec, edge_counts, waveforms


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
    return WaveformsOracleCodec(n_lanes=n_lanes, capacity_chunks=8)


def _same(a, b):
    assert (a.waveforms is None) == (b.waveforms is None)
    if a.waveforms is not None:
        assert a.waveforms.dtype == np.float32 and a.waveforms.shape == b.waveforms.shape
        assert a.waveforms.tobytes() == b.waveforms.tobytes()
    for which in ('trough', 'peak'):
        for key in ('value', 'offset', 'channel', 'index'):
            assert a[which][key].dtype == (np.float32 if key == 'value' else np.int64), (which, key)
            assert a[which][key].tobytes() == b[which][key].tobytes(), (which, key)


def _want(x, cols, taps, reference, sample, col0, before, after, W):
    """The Bunch Reader.waveforms should return, from the definition."""
    cols = np.asarray(cols)
    wave, vmin, amin, vmax, amax = waveforms(x[:, cols], 0, 0, x.shape[0], [1.0] if taps is None else taps, 1 if reference else 0, sample, col0,
                                             before, after, W)
    out = {}
    for name, v, i in (('trough', vmin, amin), ('peak', vmax, amax)):
        some = i >= 0
        out[name] = api.Bunch(value=v, offset=np.where(some, i // W - before, 0), index=i,
                              channel=np.where(some, cols[np.where(some, np.asarray(col0) + i % W, 0)], -1))
    return api.Bunch(waveforms=wave, trough=out['trough'], peak=out['peak'])


TAPS65 = api.highpass_taps(300, 5000, 65)


@pytest.mark.parametrize('reference', [None, 'median'])
def test_base_case_centre_sample_is_detects_amplitude(tmp_cfg, reference):
    x = synth_int16(0, 3000, 70, 4)
    r = _write(tmp_cfg, x, _codec(), sample_rate=700.)
    ev = r.detect(12, taps=TAPS65, sign='neg', reference=reference, exclude=7, spread=3)
    got = r.waveforms(ev.sample, ev.channel, neighbours=8, taps=TAPS65, reference=reference)
    assert edge_counts(got.sample, got.position, 20, 41, 17, 3000, 70) == BASE_COUNTS[1 if reference else 0]
    assert got.waveforms.shape == (ev.sample.size, 61, 17) and (got.before, got.after) == (20, 41)
    assert np.array_equal(got.position, ev.channel - 8) and np.array_equal(got.sample, ev.sample)
    assert got.waveforms[np.arange(ev.sample.size), 20, 8].tobytes() == ev.amplitude.tobytes()
    _same(got, _want(x, np.arange(70), TAPS65, reference, ev.sample, ev.channel - 8, 20, 41, 17))
    # fill entries are the quiet NaN, and exactly the entries outside the recording or the selection
    t = ev.sample[:, None, None] - 20 + np.arange(61)[None, :, None]
    c = got.position[:, None, None] + np.arange(17)[None, None, :]
    outside = (t < 0) | (t >= 3000) | (c < 0) | (c >= 70)
    assert outside.any() and np.array_equal(np.isnan(got.waveforms), outside | np.zeros_like(got.waveforms, bool))
    assert set(got.waveforms[outside].view(np.uint32).tolist()) == {0x7fc00000}
    # the trough of a negative-going event is at least as deep as its centre sample
    assert (got.trough.value <= ev.amplitude).all() and (got.trough.index >= 0).all()
    assert np.array_equal(got.waveforms.reshape(ev.sample.size, -1)[np.arange(ev.sample.size), got.peak.index], got.peak.value)
    r.close()


def test_callers_order_repeats_and_both_neighbourhoods(tmp_cfg):
    x = synth_int16(0, 5000, 12, 4)
    codec = _codec()
    r = _write(tmp_cfg, x, codec)
    rs = np.random.RandomState(0)
    sample = rs.randint(0, 5000, 300)
    sample[:40] = sample[40:80]                                        # repeats, shuffled
    sample[[5, 17]] = [0, 4999]
    channel = rs.randint(0, 12, 300)
    for reference in (None, 'median'):
        got = r.waveforms(sample, channel, before=7, after=12, neighbours=2, taps=TAPS65, reference=reference)
        _same(got, _want(x, np.arange(12), TAPS65, reference, sample, channel - 2, 7, 12, 5))
        assert np.array_equal(got.sample, sample) and np.array_equal(got.position, channel - 2)
        whole = r.waveforms(sample, before=7, after=12, taps=TAPS65, reference=reference)           # neighbours=None: every column
        assert whole.waveforms.shape == (300, 19, 12) and not whole.position.any()
        _same(whole, _want(x, np.arange(12), TAPS65, reference, sample, np.zeros(300, int), 7, 12, 12))
        assert np.array_equal(whole.waveforms[np.arange(300)[:, None, None], np.arange(19)[None, :, None],
                                              np.clip(got.position[:, None, None] + np.arange(5), 0, 11)][~np.isnan(got.waveforms)],
                              got.waveforms[~np.isnan(got.waveforms)])
    # a shuffled channel list with repeats: `channel` holds file channels, the position is the first that holds it
    cols = [7, 0, 0, 11, 3, 7, 5]
    ch = np.array(cols)[rs.randint(0, 7, 300)]
    first = np.array([cols.index(c) for c in ch])
    got = r.waveforms(sample, ch, before=3, after=4, neighbours=1, channels=cols, reference='median')
    assert np.array_equal(got.position, first - 1) and np.array_equal(got.channels, cols)
    _same(got, _want(x, cols, None, 'median', sample, first - 1, 3, 4, 3))
    assert set(np.unique(got.trough.channel)) <= set(cols)
    # neighbours=0: one column; an int channel selection; (0, 1) and (1, 0) snippets
    got = r.waveforms(sample, np.full(300, 5), before=0, after=1, neighbours=0, channels=5)
    assert got.waveforms.shape == (300, 1, 1) and np.array_equal(got.waveforms[:, 0, 0], x[sample, 5].astype(np.float32))
    assert np.array_equal(got.trough.value, got.peak.value) and not got.trough.offset.any() and set(got.peak.channel) == {5}
    got = r.waveforms(sample, before=1, after=0, channels=[5])
    want = np.where(sample > 0, x[np.maximum(sample - 1, 0), 5], np.nan).astype(np.float32)
    assert got.waveforms[:, 0, 0].tobytes() == np.where(sample > 0, want, FILL).astype(np.float32).tobytes()
    assert got.trough.index[5] == -1 and got.trough.channel[5] == -1 and got.trough.offset[5] == 0 and np.isnan(got.peak.value[5])
    assert (got.trough.offset[sample > 0] == -1).all()
    # no events: no device call
    codec.waveforms_calls.clear()
    none = r.waveforms(np.zeros(0, np.int64), np.zeros(0, np.int64), neighbours=3)
    assert none.waveforms.shape == (0, 61, 7) and none.trough.value.shape == (0,) and none.peak.index.dtype == np.int64
    assert r.waveforms([], waveforms=False).waveforms is None and not codec.waveforms_calls
    r.close()


def test_waveforms_false_gives_the_same_extrema(tmp_cfg):
    x = synth_int16(0, 4000, 20, 3)
    r = _write(tmp_cfg, x, _codec())
    rs = np.random.RandomState(1)
    sample, channel = rs.randint(0, 4000, 200), rs.randint(0, 20, 200)
    full = r.waveforms(sample, channel, neighbours=4, taps=TAPS65, reference='median')
    bare = r.waveforms(sample, channel, neighbours=4, taps=TAPS65, reference='median', waveforms=False)
    assert bare.waveforms is None
    bare.waveforms = full.waveforms
    _same(bare, full)
    r.close()


def test_call_cuts_lanes_give_identical_bytes(tmp_cfg, monkeypatch):
    x = synth_int16(0, 9000, 8, 5)
    codec = _codec()
    one = _write(tmp_cfg, x, codec)
    rs = np.random.RandomState(2)
    sample, channel = rs.randint(0, 9000, 400), rs.randint(0, 8, 400)
    kw = dict(before=9, after=14, neighbours=3, taps=TAPS65, reference='median')
    whole = one.waveforms(sample, channel, **kw)
    assert len(codec.waveforms_calls) == 1
    _same(whole, _want(x, np.arange(8), TAPS65, 'median', sample, channel - 3, 9, 14, 7))
    for n_lanes in (2, 3):
        lc = _codec(n_lanes)
        many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=lc, check_after_decompress=False)
        _same(many.waveforms(sample, channel, **kw), whole)
        assert {c[0] for c in lc.waveforms_calls} == set(range(n_lanes))
        assert sum(c[3] for c in lc.waveforms_calls) == 400
        for _, keys, _, _ in lc.waveforms_calls:                       # a lane reads adjacent chunks
            assert keys == list(range(keys[0], keys[-1] + 1))
        many.close()
    codec.waveforms_calls.clear()
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1)
    _same(one.waveforms(sample, channel, **kw), whole)
    assert len(codec.waveforms_calls) >= 8 and sum(c[3] for c in codec.waveforms_calls) == 400
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1 << 30)
    codec.waveforms_calls.clear()
    monkeypatch.setattr(api, 'WAVEFORMS_OUT_BYTES', 30 * (4 * 23 * 7 + 16))
    _same(one.waveforms(sample, channel, **kw), whole)
    assert [c[3] for c in codec.waveforms_calls] == [30] * 13 + [10]
    one.close()


def test_a_sparse_list_reads_only_its_chunks(tmp_cfg):
    x = synth_int16(0, 8000, 6, 7)
    codec = _codec()
    r = _write(tmp_cfg, x, codec)
    assert r.n_chunks == 8
    sample = np.array([5400, 300, 5100, 700, 5999, 0])                 # chunks 0 and 5
    got = r.waveforms(sample, before=20, after=41, taps=TAPS65)
    _same(got, _want(x, np.arange(6), TAPS65, None, sample, np.zeros(6, int), 20, 41, 6))
    assert sorted(c[1] for c in codec.waveforms_calls) == [[0], [5, 6]]      # (5999 + 41 + 32 reaches chunk 6)
    assert not any(k in c[1] for c in codec.waveforms_calls for k in (2, 3))
    # chunks 0 and 2: one whole chunk between them is unread -> two calls; 0 and 1: one call
    codec.waveforms_calls.clear()
    r.waveforms([500, 2500], taps=TAPS65)
    assert sorted(c[1] for c in codec.waveforms_calls) == [[0], [2]]
    codec.waveforms_calls.clear()
    r.waveforms([500, 1500], taps=TAPS65)
    assert [c[1] for c in codec.waveforms_calls] == [[0, 1]]
    codec.waveforms_calls.clear()
    r.waveforms([990, 2010], taps=TAPS65)                              # the supports meet in chunk 1
    assert [c[1] for c in codec.waveforms_calls] == [[0, 1, 2]]
    r.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    x = synth_int16(0, 6000, 6, 7)
    codec = _codec()
    r = _write(tmp_cfg, x, codec)
    cache = r._cache_for(0)
    sample = np.arange(50, 6000, 97)
    cold = r.waveforms(sample, taps=TAPS65)
    assert not codec.caches[cache]                                     # a gather inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    assert resident
    codec.waveforms_calls.clear()
    warm = r.waveforms(sample, taps=TAPS65)
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens, _), = codec.waveforms_calls
    assert [k for k, n in zip(keys, lens) if n == 0] == resident
    _same(warm, cold)
    # an entry dropped between the query and the call: E_MISS, then everything is sent once more
    codec.waveforms_calls.clear()
    codec.miss_next_waveforms = True
    _same(r.waveforms(sample, taps=TAPS65), cold)
    (_, _, lens_a, _), (_, _, lens_b, _) = codec.waveforms_calls
    assert 0 in lens_a and all(lens_b)
    r.close()


def test_damaged_chunk_in_the_support_raises(tmp_cfg):
    x = synth_int16(0, 8000, 4, 8)
    codec = _codec(2)
    r = _write(tmp_cfg, x, codec)
    r.close()
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    ch = r.chunk_offsets
    data[ch[3] + 20:ch[3] + 40] = b'\xff' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    r.waveforms([300, 5400], taps=TAPS65)                              # chunks 0 and 5: chunk 3 is not read
    with pytest.raises(IOError, match='#3'):
        r.waveforms([300, 3500])
    with pytest.raises(IOError, match='#3'):
        r.waveforms([2940], taps=TAPS65)                               # 2940 + 41 + 32 > 3000: the filter support alone
    r.waveforms([2940 - 14], taps=TAPS65)
    r.close()


def test_argument_errors(tmp_cfg):
    x = synth_int16(0, 2000, 5, 9)
    r = _write(tmp_cfg, x, _codec())
    ok = dict(sample=[10, 20], channel=[0, 1], neighbours=1)
    r.waveforms(**ok)
    for bad in (dict(sample=[-1, 5]), dict(sample=[2000, 5]), dict(sample=[[1, 2]]), dict(sample=[1.0, 2.0]), dict(sample='ab'),
                dict(before=-1), dict(after=-1), dict(before=0, after=0), dict(before=4000, after=97), dict(before=1.0), dict(after=True),
                dict(neighbours=-1), dict(neighbours=1.5), dict(neighbours=True), dict(neighbours=512), dict(channel=None), dict(channel=[0]),
                dict(channel=[0, 5]), dict(channel=[0, -1]), dict(channel=[0.0, 1.0]), dict(channels=[0, 2, 3]), dict(channels=[]),
                dict(reference='mean'), dict(reference=1), dict(taps=[]), dict(taps=[np.nan]), dict(taps=np.ones(8193))):
        with pytest.raises(ValueError):
            r.waveforms(**{**ok, **bad})
    with pytest.raises(IndexError):
        r.waveforms([10], channels=5)
    assert (hip.WAVEFORMS_MAX_ROWS, hip.WAVEFORMS_MAX_WIDTH) == (4096, 1024)
    assert r.waveforms([10], before=4000, after=96, waveforms=False).trough.index[0] >= 0
    assert r.waveforms([10], [0], neighbours=511).waveforms.shape == (1, 61, 1023)
    r.close()
    wide = np.zeros((10, hip.DETECT_MAX_REF_COLS + 1), np.int16)
    r = _write(tmp_cfg, wide, _codec())
    for kw in (dict(reference='median'), dict()):                      # too many columns for a median; too wide a snippet
        with pytest.raises(ValueError):
            r.waveforms([3], **kw)
    assert r.waveforms([3], channels=slice(0, 1024), reference='median').waveforms.shape == (1, 61, 1024)
    r.close()


def test_needs_a_device_codec(tmp_cfg):
    r = _write(tmp_cfg, synth_int16(0, 2000, 3, 0), OracleCodec())
    with pytest.raises(NotImplementedError):
        r.waveforms([10])
    r.close()


def test_exports_are_listed():
    assert {'mts_waveforms', 'mts_dev_waveforms'} <= set(hip.EXPORTS)
    assert callable(api.HipCodec.waveforms) and callable(hip.waveforms) and callable(hip.dev_waveforms)
