"""Reader.mean_waveforms, host side: argument handling, any order of the events, labels, call cutting, lanes, cache use and errors,
driven through a numpy restatement of mts_mean_waveforms (tests/mean_waveforms_oracle.py).  The kernel:
tests/test_gpu_mean_waveforms.py."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.mean_waveforms_oracle import MeanWaveformsOracleCodec, mean_of, mean_waveforms

TAPS65 = api.highpass_taps(300, 5000, 65)


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
    return MeanWaveformsOracleCodec(n_lanes=n_lanes, capacity_chunks=8)


def _same(a, b):
    for key, t in (('sum', np.int64), ('count', np.int64), ('skipped', np.int64), ('events', np.int64), ('mean', np.float32)):
        assert a[key].dtype == t and a[key].shape == b[key].shape, key
        assert a[key].tobytes() == b[key].tobytes(), key


def _want(x, cols, taps, reference, sample, col0, label, K, before, after, W, resolution=2.0 ** -16):
    """The Bunch Reader.mean_waveforms should return, from the definition."""
    sample, col0, label = np.asarray(sample), np.asarray(col0), np.asarray(label)
    keep = label >= 0
    total, count, skipped = mean_waveforms(x[:, np.asarray(cols)], 0, 0, x.shape[0], [1.0] if taps is None else taps, 1 if reference else 0,
                                           sample[keep], col0[keep], label[keep], K, before, after, W, resolution)
    return api.Bunch(sum=total, count=count.astype(np.int64), skipped=skipped, events=np.bincount(label[keep], minlength=K).astype(np.int64),
                     mean=mean_of(total, count, resolution))


@pytest.mark.parametrize('reference', [None, 'median'])
def test_base_case_is_the_sum_of_waveforms_snippets(tmp_cfg, reference):
    x = synth_int16(0, 3000, 70, 4)
    r = _write(tmp_cfg, x, _codec(), sample_rate=700.)
    ev = r.detect(12, taps=TAPS65, sign='neg', reference=reference, exclude=7, spread=3)
    label = ev.channel % 5
    got = r.mean_waveforms(ev.sample, label, ev.channel, neighbours=8, taps=TAPS65, reference=reference)
    assert got.mean.shape == (5, 61, 17) and (got.before, got.after, got.resolution) == (20, 41, 2.0 ** -16)
    assert np.array_equal(got.channels, np.arange(70)) and got.events.sum() == ev.sample.size
    _same(got, _want(x, np.arange(70), TAPS65, reference, ev.sample, ev.channel - 8, label, 5, 20, 41, 17))
    # identity: the same sums formed from Reader.waveforms' own snippets
    w = r.waveforms(ev.sample, ev.channel, neighbours=8, taps=TAPS65, reference=reference).waveforms
    t = ev.sample[:, None, None] - 20 + np.arange(61)[None, :, None]
    c = ev.channel[:, None, None] - 8 + np.arange(17)[None, None, :]
    inside = np.broadcast_to((t >= 0) & (t < 3000) & (c >= 0) & (c < 70), w.shape)
    assert not inside.all() and np.array_equal(np.isnan(w), ~inside)
    q = np.rint(w.astype(np.float64) / got.resolution)
    total, count = np.zeros((5, 61, 17), np.int64), np.zeros((5, 61, 17), np.int64)
    e, tau, pos = np.nonzero(inside)
    np.add.at(total, (label[e], tau, pos), q[inside].astype(np.int64))
    np.add.at(count, (label[e], tau, pos), 1)
    assert got.sum.tobytes() == total.tobytes() and got.count.tobytes() == count.tobytes() and not got.skipped.any()
    # the mean is the float mean of the snippets to the resolution
    plain = np.array([np.nanmean(np.where(inside, w, np.nan)[label == k].astype(np.float64), axis=0) for k in range(5)])
    assert np.abs(got.mean - plain).max() <= 2.0 ** -17 + np.abs(plain).max() * 2.0 ** -23
    r.close()


def test_any_order_negative_labels_default_n_labels_and_full_width(tmp_cfg):
    x = synth_int16(0, 5000, 12, 4)
    codec = _codec()
    r = _write(tmp_cfg, x, codec)
    rs = np.random.RandomState(0)
    sample = rs.randint(0, 5000, 300)
    sample[:40] = sample[40:80]                                        # repeats, shuffled
    sample[[5, 17]] = [0, 4999]
    channel = rs.randint(0, 12, 300)
    label = rs.randint(-2, 6, 300)                                     # -2 and -1: ignored
    label[[5, 17]] = [0, 5]
    assert (label < 0).sum() > 20
    for reference in (None, 'median'):
        got = r.mean_waveforms(sample, label, channel, before=7, after=12, neighbours=2, taps=TAPS65, reference=reference)
        assert got.mean.shape == (6, 19, 5)                            # n_labels=None: max(label) + 1
        _same(got, _want(x, np.arange(12), TAPS65, reference, sample, channel - 2, label, 6, 7, 12, 5))
        order = rs.permutation(300)
        _same(r.mean_waveforms(sample[order], label[order], channel[order], before=7, after=12, neighbours=2, taps=TAPS65, reference=reference), got)
        whole = r.mean_waveforms(sample, label, before=7, after=12, taps=TAPS65, reference=reference, n_labels=9, resolution=0.25)
        assert whole.mean.shape == (9, 19, 12) and whole.events[6:].tolist() == [0, 0, 0] and np.isnan(whole.mean[6:]).all()
        _same(whole, _want(x, np.arange(12), TAPS65, reference, sample, np.zeros(300, int), label, 9, 7, 12, 12, 0.25))
    # with neighbours=None, np.nan_to_num(mean) is a `templates` argument
    tpl = np.nan_to_num(whole.mean)
    assert tpl.shape == (9, 19, 12) and tpl.dtype == np.float32 and np.isfinite(tpl).all()
    # a shuffled channel list with repeats
    cols = [7, 0, 0, 11, 3, 7, 5]
    ch = np.array(cols)[rs.randint(0, 7, 300)]
    first = np.array([cols.index(c) for c in ch])
    got = r.mean_waveforms(sample, label, ch, before=3, after=4, neighbours=1, channels=cols, reference='median')
    assert np.array_equal(got.channels, cols)
    _same(got, _want(x, cols, None, 'median', sample, first - 1, label, 6, 3, 4, 3))
    # no events, only ignored events, n_labels=0: no device call
    codec.mean_waveforms_calls.clear()
    none = r.mean_waveforms(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), neighbours=3)
    assert none.mean.shape == (0, 61, 7) and none.sum.dtype == np.int64 and none.events.shape == (0,)
    none = r.mean_waveforms([5, 9], [-1, -1], n_labels=3)
    assert none.mean.shape == (3, 61, 12) and np.isnan(none.mean).all() and not none.count.any() and none.events.tolist() == [0, 0, 0]
    assert r.mean_waveforms([5, 9], [-1, -3]).mean.shape == (0, 61, 12) and not codec.mean_waveforms_calls
    r.close()


def test_call_cuts_and_lanes_give_identical_bytes(tmp_cfg, monkeypatch):
    x = synth_int16(0, 9000, 8, 5)
    codec = _codec()
    one = _write(tmp_cfg, x, codec)
    rs = np.random.RandomState(2)
    sample, channel, label = rs.randint(0, 9000, 400), rs.randint(0, 8, 400), rs.randint(-1, 7, 400)
    n = int((label >= 0).sum())
    kw = dict(before=9, after=14, neighbours=3, taps=TAPS65, reference='median')
    whole = one.mean_waveforms(sample, label, channel, **kw)
    assert len(codec.mean_waveforms_calls) == 1 and codec.mean_waveforms_calls[0][3] == n
    _same(whole, _want(x, np.arange(8), TAPS65, 'median', sample, channel - 3, label, 7, 9, 14, 7))
    for n_lanes in (2, 3):
        lc = _codec(n_lanes)
        many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=lc, check_after_decompress=False)
        _same(many.mean_waveforms(sample, label, channel, **kw), whole)
        assert {c[0] for c in lc.mean_waveforms_calls} == set(range(n_lanes))
        assert sum(c[3] for c in lc.mean_waveforms_calls) == n
        for _, keys, _, _ in lc.mean_waveforms_calls:                  # a lane reads adjacent chunks
            assert keys == list(range(keys[0], keys[-1] + 1))
        many.close()
    codec.mean_waveforms_calls.clear()
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1)
    _same(one.mean_waveforms(sample, label, channel, **kw), whole)
    assert len(codec.mean_waveforms_calls) >= 8 and sum(c[3] for c in codec.mean_waveforms_calls) == n
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1 << 30)
    codec.mean_waveforms_calls.clear()
    monkeypatch.setattr(api, 'MEAN_WAVEFORMS_EVENT_BYTES', 30 * 24)
    _same(one.mean_waveforms(sample, label, channel, **kw), whole)
    assert [c[3] for c in codec.mean_waveforms_calls] == [30] * (n // 30) + ([n % 30] if n % 30 else [])
    one.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    x = synth_int16(0, 6000, 6, 7)
    codec = _codec()
    r = _write(tmp_cfg, x, codec)
    cache = r._cache_for(0)
    sample = np.arange(50, 6000, 97)
    label = sample % 3
    cold = r.mean_waveforms(sample, label, taps=TAPS65)
    assert not codec.caches[cache]                                     # a sum inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    assert resident
    codec.mean_waveforms_calls.clear()
    warm = r.mean_waveforms(sample, label, taps=TAPS65)
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens, _), = codec.mean_waveforms_calls
    assert [k for k, n in zip(keys, lens) if n == 0] == resident
    _same(warm, cold)
    # an entry dropped between the query and the call: E_MISS, then everything is sent once more
    codec.mean_waveforms_calls.clear()
    codec.miss_next_mean_waveforms = True
    _same(r.mean_waveforms(sample, label, taps=TAPS65), cold)
    (_, _, lens_a, _), (_, _, lens_b, _) = codec.mean_waveforms_calls
    assert 0 in lens_a and all(lens_b)
    # a sparse list reads only its chunks
    codec.mean_waveforms_calls.clear()
    r.mean_waveforms([5400, 300], [0, 1], taps=TAPS65)
    assert sorted(c[1] for c in codec.mean_waveforms_calls) == [[0], [5]]
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
    r.mean_waveforms([300, 5400], [0, 0], taps=TAPS65)                 # chunks 0 and 5: chunk 3 is not read
    with pytest.raises(IOError, match='#3'):
        r.mean_waveforms([300, 3500], [0, 1])
    r.close()


def test_argument_errors(tmp_cfg, monkeypatch):
    x = synth_int16(0, 2000, 5, 9)
    r = _write(tmp_cfg, x, _codec())
    ok = dict(sample=[10, 20], label=[0, 1], channel=[0, 1], neighbours=1)
    r.mean_waveforms(**ok)
    for bad in (dict(sample=[-1, 5]), dict(sample=[2000, 5]), dict(sample=[[1, 2]]), dict(sample=[1.0, 2.0]),
                dict(before=-1), dict(before=0, after=0), dict(before=4000, after=97), dict(after=True),
                dict(neighbours=-1), dict(neighbours=512), dict(channel=None), dict(channel=[0]), dict(channel=[0, 5]),
                dict(channels=[0, 2, 3]), dict(channels=[]), dict(reference='mean'), dict(taps=[]), dict(taps=[np.nan]),
                dict(label=[0]), dict(label=[0.0, 1.0]), dict(label=[[0, 1]]), dict(label=None), dict(label=[0, 2], n_labels=2),
                dict(n_labels=-1), dict(n_labels=1.5), dict(n_labels=True), dict(n_labels=hip.MEAN_MAX_LABELS + 1),
                dict(label=[0, hip.MEAN_MAX_LABELS]),
                dict(n_labels=4096, neighbours=300, before=30, after=30),          # 4096 * 60 * 601 > 2^27
                dict(resolution=3.0), dict(resolution=0), dict(resolution=-1.0), dict(resolution=2.0 ** 61), dict(resolution=2.0 ** -61),
                dict(resolution=float('nan')), dict(resolution=float('inf')), dict(resolution='1'), dict(resolution=True)):
        with pytest.raises(ValueError):
            r.mean_waveforms(**{**ok, **bad})
    for good in (dict(resolution=2.0 ** 60), dict(resolution=2.0 ** -60), dict(resolution=1), dict(n_labels=hip.MEAN_MAX_LABELS)):
        r.mean_waveforms(**{**ok, **good})
    assert (hip.MEAN_MAX_LABELS, hip.MEAN_MAX_ENTRIES, hip.MEAN_MAX_LABEL_EVENTS) == (4096, 1 << 27, 1 << 21)
    # a label with more than 2^21 events in all (the limit lowered: the check is on the whole list, not on a call's share)
    monkeypatch.setattr(hip, 'MEAN_MAX_LABEL_EVENTS', 3)
    r.mean_waveforms([1, 2, 3, 4, 5, 6, 7], [0, 0, 0, 1, 1, 1, -1])
    with pytest.raises(ValueError, match='label 1 has 4 events'):
        r.mean_waveforms([1, 2, 3, 4, 5, 6, 7], [0, 0, 0, 1, 1, 1, 1])
    r.close()


def test_needs_a_device_codec(tmp_cfg):
    r = _write(tmp_cfg, synth_int16(0, 2000, 3, 0), OracleCodec())
    with pytest.raises(NotImplementedError):
        r.mean_waveforms([10], [0])
    r.close()


def test_exports_are_listed():
    assert {'mts_mean_waveforms', 'mts_dev_mean_waveforms'} <= set(hip.EXPORTS)
    assert callable(api.HipCodec.mean_waveforms) and callable(hip.mean_waveforms) and callable(hip.dev_mean_waveforms)
