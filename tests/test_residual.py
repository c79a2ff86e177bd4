"""Reader.residual and Reader.match_templates(subtract=), host side: argument handling, the order of the events, call cutting and the
events each call is handed, lanes, cache use and errors, driven through a numpy restatement of mts_residual and mts_match_residual
(tests/residual_oracle.py), and one exact two-pass peel.  The kernel: tests/test_gpu_residual.py."""
import re
from pathlib import Path

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.correlate_oracle import correlate, reference_rows
from tests.residual_oracle import ResidualOracleCodec, match_residual, residual
from tests.tmatch_oracle import TmatchOracleCodec, match_templates

ROOT = Path(__file__).resolve().parent.parent


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
    return ResidualOracleCodec(n_lanes=n_lanes, capacity_chunks=8)


def _events(ev):
    return ev.sample.tobytes(), ev.template.tobytes(), ev.score.tobytes()


TAPS33 = api.highpass_taps(300, 5000, 33)
X = synth_int16(0, 5000, 6, 4)                                         # five chunks of 1000 rows
K3 = np.random.RandomState(0).randn(3, 9, 6)
_rs = np.random.RandomState(7)
# 60 events with repeats and ties, some at the very ends and some astride every chunk boundary
EV = (np.concatenate([_rs.randint(0, 5000, 44), [0, 0, 4999, 4999, 998, 1000, 1003, 2001, 2001, 2996, 3999, 4000, 1500, 1500, 1500, 1502]]),
      _rs.randint(0, 3, 60), (_rs.randn(60) * 3).astype(np.float32))
CASES = ((TAPS33, 'median', 4), (None, None, 0), (None, 'median', 9))


def _want(taps, reference, before, i0, i1, ev=EV, cols=range(6), k=K3):
    return residual(X[:, np.asarray(cols)], 0, 0, 5000, i0, i1, [1.0] if taps is None else taps, 1 if reference else 0, before, k, *ev)


def test_residual_is_the_definition_and_stitches(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    for taps, reference, before in CASES:
        kw = dict(taps=taps, reference=reference, before=before)
        whole = r.residual(*EV, K3, **kw)
        assert whole.dtype == np.float32 and whole.shape == (5000, 6)
        assert whole.tobytes() == _want(taps, reference, before, 0, 5000).tobytes()
        for a, b, c in ((0, 1234, 5000), (990, 1000, 1010), (4990, 4999, 5000)):
            both = np.concatenate([r.residual(*EV, K3, a, b, **kw), r.residual(*EV, K3, b, c, **kw)])
            assert both.tobytes() == whole[a:c].tobytes()
        # an empty list is z: the referenced, filtered rows (correlate's z), a NaN as 0x7fc00000
        z = reference_rows(X, 0, 0, 5000, 0, 5000, [1.0] if taps is None else taps, 1 if reference else 0)
        assert r.residual([], [], [], K3, **kw).tobytes() == z.tobytes() != whole.tobytes()
    # a 2-D template is one template; channels choose and order the columns
    one = r.residual([100, 150], [0, 0], [1.0, -2.0], K3[1], 90, 170, before=4)
    assert one.tobytes() == r.residual([100, 150], [0, 0], [1.0, -2.0], K3[1:2], 90, 170, before=4).tobytes()
    cols = [5, 0, 0, 3]
    got = r.residual(*EV, K3[:, :, :4], 40, 1090, channels=cols, reference='median', before=2)
    assert got.tobytes() == _want(None, 'median', 2, 40, 1090, cols=cols, k=K3[:, :, :4]).tobytes()
    # an empty range: no device call
    codec.residual_calls.clear()
    assert r.residual(*EV, K3, 700, 700, before=0).shape == (0, 6) and r.residual(*EV, K3, 9, 3, before=9).shape == (0, 6)
    assert not codec.residual_calls
    r.close()


def test_order_of_the_events(tmp_cfg):
    r = _write(tmp_cfg, X, _codec())
    # distinct samples: any order of the list is the sorted one
    s = np.random.RandomState(1).permutation(5000)[:50]
    t, a = EV[1][:50], EV[2][:50]
    want = r.residual(np.sort(s), t[np.argsort(s)], a[np.argsort(s)], K3, before=4)
    p = np.random.RandomState(2).permutation(50)
    assert r.residual(s[p], t[p], a[p], K3, before=4).tobytes() == want.tobytes()
    ev = r.match_templates(K3, 50.0, before=4, subtract=(np.sort(s), t[np.argsort(s)], a[np.argsort(s)]))
    assert ev.sample.size and _events(r.match_templates(K3, 50.0, before=4, subtract=(s[p], t[p], a[p]))) == _events(ev)
    # equal samples keep the order of the list: 1 - 1e8 - 5 is not 1 - 5 - 1e8 in float32
    ones = np.ones((2, 1, 6))
    x1 = np.ones((5000, 6), np.int16)
    r.close()
    r = _write(tmp_cfg, x1, _codec())
    one = r.residual([7, 5, 5], [0, 0, 1], [2.0, 1e8, 5.0], ones, 0, 10, before=0)
    two = r.residual([7, 5, 5], [0, 1, 0], [2.0, 5.0, 1e8], ones, 0, 10, before=0)
    assert one[5].tolist() == [-100000008.0] * 6 and two[5].tolist() == [-100000000.0] * 6 and one[7].tolist() == [-1.0] * 6
    assert np.delete(one, [5, 7], axis=0).tolist() == [[1.0] * 6] * 8
    r.close()


def test_match_templates_subtract_is_the_definition_and_stitches(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    for taps, reference, before in CASES:
        t = [1.0] if taps is None else taps
        thr = np.percentile(correlate(X, 0, 0, 5000, 0, 5000, t, 1 if reference else 0, before, K3.astype(np.float32)), 90, axis=0).astype(np.float32)
        for R in (0, 3, None):
            kw = dict(taps=taps, reference=reference, before=before, exclude=R, subtract=EV)
            whole = r.match_templates(K3, thr, **kw)
            want = match_residual(X, 0, 0, 5000, 0, 5000, t, 1 if reference else 0, before, K3, thr, whole.exclude, *EV)
            assert whole.sample.size and _events(whole) == tuple(v.tobytes() for v in want)
            assert _events(whole) != _events(r.match_templates(K3, thr, **{**kw, 'subtract': None}))
            # the scores are correlate's chain on the residual
            for a, b, c in ((0, 1234, 5000), (990, 1000, 1010), (4990, 4999, 5000)):
                left, right = r.match_templates(K3, thr, a, b, **kw), r.match_templates(K3, thr, b, c, **kw)
                sel = (whole.sample >= a) & (whole.sample < c)
                for name in ('sample', 'template', 'score'):
                    assert np.concatenate([left[name], right[name]]).tobytes() == whole[name][sel].tobytes()
    # an empty list is match_templates itself, through the other entry
    codec.match_templates_calls.clear()
    codec.match_residual_calls.clear()
    assert _events(r.match_templates(K3, 40.0, before=4, subtract=([], [], []))) == _events(r.match_templates(K3, 40.0, before=4))
    assert len(codec.match_templates_calls) == 1 and len(codec.match_residual_calls) == 1
    r.close()


def test_subtract_none_makes_the_calls_it_made(tmp_cfg, monkeypatch):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    monkeypatch.setattr(api, 'TMATCH_GUESS_MIN', 10)
    monkeypatch.setattr(api, 'TMATCH_GUESS_SAMPLES', 1000)
    r.match_templates(K3, -3e38, 100, 4100, before=4, exclude=0)
    plain = list(codec.match_templates_calls)
    codec.match_templates_calls.clear()
    r.match_templates(K3, -3e38, 100, 4100, before=4, exclude=0, subtract=None)
    assert codec.match_templates_calls == plain and [c[5] for c in plain] == [10, 4000] and not codec.match_residual_calls
    # ... and with a list the same calls go to match_residual, the short buffer's second call included, each with its events
    r.match_templates(K3, -3e38, 100, 4100, before=4, exclude=0, subtract=EV)
    assert [c[:6] for c in codec.match_residual_calls] == plain
    assert codec.match_residual_calls[0][6] == codec.match_residual_calls[1][6] == sorted(s for s in EV[0].tolist() if 100 - 8 <= s < 4100 + 8)
    r.close()
    # a codec without match_residual still matches without a list
    old = _write(tmp_cfg, X, TmatchOracleCodec(n_lanes=1, capacity_chunks=8))
    assert old.match_templates(K3, 1e9, before=4, subtract=None).sample.size == 0
    with pytest.raises(NotImplementedError):
        old.match_templates(K3, 1e9, before=4, subtract=EV)
    with pytest.raises(NotImplementedError):
        old.residual(*EV, K3, before=4)
    old.close()
    none = _write(tmp_cfg, X, OracleCodec())
    with pytest.raises(NotImplementedError):
        none.residual(*EV, K3, before=4)
    none.close()


def test_lanes_and_call_cuts_give_identical_bytes_and_every_call_its_events(tmp_cfg, monkeypatch):
    codec = _codec()
    one = _write(tmp_cfg, X, codec)
    thr = np.float32(60.0)
    kw = dict(taps=TAPS33, reference='median', before=4)
    whole = one.residual(*EV, K3, 7, 4991, **kw)
    events = one.match_templates(K3, thr, 7, 4991, exclude=6, subtract=EV, **kw)
    assert len(codec.residual_calls) == 1 and len(codec.match_residual_calls) == 1 and events.sample.size
    for n_lanes in (2, 3):
        lc = _codec(n_lanes)
        many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=lc, check_after_decompress=False)
        assert many.residual(*EV, K3, 7, 4991, **kw).tobytes() == whole.tobytes()
        assert _events(many.match_templates(K3, thr, 7, 4991, exclude=6, subtract=EV, **kw)) == _events(events)
        for calls in (lc.residual_calls, lc.match_residual_calls):
            assert [c[0] for c in sorted(calls)] == list(range(n_lanes))
            bounds = sorted(c[3:5] for c in calls)                      # contiguous parts of the rows, one per lane
            assert bounds[0][0] == 7 and bounds[-1][1] == 4991 and all(a[1] == b[0] for a, b in zip(bounds[:-1], bounds[1:]))
        many.close()
    codec.residual_calls.clear()
    codec.match_residual_calls.clear()
    monkeypatch.setattr(api, 'RESIDUAL_CALL_BYTES', 1)                   # a call per chunk of the rows
    monkeypatch.setattr(api, 'TMATCH_CALL_BYTES', 1)
    assert one.residual(*EV, K3, 7, 4991, **kw).tobytes() == whole.tobytes()
    assert _events(one.match_templates(K3, thr, 7, 4991, exclude=6, subtract=EV, **kw)) == _events(events)
    assert [c[3:5] for c in codec.residual_calls] == [(7, 1000), (1000, 2000), (2000, 3000), (3000, 4000), (4000, 4991)]
    assert [c[1] for c in codec.residual_calls] == [[0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4]]       # the filter's halo: 16 rows either side
    assert [c[3:5] for c in codec.match_residual_calls] == [c[3:5] for c in codec.residual_calls]
    # the superset property: a call is handed a slice of the sorted list that holds every event whose window [s - 4, s + 5) meets the
    # rows it computes z for -- its own rows; for a match the rows, 6 either side and their template neighbours [a - 10, b + 10 + 4)
    srt = sorted(EV[0].tolist())
    for calls, lo, hi in ((codec.residual_calls, 0, 0), (codec.match_residual_calls, 6 + 4, 6 + 4)):
        for c in calls:
            a, b, got = c[3] - lo, c[4] + hi, c[-1]
            need = [s for s in srt if s - 4 < b and s + 5 > a]
            assert need and got == need and len(got) < len(srt)
    monkeypatch.setattr(api, 'RESIDUAL_CALL_BYTES', 1 << 30)
    monkeypatch.setattr(api, 'RESIDUAL_OUT_BYTES', 24 * 700)            # ... and a call's result is bounded: 700 rows
    codec.residual_calls.clear()
    assert one.residual(*EV, K3, 7, 4991, **kw).tobytes() == whole.tobytes()
    assert [c[3:5] for c in codec.residual_calls] == [(a, min(a + 700, 4991)) for a in range(7, 4991, 700)]
    one.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    kw = dict(taps=TAPS33, reference='median', before=4)
    cache = r._cache_for(0)
    cold = r.residual(*EV, K3, **kw)
    cold_ev = r.match_templates(K3, 60.0, subtract=EV, **kw)
    assert not codec.caches[cache]                                      # a scan inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    assert resident
    codec.residual_calls.clear()
    codec.match_residual_calls.clear()
    assert r.residual(*EV, K3, **kw).tobytes() == cold.tobytes() and _events(r.match_templates(K3, 60.0, subtract=EV, **kw)) == _events(cold_ev)
    assert sorted(codec.caches[cache]) == resident
    for calls in (codec.residual_calls, codec.match_residual_calls):
        (c,) = calls
        assert [k for k, n in zip(c[1], c[2]) if n == 0] == resident
    # an entry dropped between the query and the call: E_MISS, then everything is sent once more
    codec.residual_calls.clear()
    codec.miss_next_residual = True
    assert r.residual(*EV, K3, **kw).tobytes() == cold.tobytes()
    first, second = codec.residual_calls
    assert 0 in first[2] and all(second[2])
    r.close()


def test_damaged_chunk_in_the_support_raises(tmp_cfg):
    codec = _codec(2)
    r = _write(tmp_cfg, X, codec)
    r.close()
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    ch = r.chunk_offsets
    data[ch[3] + 20:ch[3] + 40] = b'\xff' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    kw = dict(taps=TAPS33, before=4)                                    # rows [a, b) read [a - 16, b + 16): the templates read nothing
    r.residual(*EV, K3, 0, 2984, **kw)
    r.residual(*EV, K3, 4016, 5000, **kw)
    with pytest.raises(IOError, match='#3'):
        r.residual(*EV, K3, 0, 2985, **kw)
    with pytest.raises(IOError, match='#3'):
        r.residual(*EV, K3, 4015, 5000, **kw)
    with pytest.raises(IOError, match='#3'):
        r.match_templates(K3, 1e9, 0, 2976, exclude=5, subtract=EV, **kw)
    r.close()


def test_argument_errors(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, synth_int16(0, 2000, 5, 9), codec)
    k = np.ones((2, 4, 5))
    good = dict(sample=[10, 20], template=[0, 1], amplitude=[1.0, 2.0], templates=k, start=10, stop=30, before=2)
    assert r.residual(**good).shape == (20, 5)
    assert r.match_templates(k, 1e9, 10, 30, before=2, subtract=([10, 20], [0, 1], [1.0, 2.0])).sample.size == 0
    codec.residual_calls.clear()
    codec.match_residual_calls.clear()
    nan = k.copy()
    nan[1, 2, 3] = np.nan
    bad_events = (dict(sample=[10]), dict(template=[0]), dict(amplitude=[1.0, 2.0, 3.0]),                   # lengths differ
                  dict(amplitude=[1.0, np.nan]), dict(amplitude=[np.inf, 1.0]), dict(amplitude=[1e39, 1.0]),  # not finite (in float32)
                  dict(template=[0, 2]), dict(template=[-1, 0]),                                             # no such template
                  dict(sample=[-1, 20]), dict(sample=[10, 2000]),                                            # outside the recording
                  dict(sample=[[10, 20]]), dict(sample=[1.0, 2.0]), dict(template=[0.0, 1.0]), dict(amplitude=['a', 'b']), dict(sample=7))
    for bad in bad_events + (dict(templates=np.ones(5)), dict(templates=np.ones((2, 4, 4))), dict(templates=np.ones((2, 257, 5))),
                             dict(templates=np.ones((0, 4, 5))), dict(templates=nan), dict(before=-1), dict(before=5), dict(before=1.0),
                             dict(reference='mean'), dict(taps=[]), dict(taps=[np.nan]), dict(channels=[0, 1, 2, 3]), dict(channels=[])):
        with pytest.raises(ValueError):
            r.residual(**{**good, **bad})
    for bad in bad_events:
        ev = {**dict(sample=[10, 20], template=[0, 1], amplitude=[1.0, 2.0]), **bad}
        with pytest.raises(ValueError):
            r.match_templates(k, 1.0, 10, 30, before=2, subtract=(ev['sample'], ev['template'], ev['amplitude']))
    for shape in (([10], [0]), ([10], [0], [1.0], [2]), 5, 'abc', np.zeros((3, 2)), dict(sample=[1])):        # wrong subtract shape
        with pytest.raises(ValueError):
            r.match_templates(k, 1.0, 10, 30, before=2, subtract=shape)
    with pytest.raises(IndexError):
        r.residual([1], [0], [1.0], np.ones((4, 1)), channels=5, before=0)
    assert not codec.residual_calls and not codec.match_residual_calls and not codec.match_templates_calls   # every error came before a device call
    # a template index is checked against the templates, an amplitude may be zero or negative, events may lie anywhere in the recording
    assert r.residual([0, 1999, 1999], [1, 1, 0], [0.0, -1.0, 3e38], k, 5, 9, before=4).shape == (4, 5)
    r.close()
    for bad in (dict(template=[0, 4]), dict(template=[0.5, 1]), dict(score=[1.0]), dict(templates=np.zeros((4, 2, 2))), dict(templates=np.ones(3)),
                dict(templates=np.full((4, 2, 2), np.inf))):
        with pytest.raises(ValueError):
            api.template_amplitudes(**{**dict(score=[1.0, 2.0], template=[0, 3], templates=np.ones((4, 2, 2))), **bad})
    zero = np.ones((3, 2, 2))
    zero[1] = 0
    with pytest.raises(ValueError, match='template 1'):
        api.template_amplitudes([1.0, 2.0, 3.0], [0, 1, 2], zero)
    assert api.template_amplitudes([1.0, 3.0], [0, 2], zero).tolist() == [0.25, 0.75]       # (a template that no event names may be zero)


def test_exports_are_listed_and_declared():
    names = {'mts_residual', 'mts_dev_residual', 'mts_match_residual', 'mts_dev_match_residual'}
    assert names <= set(hip.EXPORTS)
    for name in ('residual', 'match_residual'):
        assert callable(getattr(api.HipCodec, name)) and callable(getattr(hip, name)) and callable(getattr(hip, 'dev_' + name))
    header = (ROOT / 'include' / 'mtscomp_hip.h').read_text()
    assert names <= set(re.findall(r'\b(mts_[a-z0-9_]+)\s*\(', header))
    assert hip.RESIDUAL_MAX_EVENTS == 1 << 30


def test_exact_peel_of_two_overlapping_spikes(tmp_cfg):
    """Two integer templates on disjoint channels, planted 5 rows apart in a recording of zeros (z = x exactly): the first pass sees the
    stronger one alone, the second pass -- with it subtracted at its fitted amplitude -- exactly the weaker one, and the residual of
    both is +0 everywhere."""
    k = np.zeros((2, 7, 4))
    k[0, :, 0] = k[0, :, 1] = [1, 3, 6, 9, 6, 3, 1]                     # |K0|^2 = 346
    k[1, :, 2] = k[1, :, 3] = [1, 2, 4, 6, 4, 2, 1]                     # |K1|^2 = 156
    n0, n1 = 346.0, 156.0
    assert (np.sum(k[0] ** 2), np.sum(k[1] ** 2)) == (n0, n1)
    t0, before = 997, 3                                                 # astride the first chunk boundary
    x = np.zeros((3000, 4), np.int16)
    x[t0 - 3:t0 + 4] += k[0].astype(np.int16)
    x[t0 + 5 - 3:t0 + 5 + 4] += k[1].astype(np.int16)
    thr = np.float32(n1 / 2)
    # the oracle's verdict first: no sidelobe beyond exclude = T - 1 = 6 rows is an event (K1's autocorrelation at lag 2 is 96 > 78, and
    # beaten by 156 two rows away), and the weaker spike is hidden from the first pass and from it alone
    first = match_templates(x, 0, 0, 3000, 0, 3000, [1.0], 0, before, k, thr, 6)
    assert [v.tolist() for v in first] == [[t0], [0], [n0]]
    assert correlate(x, 0, 0, 3000, t0 + 5, t0 + 6, [1.0], 0, before, k)[0].tolist() == [12.0, n1]    # K0's lag 5: 2 * (1 * 3 + 3 * 1)
    second = match_residual(x, 0, 0, 3000, 0, 3000, [1.0], 0, before, k, thr, 6, [t0], [0], [1.0])
    assert [v.tolist() for v in second] == [[t0 + 5], [1], [n1]]
    for n_lanes in (1, 2):
        r = _write(tmp_cfg, x, _codec(n_lanes))
        ev = r.match_templates(k, thr, before=before)
        assert (ev.sample.tolist(), ev.template.tolist(), ev.score.tolist(), ev.exclude) == ([t0], [0], [n0], 6)
        amp = api.template_amplitudes(ev.score, ev.template, k)
        assert amp.tolist() == [1.0]
        ev2 = r.match_templates(k, thr, before=before, subtract=(ev.sample, ev.template, amp))
        assert (ev2.sample.tolist(), ev2.template.tolist(), ev2.score.tolist()) == ([t0 + 5], [1], [n1])
        amp2 = api.template_amplitudes(ev2.score, ev2.template, k)
        both = (np.concatenate([ev2.sample, ev.sample]), np.concatenate([ev2.template, ev.template]), np.concatenate([amp2, amp]))
        assert r.residual(*both, k, before=before).tobytes() == np.zeros((3000, 4), np.float32).tobytes()
        assert r.match_templates(k, thr, before=before, subtract=both).sample.size == 0
        assert r.residual(ev.sample, ev.template, amp, k, t0 - 3, t0 + 9, before=before)[:, :2].tobytes() == bytes(4 * 2 * 12)
        r.close()
