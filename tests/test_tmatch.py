"""Reader.match_templates, host side: argument handling, the halo at both ends of the file, call cutting, lanes, the second call of a
short buffer, cache use and errors, driven through a numpy restatement of mts_match_templates (tests/tmatch_oracle.py).  The
kernels: tests/test_gpu_match_templates.py."""
import re
from pathlib import Path

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.correlate_oracle import correlate
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
    return TmatchOracleCodec(n_lanes=n_lanes, capacity_chunks=8)


def _want(x, cols, taps, reference, i0, i1, before, k, thr, R):
    return match_templates(x[:, np.asarray(cols)], 0, 0, x.shape[0], i0, i1, [1.0] if taps is None else taps, 1 if reference else 0, before,
                           np.asarray(k, np.float32), thr, R)


def _same(ev, want):
    return ((ev.sample.dtype, ev.template.dtype, ev.score.dtype) == (np.int64, np.int64, np.float32) and
            all(a.tobytes() == b.tobytes() for a, b in zip((ev.sample, ev.template, ev.score), want)))


def _events(ev):
    return ev.sample.tobytes(), ev.template.tobytes(), ev.score.tobytes()


TAPS33 = api.highpass_taps(300, 5000, 33)
X = synth_int16(0, 5000, 6, 4)                                         # five chunks of 1000 rows
K3 = np.random.RandomState(0).randn(3, 9, 6)
THR = {(taps is not None, ref, before): np.percentile(correlate(X, 0, 0, 5000, 0, 5000, [1.0] if taps is None else taps, 1 if ref else 0, before,
                                                                K3.astype(np.float32)), 90, axis=0).astype(np.float32)
       for taps, ref, before in ((TAPS33, 'median', 4), (None, None, 0), (None, 'median', 9))}


def test_events_are_the_definition_and_stitch(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    for taps, reference, before in ((TAPS33, 'median', 4), (None, None, 0), (None, 'median', 9)):
        thr = THR[taps is not None, reference, before]
        for R in (0, 3, None):
            kw = dict(taps=taps, reference=reference, before=before, exclude=R)
            whole = r.match_templates(K3, thr, **kw)
            assert whole.exclude == (8 if R is None else R) and whole.sample.size > 0          # exclude=None: T - 1
            assert _same(whole, _want(X, range(6), taps, reference, 0, 5000, before, K3, thr, whole.exclude))
            assert (whole.start, whole.stop, whole.channels.tolist(), whole.threshold.tobytes()) == (0, 5000, list(range(6)), thr.tobytes())
            for a, b, c in ((0, 1234, 5000), (990, 1000, 1010), (4990, 4999, 5000)):
                left, right = r.match_templates(K3, thr, a, b, **kw), r.match_templates(K3, thr, b, c, **kw)
                sel = (whole.sample >= a) & (whole.sample < c)
                assert np.concatenate([left.sample, right.sample]).tobytes() == whole.sample[sel].tobytes()
                assert np.concatenate([left.template, right.template]).tobytes() == whole.template[sel].tobytes()
                assert np.concatenate([left.score, right.score]).tobytes() == whole.score[sel].tobytes()
    # a 2-D template is one template; a scalar threshold is one per template; channels choose and order the columns
    one = r.match_templates(K3[1], 5.0, 100, 300, taps=TAPS33, before=4)
    assert _events(one) == _events(r.match_templates(K3[1:2], [5.0], 100, 300, taps=TAPS33, before=4)) and not one.template.any()
    cols = [5, 0, 0, 3]
    got = r.match_templates(K3[:, :, :4], -3e38, 40, 90, channels=cols, reference='median', before=2, exclude=2)
    assert got.sample.size and _same(got, _want(X, cols, None, 'median', 40, 90, 2, K3[:, :, :4], -3e38, 2))
    # an empty range: no device call
    codec.match_templates_calls.clear()
    assert r.match_templates(K3, 1.0, 700, 700, before=0).sample.size == 0 and r.match_templates(K3[0], 1.0, 9, 3, before=9).sample.size == 0
    assert not codec.match_templates_calls
    # rows that read nothing of the recording score +0 (row 0 under a template that lies wholly before it): a call without chunks
    top = r.match_templates(K3[:, :1], -1.0, 0, 1, before=1, exclude=0)
    assert (top.sample.tolist(), top.template.tolist(), top.score.tobytes()) == ([0], [0], np.zeros(1, np.float32).tobytes())
    assert r.match_templates(K3[:, :1], 1.0, 0, 1, before=1, exclude=0).sample.size == 0
    assert [c[1] for c in codec.match_templates_calls] == [[], []]
    r.close()


def test_chunk_spans_include_the_halo_at_both_ends(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    # L = 33: half = 16; T = 9, before = 4, R = 5: rows [a, b) read file rows [a - 5 - 4 + 16 - 32, b + 5 + 4 + 16) = [a - 25, b + 25)

    def spans(a, b, **kw):
        codec.match_templates_calls.clear()
        r.match_templates(K3, 1e9, a, b, taps=TAPS33, before=4, exclude=5, **kw)
        return [c[1] for c in codec.match_templates_calls], [c[3:5] for c in codec.match_templates_calls]
    assert spans(1025, 1975) == ([[1]], [(1025, 1975)])
    assert spans(1024, 1975)[0] == [[0, 1]] and spans(1025, 1976)[0] == [[1, 2]]
    assert spans(0, 975)[0] == [[0]] and spans(0, 976)[0] == [[0, 1]]            # the halo before row 0 does not exist
    assert spans(4025, 5000)[0] == [[4]] and spans(4024, 5000)[0] == [[3, 4]]    # nor the one past the last row
    assert spans(0, 5000) == ([[0, 1, 2, 3, 4]], [(0, 5000)])
    # exclude widens the span on both sides; before shifts the template, not the filter
    codec.match_templates_calls.clear()
    r.match_templates(K3, 1e9, 1016, 1976, taps=TAPS33, before=0, exclude=0)    # [a - 16, b + 8 + 16)
    r.match_templates(K3, 1e9, 1025, 1985, taps=TAPS33, before=9, exclude=0)    # [a - 25, b - 1 + 16)
    r.match_templates(K3, 1e9, 1275, 1725, taps=TAPS33, before=4, exclude=255)  # [a - 275, b + 275)
    r.match_templates(K3, 1e9, 1274, 1725, taps=TAPS33, before=4, exclude=255)
    assert [c[1] for c in codec.match_templates_calls] == [[1], [1], [1], [0, 1]]
    r.close()


def test_lanes_and_call_cuts_give_identical_events(tmp_cfg, monkeypatch):
    codec = _codec()
    one = _write(tmp_cfg, X, codec)
    thr = THR[True, 'median', 4]
    kw = dict(taps=TAPS33, reference='median', before=4, exclude=6)
    whole = one.match_templates(K3, thr, 7, 4991, **kw)
    assert len(codec.match_templates_calls) == 1
    assert whole.sample.size and _same(whole, _want(X, range(6), TAPS33, 'median', 7, 4991, 4, K3, thr, 6))
    for n_lanes in (2, 3):
        lc = _codec(n_lanes)
        many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=lc, check_after_decompress=False)
        assert _events(many.match_templates(K3, thr, 7, 4991, **kw)) == _events(whole)
        assert [c[0] for c in sorted(lc.match_templates_calls)] == list(range(n_lanes))
        bounds = sorted(c[3:5] for c in lc.match_templates_calls)          # contiguous parts of the rows, one per lane
        assert bounds[0][0] == 7 and bounds[-1][1] == 4991 and all(a[1] == b[0] for a, b in zip(bounds[:-1], bounds[1:]))
        for c in lc.match_templates_calls:                                 # a lane reads adjacent chunks
            assert c[1] == list(range(c[1][0], c[1][-1] + 1))
        many.close()
    codec.match_templates_calls.clear()
    monkeypatch.setattr(api, 'TMATCH_CALL_BYTES', 1)                      # a call per chunk of the rows
    assert _events(one.match_templates(K3, thr, 7, 4991, **kw)) == _events(whole)
    assert [c[3:5] for c in codec.match_templates_calls] == [(7, 1000), (1000, 2000), (2000, 3000), (3000, 4000), (4000, 4991)]
    assert [c[1] for c in codec.match_templates_calls] == [[0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4]]
    one.close()


def test_short_buffer_is_called_again(tmp_cfg, monkeypatch):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    monkeypatch.setattr(api, 'TMATCH_GUESS_MIN', 10)
    monkeypatch.setattr(api, 'TMATCH_GUESS_SAMPLES', 1000)
    dense = r.match_templates(K3, -3e38, 100, 4100, before=4, exclude=0)                  # every row is an event
    assert dense.sample.tolist() == list(range(100, 4100))
    assert [c[5] for c in codec.match_templates_calls] == [10, 4000]                      # the guess, then room for all
    assert _same(dense, _want(X, range(6), None, None, 100, 4100, 4, K3, -3e38, 0))
    codec.match_templates_calls.clear()
    sparse = r.match_templates(K3, 1e9, 100, 4100, before=4)
    assert sparse.sample.size == 0 and [c[5] for c in codec.match_templates_calls] == [10]
    monkeypatch.setattr(api, 'TMATCH_GUESS_MIN', 4096)
    monkeypatch.setattr(api, 'TMATCH_GUESS_SAMPLES', 64)
    codec.match_templates_calls.clear()
    r.match_templates(K3, 1e9, 0, 100, before=4)
    r.match_templates(K3, 1e9, before=4)
    assert [c[5] for c in codec.match_templates_calls] == [4096, 4096]
    r.close()
    big = _write(tmp_cfg, np.zeros((64 * 5000, 1), np.int16), _codec())
    big.match_templates(np.ones((1, 1)), 1.0, before=0)
    assert [c[5] for c in big.codec.match_templates_calls] == [5000]                       # one event per TMATCH_GUESS_SAMPLES rows
    big.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    thr = THR[True, 'median', 4]
    cache = r._cache_for(0)
    cold = r.match_templates(K3, thr, taps=TAPS33, reference='median', before=4)
    assert cold.sample.size and not codec.caches[cache]                 # a scan inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    assert resident
    codec.match_templates_calls.clear()
    warm = r.match_templates(K3, thr, taps=TAPS33, reference='median', before=4)
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens, _, _, _), = codec.match_templates_calls
    assert [k for k, n in zip(keys, lens) if n == 0] == resident
    assert _events(warm) == _events(cold)
    # an entry dropped between the query and the call: E_MISS, then everything is sent once more
    codec.match_templates_calls.clear()
    codec.miss_next_match_templates = True
    assert _events(r.match_templates(K3, thr, taps=TAPS33, reference='median', before=4)) == _events(cold)
    (_, _, lens_a, _, _, _), (_, _, lens_b, _, _, _) = codec.match_templates_calls
    assert 0 in lens_a and all(lens_b)
    r.close()


def test_damaged_chunk_in_the_halo_raises(tmp_cfg):
    codec = _codec(2)
    r = _write(tmp_cfg, X, codec)
    r.close()
    data = bytearray((tmp_cfg / 'data.cbin').read_bytes())
    ch = r.chunk_offsets
    data[ch[3] + 20:ch[3] + 40] = b'\xff' * 20
    (tmp_cfg / 'data.cbin').write_bytes(bytes(data))
    r = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=codec, check_after_decompress=False)
    kw = dict(taps=TAPS33, before=4, exclude=5)                         # rows [a, b) read [a - 25, b + 25)
    r.match_templates(K3, 1e9, 0, 2975, **kw)                           # rows [.., 3000): chunk 3 is not read
    r.match_templates(K3, 1e9, 4025, 5000, **kw)
    with pytest.raises(IOError, match='#3'):
        r.match_templates(K3, 1e9, 0, 2976, **kw)                       # the halo alone reaches it, from below ...
    with pytest.raises(IOError, match='#3'):
        r.match_templates(K3, 1e9, 4024, 5000, **kw)                    # ... and from above
    with pytest.raises(IOError, match='#3'):
        r.match_templates(K3, -3e38, exclude=0, taps=TAPS33, before=4)  # (a short buffer near a failed chunk is not called again)
    r.close()


def test_argument_errors(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, synth_int16(0, 2000, 5, 9), codec)
    k = np.ones((2, 4, 5))
    assert r.match_templates(k, 1e9, 10, 30, before=2).sample.size == 0
    codec.match_templates_calls.clear()
    nan, inf, big = k.copy(), k.copy(), k.copy()
    nan[1, 2, 3], inf[0, 0, 0], big[1, 3, 4] = np.nan, -np.inf, 1e39           # (1e39 is finite in float64, not in float32)
    for bad in (dict(templates=np.ones(5)), dict(templates=np.ones((1, 2, 4, 5))), dict(templates=np.ones((2, 4, 5), dtype=complex)),
                dict(templates='ab'), dict(templates=np.ones((2, 4, 4))), dict(templates=np.ones((2, 4, 6))), dict(templates=np.ones((4, 4))),
                dict(templates=np.ones((2, 0, 5))), dict(templates=np.ones((2, 257, 5))), dict(templates=np.ones((0, 4, 5))),
                dict(templates=np.ones((1025, 1, 5))), dict(templates=nan), dict(templates=inf), dict(templates=big),
                dict(before=-1), dict(before=5), dict(before=20), dict(before=1.0), dict(before=True), dict(before=None),
                dict(reference='mean'), dict(reference=1), dict(taps=[]), dict(taps=[np.nan]), dict(taps=np.ones(8193)),
                dict(channels=[0, 1, 2, 3]), dict(channels=[]),
                dict(exclude=-1), dict(exclude=256), dict(exclude=1.0), dict(exclude=True), dict(exclude='a'),
                dict(threshold=np.nan), dict(threshold=np.inf), dict(threshold=1e39), dict(threshold=[1.0, np.nan]), dict(threshold=[1.0]),
                dict(threshold=[1.0, 2.0, 3.0]), dict(threshold=[[1.0, 2.0]]), dict(threshold='x'), dict(threshold=None), dict(threshold=1j)):
        with pytest.raises(ValueError):
            r.match_templates(**{**dict(templates=k, threshold=1.0, start=10, stop=30, before=2), **bad})
    with pytest.raises(IndexError):
        r.match_templates(np.ones((4, 1)), 1.0, channels=5, before=0)
    assert not codec.match_templates_calls                              # every error came before a device call
    assert hip.TMATCH_MAX_EXCLUDE == 255
    assert r.match_templates(np.ones((2, 256, 5)), 1e9, 10, 12, before=256).exclude == 255    # exclude=None: min(T - 1, 255)
    assert r.match_templates(np.ones((2, 1, 5)), 1e9, 10, 12, before=0).exclude == 0
    assert r.match_templates(np.ones((1024, 1, 5)), [-5.0] * 1024, 10, 12, before=0, exclude=255).threshold.tolist() == [-5.0] * 1024   # of any sign
    r.close()
    wide = np.zeros((10, hip.CORRELATE_MAX_COLS + 1), np.int16)
    r = _write(tmp_cfg, wide, _codec())
    for kw in (dict(reference='median'), dict()):                      # too many columns for a median; too wide a template
        with pytest.raises(ValueError):
            r.match_templates(np.zeros((1, 1, 1025)), 1.0, before=0, **kw)
    assert r.match_templates(np.zeros((1, 1, 1024)), -1.0, channels=slice(0, 1024), reference='median', before=1).sample.tolist() == list(range(10))
    r.close()


def test_needs_a_device_codec(tmp_cfg):
    r = _write(tmp_cfg, synth_int16(0, 2000, 3, 0), OracleCodec())
    with pytest.raises(NotImplementedError):
        r.match_templates(np.ones((1, 2, 3)), 1.0, before=1)
    r.close()


def test_exports_are_listed_and_declared():
    assert {'mts_match_templates', 'mts_dev_match_templates'} <= set(hip.EXPORTS)
    assert callable(api.HipCodec.match_templates) and callable(hip.match_templates) and callable(hip.dev_match_templates)
    header = (ROOT / 'include' / 'mtscomp_hip.h').read_text()
    assert {'mts_match_templates', 'mts_dev_match_templates'} <= set(re.findall(r'\b(mts_[a-z0-9_]+)\s*\(', header))
    common = (ROOT / 'mtscomp_amd' / 'csrc' / 'common.h').read_text()
    assert re.search(r'#define MTS_TMATCH_MAX_EXCLUDE %d\b' % hip.TMATCH_MAX_EXCLUDE, header)
    assert 'TMATCH_MAX_EXCLUDE = MTS_TMATCH_MAX_EXCLUDE;' in common
