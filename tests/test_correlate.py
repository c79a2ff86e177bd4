"""Reader.correlate, host side: argument handling, the halo at both ends of the file, call cutting, lanes, cache use and errors,
driven through a numpy restatement of mts_correlate (tests/correlate_oracle.py).  The kernel: tests/test_gpu_correlate.py."""
import re
from pathlib import Path

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.correlate_oracle import CorrelateOracleCodec, correlate

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
    return CorrelateOracleCodec(n_lanes=n_lanes, capacity_chunks=8)


def _want(x, cols, taps, reference, i0, i1, before, k):
    k = np.asarray(k)
    return correlate(x[:, np.asarray(cols)], 0, 0, x.shape[0], i0, i1, [1.0] if taps is None else taps, 1 if reference else 0, before,
                     k[None] if k.ndim == 2 else k)


TAPS33 = api.highpass_taps(300, 5000, 33)
X = synth_int16(0, 5000, 6, 4)                                         # five chunks of 1000 rows
K3 = np.random.RandomState(0).randn(3, 9, 6)


def test_scores_are_the_definition_and_stitch(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    for taps, reference, before in ((TAPS33, 'median', 4), (None, None, 0), (None, 'median', 9)):
        whole = r.correlate(K3, taps=taps, reference=reference, before=before)
        assert whole.dtype == np.float32 and whole.shape == (5000, 3)
        assert whole.tobytes() == _want(X, range(6), taps, reference, 0, 5000, before, K3).tobytes()
        for a, b, c in ((0, 1234, 5000), (990, 1000, 1010), (4990, 4999, 5000)):
            parts = np.concatenate([r.correlate(K3, a, b, taps=taps, reference=reference, before=before),
                                    r.correlate(K3, b, c, taps=taps, reference=reference, before=before)])
            assert parts.tobytes() == whole[a:c].tobytes()
    # a 2-D template is one template and gives a 1-D result; channels choose and order the columns
    one = r.correlate(K3[1], 100, 300, taps=TAPS33, before=4)
    assert one.shape == (200,) and one.tobytes() == r.correlate(K3[1:2], 100, 300, taps=TAPS33, before=4)[:, 0].tobytes()
    cols = [5, 0, 0, 3]
    got = r.correlate(K3[:, :, :4], 40, 90, channels=cols, reference='median', before=2)
    assert got.tobytes() == _want(X, cols, None, 'median', 40, 90, 2, K3[:, :, :4]).tobytes()
    assert r.correlate(K3[:, :, 0:1], 40, 90, channels=2, before=1).shape == (50, 3)
    # an empty range: no device call
    codec.correlate_calls.clear()
    assert r.correlate(K3, 700, 700, before=0).shape == (0, 3) and r.correlate(K3[0], 9, 3, before=9).shape == (0,) and not codec.correlate_calls
    # rows that read nothing of the recording: +0 without a call (row 0 under a template that lies wholly before it)
    top = r.correlate(K3[:, :1], 0, 1, before=1)
    assert top.tobytes() == np.zeros((1, 3), np.float32).tobytes() and not codec.correlate_calls
    r.close()


def test_chunk_spans_include_the_halo_at_both_ends(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    # L = 33: half = 16; T = 9, before = 4: rows [a, b) read file rows [a - 4 + 16 - 32, b + 4 + 16) = [a - 20, b + 20)

    def spans(a, b, **kw):
        codec.correlate_calls.clear()
        r.correlate(K3, a, b, taps=TAPS33, before=4, **kw)
        return [c[1] for c in codec.correlate_calls], [c[3:] for c in codec.correlate_calls]
    assert spans(1020, 1980) == ([[1]], [(1020, 1980)])
    assert spans(1019, 1980)[0] == [[0, 1]] and spans(1020, 1981)[0] == [[1, 2]]
    assert spans(0, 980)[0] == [[0]] and spans(0, 981)[0] == [[0, 1]]            # the halo before row 0 does not exist
    assert spans(4020, 5000)[0] == [[4]] and spans(4019, 5000)[0] == [[3, 4]]    # nor the one past the last row
    assert spans(0, 5000) == ([[0, 1, 2, 3, 4]], [(0, 5000)])
    # before = 0 and before = T shift the template, not the filter
    codec.correlate_calls.clear()
    r.correlate(K3, 1016, 1976, taps=TAPS33, before=0)                          # [a - 16, b + 8 + 16)
    r.correlate(K3, 1025, 1985, taps=TAPS33, before=9)                          # [a - 25, b - 1 + 16)
    assert [c[1] for c in codec.correlate_calls] == [[1], [1]]
    r.close()


def test_lanes_and_call_cuts_give_identical_bytes(tmp_cfg, monkeypatch):
    codec = _codec()
    one = _write(tmp_cfg, X, codec)
    kw = dict(taps=TAPS33, reference='median', before=4)
    whole = one.correlate(K3, 7, 4991, **kw)
    assert len(codec.correlate_calls) == 1
    assert whole.tobytes() == _want(X, range(6), TAPS33, 'median', 7, 4991, 4, K3).tobytes()
    for n_lanes in (2, 3):
        lc = _codec(n_lanes)
        many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=lc, check_after_decompress=False)
        assert many.correlate(K3, 7, 4991, **kw).tobytes() == whole.tobytes()
        assert [c[0] for c in sorted(lc.correlate_calls)] == list(range(n_lanes))
        bounds = sorted(c[3:] for c in lc.correlate_calls)                 # contiguous parts of the rows, one per lane
        assert bounds[0][0] == 7 and bounds[-1][1] == 4991 and all(a[1] == b[0] for a, b in zip(bounds[:-1], bounds[1:]))
        for _, keys, _, _, _ in lc.correlate_calls:                        # a lane reads adjacent chunks
            assert keys == list(range(keys[0], keys[-1] + 1))
        many.close()
    codec.correlate_calls.clear()
    monkeypatch.setattr(api, 'CORRELATE_CALL_BYTES', 1)                   # a call per chunk of the rows
    assert one.correlate(K3, 7, 4991, **kw).tobytes() == whole.tobytes()
    assert [c[3:] for c in codec.correlate_calls] == [(7, 1000), (1000, 2000), (2000, 3000), (3000, 4000), (4000, 4991)]
    assert [c[1] for c in codec.correlate_calls] == [[0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4]]
    monkeypatch.setattr(api, 'CORRELATE_CALL_BYTES', 1 << 30)
    codec.correlate_calls.clear()
    monkeypatch.setattr(api, 'CORRELATE_OUT_BYTES', 700 * 3 * 4)          # 700 rows of three scores per call
    assert one.correlate(K3, 7, 4991, **kw).tobytes() == whole.tobytes()
    assert [c[4] - c[3] for c in codec.correlate_calls] == [700] * 7 + [84]
    one.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, X, codec)
    cache = r._cache_for(0)
    cold = r.correlate(K3, taps=TAPS33, before=4)
    assert not codec.caches[cache]                                     # a scan inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    assert resident
    codec.correlate_calls.clear()
    warm = r.correlate(K3, taps=TAPS33, before=4)
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens, _, _), = codec.correlate_calls
    assert [k for k, n in zip(keys, lens) if n == 0] == resident
    assert warm.tobytes() == cold.tobytes()
    # an entry dropped between the query and the call: E_MISS, then everything is sent once more
    codec.correlate_calls.clear()
    codec.miss_next_correlate = True
    assert r.correlate(K3, taps=TAPS33, before=4).tobytes() == cold.tobytes()
    (_, _, lens_a, _, _), (_, _, lens_b, _, _) = codec.correlate_calls
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
    kw = dict(taps=TAPS33, before=4)
    r.correlate(K3, 0, 2980, **kw)                                      # rows [.., 3000): chunk 3 is not read
    r.correlate(K3, 4020, 5000, **kw)
    with pytest.raises(IOError, match='#3'):
        r.correlate(K3, 0, 2981, **kw)                                  # the halo alone reaches it, from below ...
    with pytest.raises(IOError, match='#3'):
        r.correlate(K3, 4019, 5000, **kw)                               # ... and from above
    with pytest.raises(IOError, match='#3'):
        r.correlate(K3, **kw)
    r.close()


def test_argument_errors(tmp_cfg):
    codec = _codec()
    r = _write(tmp_cfg, synth_int16(0, 2000, 5, 9), codec)
    k = np.ones((2, 4, 5))
    assert r.correlate(k, 10, 30, before=2).shape == (20, 2)
    codec.correlate_calls.clear()
    nan, inf, big = k.copy(), k.copy(), k.copy()
    nan[1, 2, 3], inf[0, 0, 0], big[1, 3, 4] = np.nan, -np.inf, 1e39           # (1e39 is finite in float64, not in float32)
    for bad in (dict(templates=np.ones(5)), dict(templates=np.ones((1, 2, 4, 5))), dict(templates=np.ones((2, 4, 5), dtype=complex)),
                dict(templates='ab'), dict(templates=np.ones((2, 4, 4))), dict(templates=np.ones((2, 4, 6))), dict(templates=np.ones((4, 4))),
                dict(templates=np.ones((2, 0, 5))), dict(templates=np.ones((2, 257, 5))), dict(templates=np.ones((0, 4, 5))),
                dict(templates=np.ones((1025, 1, 5))), dict(templates=nan), dict(templates=inf), dict(templates=big),
                dict(before=-1), dict(before=5), dict(before=20), dict(before=1.0), dict(before=True), dict(before=None),
                dict(reference='mean'), dict(reference=1), dict(taps=[]), dict(taps=[np.nan]), dict(taps=np.ones(8193)),
                dict(channels=[0, 1, 2, 3]), dict(channels=[])):
        with pytest.raises(ValueError):
            r.correlate(**{**dict(templates=k, start=10, stop=30, before=2), **bad})
    with pytest.raises(IndexError):
        r.correlate(np.ones((4, 1)), channels=5, before=0)
    assert not codec.correlate_calls                                    # every error came before a device call
    assert (hip.CORRELATE_MAX_T, hip.CORRELATE_MAX_OUT, hip.CORRELATE_MAX_COLS) == (256, 1024, 1024)
    assert r.correlate(np.ones((2, 256, 5)), 10, 12, before=256).shape == (2, 2)
    assert r.correlate(np.ones((1024, 1, 5)), 10, 12, before=0).shape == (2, 1024)
    r.close()
    wide = np.zeros((10, hip.CORRELATE_MAX_COLS + 1), np.int16)
    r = _write(tmp_cfg, wide, _codec())
    for kw in (dict(reference='median'), dict()):                      # too many columns for a median; too wide a template
        with pytest.raises(ValueError):
            r.correlate(np.zeros((1, 1, 1025)), before=0, **kw)
    assert r.correlate(np.zeros((1, 1, 1024)), channels=slice(0, 1024), reference='median', before=1).shape == (10, 1)
    r.close()


def test_needs_a_device_codec(tmp_cfg):
    r = _write(tmp_cfg, synth_int16(0, 2000, 3, 0), OracleCodec())
    with pytest.raises(NotImplementedError):
        r.correlate(np.ones((1, 2, 3)), before=1)
    r.close()


def test_exports_are_listed_and_declared():
    assert {'mts_correlate', 'mts_dev_correlate'} <= set(hip.EXPORTS)
    assert callable(api.HipCodec.correlate) and callable(hip.correlate) and callable(hip.dev_correlate)
    header = (ROOT / 'include' / 'mtscomp_hip.h').read_text()
    assert {'mts_correlate', 'mts_dev_correlate'} <= set(re.findall(r'\b(mts_[a-z0-9_]+)\s*\(', header))
    common = (ROOT / 'mtscomp_amd' / 'csrc' / 'common.h').read_text()
    for name, value in (('MAX_T', hip.CORRELATE_MAX_T), ('MAX_OUT', hip.CORRELATE_MAX_OUT), ('MAX_COLS', hip.CORRELATE_MAX_COLS)):
        assert re.search(r'#define MTS_CORRELATE_%s %d\b' % (name, value), header)
        assert 'CORRELATE_%s = MTS_CORRELATE_%s;' % (name, name) in common
