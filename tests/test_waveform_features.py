"""Reader.waveform_features and api.waveform_basis, host side: argument handling, any order of the events, the 1-D basis, call
cutting, lanes, cache use and errors, driven through a numpy restatement of mts_waveform_features (tests/features_oracle.py).  The
kernel: tests/test_gpu_waveform_features.py."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from mtscomp_amd.synth import synth_int16
from tests.codec_oracle import OracleCodec
from tests.features_oracle import FeaturesOracleCodec, chain, features

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
    return FeaturesOracleCodec(n_lanes=n_lanes, capacity_chunks=8)


def _basis(P, T, seed=0):
    return np.random.RandomState(seed).standard_normal((P, T)).astype(np.float32)


def _same(a, b):
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


def _want(x, cols, taps, reference, sample, col0, before, after, W, basis):
    return features(x[:, np.asarray(cols)], 0, 0, x.shape[0], [1.0] if taps is None else taps, 1 if reference else 0, sample, col0, before,
                    after, W, basis)


@pytest.mark.parametrize('reference', [None, 'median'])
def test_detect_then_features_is_the_chain_on_waveforms_snippets(tmp_cfg, reference):
    x = synth_int16(0, 3000, 70, 4)
    r = _write(tmp_cfg, x, _codec(), sample_rate=700.)
    ev = r.detect(12, taps=TAPS65, sign='neg', reference=reference, exclude=7, spread=3)
    assert ev.sample.size > 300
    w = r.waveforms(ev.sample, ev.channel, neighbours=8, taps=TAPS65, reference=reference).waveforms
    basis = api.waveform_basis(w, 3)
    got = r.waveform_features(ev.sample, basis, ev.channel, neighbours=8, taps=TAPS65, reference=reference)
    assert got.features.shape == (ev.sample.size, 3, 17) and (got.before, got.after) == (20, 41)
    assert got.basis.dtype == np.float32 and got.basis.tobytes() == basis.tobytes()
    assert np.array_equal(got.channels, np.arange(70)) and np.array_equal(got.sample, ev.sample) and np.array_equal(got.position, ev.channel - 8)
    _same(got.features, chain(w, basis))                              # identity: the chain on Reader.waveforms' own snippets
    _same(got.features, _want(x, np.arange(70), TAPS65, reference, ev.sample, ev.channel - 8, 20, 41, 17, basis))
    nan = np.isnan(got.features)
    assert nan.any() and not nan.all() and np.array_equal(nan.any(axis=1), np.isnan(w).any(axis=1))
    # the features are the float projection of the snippets to float32 accuracy
    ok = ~nan
    plain = np.einsum('etw,pt->epw', np.nan_to_num(w).astype(np.float64), basis.astype(np.float64))
    scale = np.einsum('etw,pt->epw', np.abs(np.nan_to_num(w)).astype(np.float64), np.abs(basis).astype(np.float64))
    assert (np.abs(got.features[ok] - plain[ok]) <= 61 * 2.0 ** -24 * scale[ok] + 1e-30).all()
    r.close()


def test_any_order_repeats_one_d_basis_and_full_width(tmp_cfg):
    x = synth_int16(0, 5000, 12, 4)
    codec = _codec()
    r = _write(tmp_cfg, x, codec)
    rs = np.random.RandomState(0)
    sample = rs.randint(0, 5000, 300)
    sample[:40] = sample[40:80]                                        # repeats, shuffled
    sample[[5, 17]] = [0, 4999]
    channel = rs.randint(0, 12, 300)
    basis = _basis(5, 19)
    for reference in (None, 'median'):
        got = r.waveform_features(sample, basis, channel, before=7, after=12, neighbours=2, taps=TAPS65, reference=reference)
        assert got.features.shape == (300, 5, 5)
        _same(got.features, _want(x, np.arange(12), TAPS65, reference, sample, channel - 2, 7, 12, 5, basis))
        order = rs.permutation(300)
        again = r.waveform_features(sample[order], basis, channel[order], before=7, after=12, neighbours=2, taps=TAPS65, reference=reference)
        _same(again.features, got.features[order])
        whole = r.waveform_features(sample, basis, before=7, after=12, taps=TAPS65, reference=reference)
        assert whole.features.shape == (300, 5, 12) and not whole.position.any()
        _same(whole.features, _want(x, np.arange(12), TAPS65, reference, sample, np.zeros(300, int), 7, 12, 12, basis))
        # a 1-D basis: no P axis, the same bytes as the one-row basis
        one = r.waveform_features(sample, basis[2], channel, before=7, after=12, neighbours=2, taps=TAPS65, reference=reference)
        assert one.features.shape == (300, 5) and one.basis.shape == (1, 19)
        _same(one.features, got.features[:, 2])
    # a float64 basis is rounded once, and the Bunch holds what was used; ints are taken
    b64 = np.random.RandomState(1).standard_normal((2, 19))
    got = r.waveform_features(sample, b64, before=7, after=12)
    assert got.basis.dtype == np.float32 and np.array_equal(got.basis, b64.astype(np.float32))
    _same(got.features, _want(x, np.arange(12), None, None, sample, np.zeros(300, int), 7, 12, 12, b64.astype(np.float32)))
    r.waveform_features(sample, np.ones((1, 19), int), before=7, after=12)
    # a shuffled channel list with repeats
    cols = [7, 0, 0, 11, 3, 7, 5]
    ch = np.array(cols)[rs.randint(0, 7, 300)]
    first = np.array([cols.index(c) for c in ch])
    got = r.waveform_features(sample, _basis(2, 7), ch, before=3, after=4, neighbours=1, channels=cols, reference='median')
    assert np.array_equal(got.channels, cols)
    _same(got.features, _want(x, cols, None, 'median', sample, first - 1, 3, 4, 3, _basis(2, 7)))
    # no events: no device call
    codec.waveform_features_calls.clear()
    none = r.waveform_features(np.zeros(0, np.int64), _basis(3, 61), np.zeros(0, np.int64), neighbours=3)
    assert none.features.shape == (0, 3, 7) and none.features.dtype == np.float32 and not codec.waveform_features_calls
    assert r.waveform_features(np.zeros(0, np.int64), _basis(3, 61)[0]).features.shape == (0, 12)
    r.close()


def test_call_cuts_and_lanes_give_identical_bytes(tmp_cfg, monkeypatch):
    x = synth_int16(0, 9000, 8, 5)
    codec = _codec()
    one = _write(tmp_cfg, x, codec)
    rs = np.random.RandomState(2)
    sample, channel = rs.randint(0, 9000, 400), rs.randint(0, 8, 400)
    basis = _basis(4, 23)
    kw = dict(before=9, after=14, neighbours=3, taps=TAPS65, reference='median')
    whole = one.waveform_features(sample, basis, channel, **kw).features
    assert len(codec.waveform_features_calls) == 1 and codec.waveform_features_calls[0][3] == 400
    _same(whole, _want(x, np.arange(8), TAPS65, 'median', sample, channel - 3, 9, 14, 7, basis))
    for n_lanes in (2, 3):
        lc = _codec(n_lanes)
        many = mtscomp_amd.decompress(tmp_cfg / 'data.cbin', tmp_cfg / 'data.ch', codec=lc, check_after_decompress=False)
        _same(many.waveform_features(sample, basis, channel, **kw).features, whole)
        assert {c[0] for c in lc.waveform_features_calls} == set(range(n_lanes))
        assert sum(c[3] for c in lc.waveform_features_calls) == 400
        for _, keys, _, _ in lc.waveform_features_calls:               # a lane reads adjacent chunks
            assert keys == list(range(keys[0], keys[-1] + 1))
        many.close()
    codec.waveform_features_calls.clear()
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1)
    _same(one.waveform_features(sample, basis, channel, **kw).features, whole)
    assert len(codec.waveform_features_calls) >= 8 and sum(c[3] for c in codec.waveform_features_calls) == 400
    monkeypatch.setattr(api, 'WAVEFORMS_CALL_BYTES', 1 << 30)
    codec.waveform_features_calls.clear()
    monkeypatch.setattr(api, 'WAVEFORMS_OUT_BYTES', 30 * 4 * 4 * 7)    # 4 P W bytes an event: 30 events a call
    _same(one.waveform_features(sample, basis, channel, **kw).features, whole)
    assert [c[3] for c in codec.waveform_features_calls] == [30] * 13 + [10]
    one.close()


def test_reads_resident_chunks_in_place_and_keeps_nothing(tmp_cfg):
    x = synth_int16(0, 6000, 6, 7)
    codec = _codec()
    r = _write(tmp_cfg, x, codec)
    cache = r._cache_for(0)
    sample = np.arange(50, 6000, 97)
    basis = _basis(3, 61)
    cold = r.waveform_features(sample, basis, taps=TAPS65).features
    assert not codec.caches[cache]                                     # a projection inserts nothing
    r[2100:2200]
    resident = sorted(codec.caches[cache])
    assert resident
    codec.waveform_features_calls.clear()
    warm = r.waveform_features(sample, basis, taps=TAPS65).features
    assert sorted(codec.caches[cache]) == resident
    (_, keys, lens, _), = codec.waveform_features_calls
    assert [k for k, n in zip(keys, lens) if n == 0] == resident
    _same(warm, cold)
    # an entry dropped between the query and the call: E_MISS, then everything is sent once more
    codec.waveform_features_calls.clear()
    codec.miss_next_waveform_features = True
    _same(r.waveform_features(sample, basis, taps=TAPS65).features, cold)
    (_, _, lens_a, _), (_, _, lens_b, _) = codec.waveform_features_calls
    assert 0 in lens_a and all(lens_b)
    # a sparse list reads only its chunks
    codec.waveform_features_calls.clear()
    r.waveform_features([5400, 300], basis, taps=TAPS65)
    assert sorted(c[1] for c in codec.waveform_features_calls) == [[0], [5]]
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
    basis = _basis(2, 61)
    r.waveform_features([300, 5400], basis, taps=TAPS65)               # chunks 0 and 5: chunk 3 is not read
    with pytest.raises(IOError, match='#3'):
        r.waveform_features([300, 3500], basis)
    r.close()


def test_argument_errors(tmp_cfg):
    x = synth_int16(0, 2000, 5, 9)
    r = _write(tmp_cfg, x, _codec())
    ok = dict(sample=[10, 20], basis=_basis(3, 61), channel=[0, 1], neighbours=1)
    r.waveform_features(**ok)
    for bad in (dict(sample=[-1, 5]), dict(sample=[2000, 5]), dict(sample=[[1, 2]]), dict(sample=[1.0, 2.0]),
                dict(before=-1), dict(before=0, after=0), dict(before=4000, after=97), dict(after=True),
                dict(neighbours=-1), dict(neighbours=512), dict(channel=None), dict(channel=[0]), dict(channel=[0, 5]),
                dict(channels=[0, 2, 3]), dict(channels=[]), dict(reference='mean'), dict(taps=[]), dict(taps=[np.nan])):
        with pytest.raises(ValueError):
            r.waveform_features(**{**ok, **bad})
    shape = r"basis must be a \(P, 61\) or \(61,\) array of numbers \(before \+ after = 61\), got shape "
    for bad, text in ((_basis(3, 60), shape + r"\(3, 60\)"), (_basis(61, 3), shape), (np.zeros((1, 3, 61)), shape), (np.float32(1.0), shape),
                      (None, shape), (np.zeros((2, 61), complex), shape), ([['a'] * 61], shape), (np.zeros((0, 61)), "at most 32 components"),
                      (_basis(33, 61), r"at most 32 components and 8192 basis entries \(components x rows\), got 33 and 2013")):
        with pytest.raises(ValueError, match=text):
            r.waveform_features(**{**ok, 'basis': bad})
    with pytest.raises(ValueError, match="got 9 and 8199"):            # P * T over the limit with P within it
        r.waveform_features([1000], _basis(9, 911), before=500, after=411)
    r.waveform_features([1000], _basis(8, 1024), before=500, after=524)             # 8192 entries: taken
    r.waveform_features([1000], _basis(32, 61))
    for v in (np.nan, np.inf, -np.inf, 1e39):                           # 1e39 is finite as float64, inf as float32
        b = _basis(3, 61).astype(np.float64)
        b[1, 7] = v
        with pytest.raises(ValueError, match="basis must be finite as float32"):
            r.waveform_features(**{**ok, 'basis': b})
    assert (hip.FEATURES_MAX_COMPONENTS, hip.FEATURES_MAX_BASIS) == (32, 8192)
    r.close()


def test_needs_a_device_codec(tmp_cfg):
    r = _write(tmp_cfg, synth_int16(0, 2000, 3, 0), OracleCodec())
    with pytest.raises(NotImplementedError):
        r.waveform_features([10], _basis(1, 61))
    r.close()


def test_exports_are_listed():
    assert {'mts_waveform_features', 'mts_dev_waveform_features'} <= set(hip.EXPORTS)
    assert callable(api.HipCodec.waveform_features) and callable(hip.waveform_features) and callable(hip.dev_waveform_features)


# ---- api.waveform_basis -----------------------------------------------------------------------------------------------------------
def _separated(rs, n, T, W, sing):
    """(n, T, W) snippets whose columns have the singular values `sing` along known orthonormal directions, and those directions."""
    q, _ = np.linalg.qr(rs.standard_normal((T, T)))
    u, _ = np.linalg.qr(rs.standard_normal((n * W, T)))
    cols = (u * np.asarray(sing)) @ q.T                                # (n W, T): V = q
    return cols.reshape(n, W, T).transpose(0, 2, 1).copy(), q.T


def test_waveform_basis_is_orthonormal_and_matches_the_svd():
    rs = np.random.RandomState(7)
    T, sing = 12, 100.0 * 0.5 ** np.arange(12)                        # well separated
    w, _ = _separated(rs, 40, T, 5, sing)
    for P in (1, 3, 12):
        b = api.waveform_basis(w, P)
        assert b.shape == (P, T) and b.dtype == np.float32 and b.flags.c_contiguous
        assert np.abs(b.astype(np.float64) @ b.astype(np.float64).T - np.eye(P)).max() <= 1e-5
        v = np.linalg.svd(w.transpose(0, 2, 1).reshape(-1, T), full_matrices=False)[2][:P]
        assert np.abs(np.abs(b.astype(np.float64) @ v.T) - np.eye(P)).max() <= 1e-5
        # the sign rule: the entry of largest magnitude is positive
        top = np.abs(b).argmax(axis=1)
        assert (b[np.arange(P), top] > 0).all()
    assert api.waveform_basis(w).shape == (3, T)                        # the default
    # float32 snippets, and a 2-D (T, W) array, and the mean of mean_waveforms (K, T, W): any (..., T, W)
    assert np.abs(api.waveform_basis(w.astype(np.float32), 3) - api.waveform_basis(w, 3)).max() <= 1e-5
    assert api.waveform_basis(w[0], 2).shape == (2, T)
    assert np.array_equal(api.waveform_basis(w.reshape(8, 5, T, 5), 3), api.waveform_basis(w, 3))


def test_waveform_basis_sign_rule_on_a_tie_and_dropped_columns():
    # one direction with two entries of the same magnitude: the first decides the sign
    v = np.zeros((1, 4, 2))
    v[0, :, 0] = [0.0, -2.0, 2.0, 1.0]
    v[0, :, 1] = [0.0, -4.0, 4.0, 2.0]
    b = api.waveform_basis(v, 1)
    assert b[0, 1] > 0 and b[0, 2] < 0 and abs(b[0, 1]) == abs(b[0, 2])
    # columns with a NaN are dropped: the basis of the rest
    rs = np.random.RandomState(3)
    w, _ = _separated(rs, 30, 8, 4, 50.0 * 0.5 ** np.arange(8))
    holed = w.copy()
    holed[3, 2, 1] = np.nan
    holed[7, :, 0] = np.nan
    keep = np.ones((30, 4), bool)
    keep[3, 1] = keep[7, 0] = False
    rest = w.transpose(0, 2, 1)[keep]                                  # (n_kept, T)
    assert np.array_equal(api.waveform_basis(holed, 3), api.waveform_basis(rest.T[None], 3))
    assert not np.array_equal(api.waveform_basis(holed, 3), api.waveform_basis(w, 3))


def test_waveform_basis_errors():
    w = np.random.RandomState(0).standard_normal((5, 6, 2))
    for bad in (dict(n_components=0), dict(n_components=7), dict(n_components=2.0), dict(n_components=True), dict(n_components=None)):
        with pytest.raises(ValueError, match="n_components must be an int in \\[1, 6\\]"):
            api.waveform_basis(w, **bad)
    for bad in (np.zeros(6), np.float64(1.0), np.zeros((3, 0, 2)), np.array([['a', 'b']])):
        with pytest.raises(ValueError, match="waveforms must be a"):
            api.waveform_basis(bad)
    few = np.full((1, 6, 4), np.nan)
    few[0, :, :2] = 1.0
    with pytest.raises(ValueError, match="3 components need at least as many columns without a NaN, got 2"):
        api.waveform_basis(few, 3)
    assert api.waveform_basis(few, 2).shape == (2, 6)
    with pytest.raises(ValueError, match="got 0"):
        api.waveform_basis(np.zeros((0, 6, 4)), 1)
    w[0, 0, 0] = np.inf
    with pytest.raises(ValueError, match="finite or NaN"):
        api.waveform_basis(w, 1)
