"""Reader.cov(taps=, reference=) and mts_filtered_gram / mts_dev_filtered_gram on the MI355X: k_zgram and its z-slab loop.

The contract is bit-identity with the existing kernel on the same items: a recording is filtered on the device (residual([], ...), whose
bytes are z), the float32 rows are written as a float32 recording, and cov of that file (k_gram<float> + k_gram_colsum) must equal
cov(taps=, reference=) of the original in every bit of gram and sum, NaN entries at the same places (payload aside).  Beside that:
exactness on integers, the group seam, gram_oracle's bound on the oracle's z (tests/filtered_select_oracle.py), the seams of the host
loop, the limits and refusals, NaN and infinity.  Shapes: 2 * 4096 + 5 rows (two whole Gram slabs and a tail of 5) in chunks of 3000,
so that chunk boundaries fall inside Gram slabs; columns 1, 5, 64, 65, 130 (1, 1, 1, 3, 6 super-tile pairs; n_cols % 4 of 1, 1, 0, 1, 2:
the float, float4 and float2 staging)."""
import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.filtered_select_oracle import z_rows
from tests.gram_oracle import assert_gram_within, check_cov_result, tree_height

pytestmark = pytest.mark.gpu

E_ARG = -1
SR = hip.GRAM_SLAB_ROWS
ROWS, NC, CHUNK = 2 * SR + 5, 130, 3000
TAPS = {1: [1.0], 21: api.highpass_taps(300, 30000, 21), 101: api.highpass_taps(300, 30000, 101)}


def _compress(d, x, chunk, **kw):
    """(a module fixture cannot take monkeypatch: the config path is set and put back by hand)"""
    x.tofile(d / 'd.bin')
    api.CONFIG_PATH, keep = d / '.mtscomp', api.CONFIG_PATH
    try:
        mtscomp_amd.compress(d / 'd.bin', d / 'd.cbin', d / 'd.ch', sample_rate=float(chunk), n_channels=x.shape[1], dtype=x.dtype,
                             chunk_duration=1.0, check_after_compress=False, **kw)
    finally:
        api.CONFIG_PATH = keep
    (d / 'd.bin').unlink()


def _open(d, codec=None):
    return mtscomp_amd.decompress(d / 'd.cbin', d / 'd.ch', codec=codec, check_after_decompress=False)


def _int16(rows, nc, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(rows, nc) * 900 + rs.randn(nc) * 3000 + 2000 * np.sin(np.arange(rows) / 300.)[:, None]).clip(-32768, 32767).astype(np.int16)
    return x


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """The recordings, written once: name -> (directory, the array)."""
    out = {}
    rs = np.random.RandomState(5)
    f32 = (rs.randn(SR + 300, 6) * 10).astype(np.float32)
    f32[1000, 1] = np.nan
    f32[SR + 100, 2] = np.inf
    for name, x, chunk, kw in (('int16', _int16(ROWS, NC, 1), CHUNK, {}), ('seams', _int16(3 * SR + 1234, 67, 2), 1000, {}),
                               ('wide', _int16(64, 1025, 3), 40, {}), ('float32', f32, 1500, dict(do_time_diff=False))):
        d = tmp_path_factory.mktemp(name)
        _compress(d, x, chunk, **kw)
        out[name] = (d, x)
    return out


@pytest.fixture
def cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)


def _zfile(r, d, cols, taps, reference, chunk):
    """z of the whole recording from the device (residual without events: an existing operation), written as a float32 recording in
    d and opened.  -> (the Reader, z)."""
    z = r.residual([], [], [], np.zeros((1, 1, len(cols)), np.float32), channels=list(cols), before=0, taps=taps, reference=reference)
    assert z.dtype == np.float32 and z.shape == (r.n_samples, len(cols))
    d.mkdir(exist_ok=True)
    _compress(d, np.ascontiguousarray(z), chunk, do_time_diff=False)
    return _open(d), z


def _same_bits(got, want, what=''):
    """gram and sum: NaN entries at the same places (payload aside), every other bit equal."""
    for key in ('gram', 'sum'):
        a, b = got[key], want[key]
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape, (what, key)
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb), (what, key, 'NaN places')
        assert a[~na].tobytes() == b[~nb].tobytes(), (what, key, int((a[~na].view(np.uint64) != b[~nb].view(np.uint64)).sum()))
    assert got.count.tolist() == want.count.tolist()


# (start, stop, window): the whole recording -- the filter reads zeros outside it at both ends -- in one window of 2 * 4096 + 5 rows
# and in windows around the Gram slab; ranges and windows of 1 and 3 rows across a chunk boundary; interior ranges of 4095 and 4097
# rows whose support crosses chunk boundaries, the second with a window that leaves a tail
GRID = [(0, ROWS, None), (0, ROWS, SR), (0, ROWS, SR - 1), (0, ROWS, SR + 1), (CHUNK - 10, CHUNK + 13, 1), (CHUNK - 10, CHUNK + 13, 3),
        (CHUNK - 1, CHUNK, None), (CHUNK - 1, CHUNK + 2, None), (1500, 1500 + SR - 1, None), (37, 37 + SR + 1, None), (2999, ROWS - 11, 2500)]


# the bound, with its teeth, on the oracle's z: the whole recording, and windows with a tail over a range inside it
BOUND_GRID = {(0, ROWS, None), (2999, ROWS - 11, 2500)}


@pytest.mark.parametrize('n_taps,reference', [(1, None), (21, None), (21, 'median'), (101, 'median')])
@pytest.mark.parametrize('k', [1, 5, 64, 65, 130])
def test_bit_for_bit_against_the_unfiltered_kernel(files, cfg, tmp_path, k, n_taps, reference):
    d, x = files['int16']
    rs = np.random.RandomState(k)
    cols = sorted(rs.choice(NC, k, replace=False).tolist()) if k < NC else list(range(NC))
    taps = TAPS[n_taps]
    r = _open(d)
    rz, z = _zfile(r, tmp_path / 'z', cols, taps, reference, CHUNK)
    zo = z_rows(x[:, cols], 0, 0, ROWS, 0, ROWS, taps, 1 if reference else 0)
    assert z.tobytes() == zo.tobytes()                                  # (the device's z is the oracle's)
    for start, stop, window in GRID:
        got = r.cov(start, stop, channels=cols, window=window, taps=taps, reference=reference)
        assert got.reference == reference and got.taps.tolist() == list(taps)
        _same_bits(got, rz.cov(start, stop, window=window), (start, stop, window))
        # every result within the bound of the oracle's z; the teeth where a window is long enough for them (k > 1: a single
        # column may hold a z near 0, which no bound of this form can see)
        check_cov_result(got, zo, start, stop, window, teeth=(start, stop, window) in BOUND_GRID and k > 1)
    rz.close()
    r.close()


def test_exact_on_integers(files, cfg):
    """taps=[1.0] and no reference: z is float32(x), every partial an integer below 2^53 -- the unfiltered call's int64 results."""
    d, x = files['int16']
    r = _open(d)
    for cols in ([7], list(range(NC)), [3, 3, 129, 0, 64]):
        for start, stop, window in GRID:
            want = r.cov(start, stop, channels=cols, window=window)
            assert want.gram.dtype == np.int64
            for kw in (dict(taps=[1.0]), dict(taps=[1.0], reference=None)):
                got = r.cov(start, stop, channels=cols, window=window, **kw)
                assert got.gram.dtype == np.float64 and got.sum.dtype == np.float64
                assert got.gram.tobytes() == want.gram.astype(np.float64).tobytes() and got.sum.tobytes() == want.sum.astype(np.float64).tobytes()
                assert (got.gram.astype(np.int64) == want.gram).all()
    r.close()


def test_group_seam(cfg, tmp_path):
    """One window of 2^20 + 4097 rows: two groups, the second of one Gram slab and one row."""
    n = hip.GRAM_GROUP_ROWS + SR + 1
    rs = np.random.RandomState(8)
    x = (rs.randn(n, 2) * 700 + 500 * np.sin(np.arange(n) / 50.)[:, None]).astype(np.int16)
    # column 0 alternates +-8000 (+- 100): the taps below turn that into |z| = 9600 (+- 160), 8800 in the first row, so that every row
    # moves the diagonal by far more than the allowance of 2^20 rows -- the bound has its teeth in every row
    x[:, 0] = (8000 * (1 - 2 * (np.arange(n) % 2)) + rs.randint(-100, 101, n)).astype(np.int16)
    (tmp_path / 'x').mkdir()
    _compress(tmp_path / 'x', x, 1 << 18)
    r = _open(tmp_path / 'x')
    taps = [0.1, -0.3, 0.7, -0.3, -0.2]
    rz, z = _zfile(r, tmp_path / 'z', [0, 1], taps, None, 1 << 18)
    got = r.cov(taps=taps)
    assert got.count.tolist() == [n] and hip.gram_groups(0, n, n) == 2
    _same_bits(got, rz.cov(), 'seam')
    zo = z_rows(x, 0, 0, n, 0, n, taps, 0)
    assert z.tobytes() == zo.tobytes()
    assert_gram_within(got.gram[0], zo, tree_height(n))
    rz.close()
    r.close()


def _results(r, cols, windows=(None, 1000, 300)):
    out = []
    for window in windows:
        lo, hi = (0, r.n_samples) if window != 300 else (2950, 5100)
        got = r.cov(lo, hi, channels=cols, window=window, taps=TAPS[21], reference='median')
        out += [got.gram.tobytes(), got.sum.tobytes()]
    return out


def test_seams_of_the_host_loop(files, cfg, tmp_path, monkeypatch):
    """z slabs of exactly one Gram slab (3 Gram slabs and a tail in the group: 4 z slabs), of two, pieces of one chunk with a group or
    several in a chunk, a call per group, two lanes, resident chunks, the device entry, one call against two: the same bytes, and
    right by the bit-for-bit comparison.  A scan inserts nothing."""
    d, x = files['seams']
    n, nc = x.shape
    cols = list(range(nc))
    r = _open(d, api.HipCodec(devices=[0]))
    keys = list(range(r.n_chunks))
    cache = r._cache_for(0)
    base = _results(r, cols)
    assert not any(hip.cache_query(cache, keys).tolist())               # a scan inserts nothing
    rz, _ = _zfile(r, tmp_path / 'z', cols, TAPS[21], 'median', 1000)
    for window in (None, 1000):
        _same_bits(r.cov(channels=cols, window=window, taps=TAPS[21], reference='median'), rz.cov(window=window), window)
    rz.close()
    for slabs in (1, 2):
        monkeypatch.setenv('MTS_ZGRAM_SLAB_BYTES', str(slabs * SR * 4 * nc))
        assert _results(r, cols) == base, slabs
    monkeypatch.setenv('MTS_ZGRAM_SLAB_BYTES', '1')                     # less than a Gram slab: one is kept
    assert _results(r, cols, (None,)) == base[:2]
    monkeypatch.delenv('MTS_ZGRAM_SLAB_BYTES')
    monkeypatch.setenv('MTS_PIPE_BYTES', str(1000 * nc * 2))            # pieces of one chunk: cut between the groups of window=1000,
    monkeypatch.setenv('MTS_BATCH_BYTES', str(1 << 20))                 # several groups of window=300 in a piece
    assert _results(r, cols) == base
    monkeypatch.setenv('MTS_ZGRAM_SLAB_BYTES', str(SR * 4 * nc))
    assert _results(r, cols) == base
    for name in ('MTS_ZGRAM_SLAB_BYTES', 'MTS_PIPE_BYTES', 'MTS_BATCH_BYTES'):
        monkeypatch.delenv(name)
    monkeypatch.setattr(api, 'GRAM_CALL_BYTES', 1)                      # a call per group
    assert _results(r, cols) == base
    monkeypatch.setattr(api, 'GRAM_CALL_BYTES', 1 << 30)
    two = _open(d, api.HipCodec(devices=[0, 0]))                        # two lanes on one device
    assert _results(two, cols) == base
    two.close()
    # the C ABI: one call against the same groups in two, and the device entry
    data = (d / 'd.cbin').read_bytes()
    offs, lens, bounds = np.array(r.chunk_offsets[:-1]), np.diff(r.chunk_offsets), np.array(r.chunk_bounds)
    head = (keys, bounds[:-1], data, offs, lens, np.diff(bounds), nc, np.int16, r._flags())
    mid = (0, n, TAPS[21], cols, 1, 37, n - 11, 2500)
    n_groups = hip.gram_groups(37, n - 11, 2500)
    st, G, S = hip.filtered_gram(0, *head, *mid, 0, n_groups)
    assert st == [0] * len(keys) and G.shape == (n_groups, nc, nc) and S.shape == (n_groups, nc)
    for cut in (1, n_groups - 1):
        _, Ga, Sa = hip.filtered_gram(0, *head, *mid, 0, cut)
        _, Gb, Sb = hip.filtered_gram(0, *head, *mid, cut, n_groups)
        assert Ga.tobytes() + Gb.tobytes() == G.tobytes() and Sa.tobytes() + Sb.tobytes() == S.tobytes()
    cbuf = hip.DevBuffer(len(data) + 256)
    cbuf.upload(np.frombuffer(data, np.uint8))
    st, Gd, Sd, out = hip.dev_filtered_gram(cbuf, offs, lens, bounds[:-1], np.diff(bounds), nc, np.int16, r._flags(), *mid, 0, n_groups)
    assert st == [0] * len(keys) and Gd.tobytes() == G.tobytes() and Sd.tobytes() == S.tobytes()
    out.free()
    cbuf.free()
    # a call with exactly the chunks of its support: group 1 is rows [2537, 5037), 21 taps read 10 rows either side
    k1 = [2, 3, 4, 5]
    h1 = (k1, bounds[k1], data, offs[k1], lens[k1], np.diff(bounds)[k1], nc, np.int16, r._flags())
    st, G1, S1 = hip.filtered_gram(0, *h1, *mid, 1, 2)
    assert st == [0] * 4 and G1.tobytes() == G[1:2].tobytes() and S1.tobytes() == S[1:2].tobytes()
    # resident against cold
    r[1005:1010]
    r[4005:4010]
    before = hip.cache_query(cache, keys).tolist()
    assert before[1] == nc and before[4] == nc
    assert _results(r, cols) == base
    assert hip.cache_query(cache, keys).tolist() == before
    lens_w = np.where(np.array(before) > 0, 0, lens)
    st, Gw, Sw = hip.filtered_gram(cache, keys, bounds[:-1], data, offs, lens_w, *head[5:], *mid, 0, n_groups)
    assert st == [0] * len(keys) and Gw.tobytes() == G.tobytes() and Sw.tobytes() == S.tobytes()
    r.close()


def test_limits_and_refusals(files, cfg, tmp_path):
    """1024 columns with the median reference; MTS_E_ARG for 1025 columns with a reference, a tap that is not finite, a grid outside
    the valid range and chunks short of the support."""
    d, x = files['wide']
    r = _open(d)
    cols = list(range(1024))
    rz, z = _zfile(r, tmp_path / 'z', cols, [0.5, -0.5], 'median', 40)
    got = r.cov(channels=cols, taps=[0.5, -0.5], reference='median')
    _same_bits(got, rz.cov(), 'wide')
    check_cov_result(got, z_rows(x[:, cols], 0, 0, 64, 0, 64, [0.5, -0.5], 1), 0, 64, None)
    rz.close()
    with pytest.raises(ValueError, match='1024'):
        r.cov(reference='median')
    assert r.cov(taps=[1.0]).gram.shape == (1, 1025, 1025)             # without a reference the limit is mts_gram's
    data = (d / 'd.cbin').read_bytes()
    keys = list(range(r.n_chunks))
    offs, lens, bounds = np.array(r.chunk_offsets[:-1]), np.diff(r.chunk_offsets), np.array(r.chunk_bounds)
    head = (keys, bounds[:-1], data, offs, lens, np.diff(bounds), 1025, np.int16, r._flags())

    def refused(*args, head=head):
        with pytest.raises(hip.HipError) as e:
            hip.filtered_gram(0, *head, *args)
        assert e.value.code == E_ARG
    hip.filtered_gram(0, *head, 0, 64, [1.0, 2.0], cols, 1, 0, 64, 64, 0, 1)
    refused(0, 64, [1.0, 2.0], list(range(1025)), 1, 0, 64, 64, 0, 1)                      # 1025 columns with a reference
    refused(0, 64, [1.0, np.inf], cols, 1, 0, 64, 64, 0, 1)                                # a tap that is not finite
    refused(0, 64, [1.0, np.nan], cols, 0, 0, 64, 64, 0, 1)
    refused(0, 64, [1.0], cols, 2, 0, 64, 64, 0, 1)                                        # a reference that is none
    refused(0, 60, [1.0], cols, 1, 0, 64, 64, 0, 1)                                        # a grid outside the valid range
    refused(5, 64, [1.0], cols, 1, 0, 64, 64, 0, 1)
    refused(0, 64, [1.0], cols, 1, 0, 64, 0, 0, 1)                                         # mts_gram's: window_rows, the groups
    refused(0, 64, [1.0], cols, 1, 0, 64, 32, 0, 3)
    refused(0, 64, [1.0], cols, 1, 0, 64, 32, 1, 1)
    # chunks short of the support: rows [40, 64) with 5 taps read rows 38 and 39 of chunk 0
    h1 = ([1], bounds[1:2], data, offs[1:2], lens[1:2], np.diff(bounds)[1:2], 1025, np.int16, r._flags())
    hip.filtered_gram(0, *h1, 0, 64, [1.0], cols, 1, 40, 64, 24, 0, 1)
    refused(0, 64, [0.2] * 5, cols, 1, 40, 64, 24, 0, 1, head=h1)
    r.close()


def test_nan_and_infinity(files, cfg, tmp_path):
    """A float32 recording with one NaN item and, in another window, one +inf.  Without a reference the entries of the NaN's column
    are NaN in this and in the reference path and all others bit-equal; with the median reference every entry of that window is NaN.
    The infinity's column is not finite (21 taps make it +inf and -inf over 21 rows), every other entry is."""
    d, x = files['float32']
    n = len(x)
    cols = list(range(x.shape[1]))
    r = _open(d)
    assert np.array_equal(r[:], x, equal_nan=True)
    for n_taps, reference in ((21, None), (1, None), (21, 'median'), (1, 'median')):
        rz, z = _zfile(r, tmp_path / ('z%d%s' % (n_taps, reference)), cols, TAPS[n_taps], reference, 1500)
        for window in (None, SR):
            got = r.cov(window=window, taps=TAPS[n_taps], reference=reference)
            _same_bits(got, rz.cov(window=window), (n_taps, reference, window))
            check_cov_result(got, z_rows(x, 0, 0, n, 0, n, TAPS[n_taps], 1 if reference else 0), 0, n, window, teeth=False)
        g = got.gram                                                    # windows [0, 4096) -- the NaN -- and [4096, 4396) -- the infinity
        clean = [0, 1, 3, 4, 5]
        if reference:                                                   # the NaN poisons the median of its rows: every column of them
            assert np.isnan(g[0]).all() and np.isnan(got.sum[0]).all()
        else:
            assert np.isnan(g[0][1]).all() and np.isnan(g[0][:, 1]).all() and np.isnan(got.sum[0, 1])
            assert np.isfinite(g[0][[0, 2, 3, 4, 5]][:, [0, 2, 3, 4, 5]]).all()
        # the infinity (a row's median over 6 columns stays finite beside it): its column's entries are not finite -- +inf on the
        # diagonal, +-inf or, from both signs, NaN off it --, all others are
        assert np.isposinf(g[1][2, 2]) and not np.isfinite(g[1][2]).any() and not np.isfinite(g[1][:, 2]).any()
        assert np.isfinite(g[1][clean][:, clean]).all()
        if n_taps == 1:
            assert np.isinf(g[1][2]).all() and np.isposinf(got.sum[1, 2])
        rz.close()
    r.close()
