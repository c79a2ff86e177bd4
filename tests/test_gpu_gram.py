"""Reader.cov and mts_gram / mts_dev_gram on the MI355X: the fp64 MFMA Gram kernel against tests/gram_oracle.py over the oracle's decode
of the golden files, exact extremes across a group boundary, integer-valued float data, float data within the bound and bit for bit
across column sets, lanes, calls and residency, column counts that exercise partial and diagonal tiles, special floats, the
configs[1] recording in HBM, the cache, damaged chunks and argument errors."""
import ctypes as C
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.gram_oracle import check_cov_result, exact_gram, tree_height
from tests.test_golden import CASES, golden_cbin
from tests.test_gpu_window_stats import _hbm_recording, _oracle_decode

pytestmark = pytest.mark.gpu

E_ARG = -1
ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = sorted(n for n, c in CASES.items() if golden_cbin(c) is not None)


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _file(tmp, x, rate=1000., chunk_duration=1., codec=None, **kw):
    raw = tmp / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'd.cbin', tmp / 'd.ch', sample_rate=rate, n_channels=x.shape[1], dtype=x.dtype,
                         chunk_duration=chunk_duration, check_after_compress=False, **kw)
    return _open(tmp, codec)


def _open(tmp, codec=None):
    return mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', codec=codec, check_after_decompress=False)


def _cols(channels, nc):
    return list(range(*channels.indices(nc))) if isinstance(channels, slice) else [int(c) % nc for c in channels]


@pytest.mark.parametrize('name', GOLDEN)
def test_golden_files(name, tmp_cfg):
    case = CASES[name]
    hdr = json.loads(case['ch_text'])
    p = tmp_cfg / (name + '.cbin')
    p.write_bytes(golden_cbin(case))
    r = mtscomp_amd.Reader(check_after_decompress=False)
    r.open(p, cmeta=hdr)
    dec = _oracle_decode(case)
    nc, n = hdr['n_channels'], hdr['shape'][0]
    shuffled = list(np.random.RandomState(len(name)).permutation(nc)) + [0, nc - 1, 0]
    chunk_len = hdr['chunk_bounds'][1] - hdr['chunk_bounds'][0]
    worst = 0.0
    for window in (1, 7, chunk_len, 3001, n + 5, None):
        for channels in (slice(None), slice(1, None, 3), shuffled):
            cols = _cols(channels, nc)
            if not cols:
                continue
            got = r.cov(channels=channels, window=window)
            worst = max(worst, check_cov_result(got, dec[:, cols], 0, n, window))
    got = r.cov(-n // 2, -1, channels=[nc - 1], window=1000, ddof=0)
    check_cov_result(got, dec[:, [nc - 1]], n - n // 2, n - 1, 1000, ddof=0)
    print('%s: largest error / allowance %.3g' % (name, worst))
    r.close()


def test_exact_extremes_across_a_group_boundary(tmp_cfg):
    rows = (1 << 20) + 1000
    x = np.zeros((rows, 5), np.int16)
    x[:, 0] = -32768
    x[:, 1] = np.where(np.arange(rows) % 2, 32767, -32768)
    x[:, 2] = 32767
    x[:, 3] = -32768
    x[:, 4] = (np.random.RandomState(1).randn(rows) * 9000).clip(-32768, 32767).astype(np.int16)
    r = _file(tmp_cfg, x, rate=30000., chunk_duration=3.3)
    a = x.astype(np.int64)
    want = a.T @ a
    for window in (None, rows, (1 << 20) + 1, 1 << 19, 300001):
        got = r.cov(window=window)
        w = window or rows
        for k in range(len(got.count)):
            b = a[k * w:(k + 1) * w]
            assert np.array_equal(got.gram[k], b.T @ b), window
            assert np.array_equal(got.sum[k], b.sum(0)), window
        if window in (None, rows):
            assert np.array_equal(got.gram[0], want)
    got = r.cov(channels=[3, 1, 3, 0])
    assert np.array_equal(got.gram[0], want[np.ix_([3, 1, 3, 0], [3, 1, 3, 0])])
    r.close()
    u = np.full((rows, 3), 65535, np.uint16)
    u[:, 1] = np.random.RandomState(2).randint(0, 65536, rows)
    r = _file(tmp_cfg, u, rate=30000., chunk_duration=3.3)
    a = u.astype(np.int64)
    got = r.cov()
    assert got.gram.dtype == np.int64 and np.array_equal(got.gram[0], a.T @ a)
    assert got.gram[0, 0, 0] == rows * 65535 ** 2 and np.array_equal(got.sum[0], a.sum(0))
    r.close()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_integer_valued_float_data_is_exact(tmp_cfg, dtype):
    rows = 3 * (1 << 20) // 2                                    # (< 2^22 rows of |x| <= 2^15: every partial sum is exact)
    rs = np.random.RandomState(3)
    x = rs.randint(-(1 << 15), (1 << 15) + 1, size=(rows, 4)).astype(dtype)
    x[:, 3] = -(1 << 15)
    r = _file(tmp_cfg, x, rate=30000., chunk_duration=5.0)
    dec = r[:]
    assert np.array_equal(dec, x)
    for window in (None, 100000, 1 << 20):
        got = r.cov(window=window)
        w = window or rows
        for k in range(len(got.count)):
            b = x[k * w:(k + 1) * w]
            assert got.gram[k].tobytes() == exact_gram(b.astype(np.int32)).astype(np.float64).tobytes()
    r.close()


def test_float_data_bound_and_bit_identity(tmp_cfg, monkeypatch):
    rows, nc = (1 << 20) + 70000, 7
    rs = np.random.RandomState(4)
    x = (rs.randn(rows, nc) * 30 + rs.randn(nc) * 5000).astype(np.float32)
    r = _file(tmp_cfg, x, rate=30000., chunk_duration=3.7, codec=api.HipCodec(devices=[0]), do_time_diff=False)
    dec = r[:]
    base = r.cov(5, None)
    print('largest error / allowance %.3g (h = %d)' % (check_cov_result(base, dec, 5, rows, None), tree_height(rows - 5)))
    G = base.gram[0]
    for cols in ([3], [6, 0], [2, 2, 5, 0, 2], list(range(nc))[::-1]):
        g = r.cov(5, None, channels=cols).gram[0]
        assert g.tobytes() == np.ascontiguousarray(G[np.ix_(cols, cols)]).tobytes(), cols
    two = _open(tmp_cfg, api.HipCodec(devices=[0, 0]))
    for window in (None, 1 << 20, 400000, 4096 * 3 + 5):
        a = r.cov(5, None, window=window)
        b = two.cov(5, None, window=window)
        assert a.gram.tobytes() == b.gram.tobytes() and a.sum.tobytes() == b.sum.tobytes() and a.cov.tobytes() == b.cov.tobytes()
        if window == 400000:
            check_cov_result(a, dec, 5, rows, window)
    monkeypatch.setattr(api, 'GRAM_CALL_BYTES', 1)             # one call per group
    c = two.cov(5, None)
    assert c.gram.tobytes() == base.gram.tobytes() and c.sum.tobytes() == base.sum.tobytes()
    monkeypatch.setattr(api, 'GRAM_CALL_BYTES', 1 << 30)
    r.close()
    two.close()
    r = _open(tmp_cfg, api.HipCodec(devices=[0]))               # (a fresh reader: nothing in its host LRU, so slices go to the device)
    for k in range(2, 7):                                        # some chunks resident
        r[r.chunk_bounds[k]:r.chunk_bounds[k] + 3]
    keys = list(range(r.n_chunks))
    before = hip.cache_query(r._cache_for(0), keys).tolist()
    assert sum(int(q) >= nc for q in before) >= 4
    warm = r.cov(5, None)
    assert warm.gram.tobytes() == base.gram.tobytes() and warm.sum.tobytes() == base.sum.tobytes()
    assert hip.cache_query(r._cache_for(0), keys).tolist() == before
    r.close()


@pytest.mark.parametrize('dtype', ['int16', 'float32'])
def test_column_counts(tmp_cfg, dtype):
    nc, rows = 385, 9001
    rs = np.random.RandomState(5)
    x = (rs.randn(rows, nc) * 3000).clip(-32768, 32767)
    x = x.astype(np.int16) if dtype == 'int16' else (x + 1000).astype(np.float32)
    r = _file(tmp_cfg, x, rate=3000., chunk_duration=1.0, do_time_diff=dtype == 'int16')
    dec = r[:]
    full = r.cov()
    check_cov_result(full, dec, 0, rows, None)
    for k in (1, 15, 16, 17, 31, 33, 65, 385):
        cols = sorted(rs.choice(nc - 1, k - 1, replace=False).tolist()) + [nc - 1]
        rs.shuffle(cols)
        got = r.cov(channels=cols, window=4000)
        check_cov_result(got, dec[:, cols], 0, rows, 4000)
        g = r.cov(channels=cols).gram[0]
        assert g.tobytes() == np.ascontiguousarray(full.gram[0][np.ix_(cols, cols)]).tobytes(), k
    r.close()


def test_special_floats(tmp_cfg):
    rs = np.random.RandomState(6)
    x = (rs.randn(9000, 6) * 10).astype(np.float32)
    x[1000, 1] = np.nan
    x[3000, 2] = np.inf
    x[4500, 3] = -np.inf
    x[5000, 4], x[5001, 4] = np.inf, -np.inf
    x[:, 5] = 0
    x[4500, 5] = 1.0                                             # -inf * 1 in (3, 5)
    r = _file(tmp_cfg, x, do_time_diff=False)
    dec = r[:]
    assert np.array_equal(dec, x, equal_nan=True)
    for window in (None, 2000, 1):
        got = r.cov(window=window)
        check_cov_result(got, dec, 0, 9000, window)
    g = r.cov().gram[0]
    xf = x.astype(np.float64)
    want = xf.T @ xf
    assert np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(np.isinf(g), np.isinf(want))
    assert np.array_equal(g[np.isinf(g)], want[np.isinf(want)])
    assert np.isnan(g[1]).all() and g[2, 2] == np.inf and g[3, 5] == -np.inf and g[4, 4] == np.inf
    r.close()


def test_config1_in_hbm_bit_identical():
    """configs[1] (60 s x 385 int16) in HBM: mts_dev_gram with every column, window None and 30000, against numpy int64 by blocked
    float64 BLAS; then a range that starts and ends inside chunks, 50 shuffled columns, a call on a run of groups that begins after
    the first one with only the chunks those groups read."""
    nc = 385
    raw, cbuf, slots, sizes, bounds = _hbm_recording(nc=nc)
    x = raw.download(dtype=np.int16).reshape(-1, nc)
    n = x.shape[0]
    flags = hip.make_flags(True, False, 'F')
    rows = np.diff(bounds)
    out = None
    st, got, s, out = hip.dev_gram(cbuf, slots, sizes, bounds[:-1], rows, nc, np.int16, flags, 0, n, n, 0, 2, np.arange(nc), out=out)
    assert st == [0] * len(rows) and got.shape == (2, nc, nc) and got.dtype == np.int64
    want = exact_gram(x)
    assert np.array_equal(got[0] + got[1], want)
    assert np.array_equal(got[0], exact_gram(x[:1 << 20]))
    assert np.array_equal(s.sum(0), x.astype(np.int64).sum(0))
    n_win = n // 30000
    st, got, s, out = hip.dev_gram(cbuf, slots, sizes, bounds[:-1], rows, nc, np.int16, flags, 0, n, 30000, 0, n_win, np.arange(nc), out=out)
    assert st == [0] * len(rows)
    assert np.array_equal(got.sum(axis=0), want)
    for w in (0, 17, n_win - 1):
        assert np.array_equal(got[w], exact_gram(x[w * 30000:(w + 1) * 30000]))
    cols = np.random.RandomState(2).permutation(nc)[:50]
    rb, re, win = 12345, n - 777, 4567
    ng = hip.gram_groups(rb, re, win)
    g0, g1 = 3, ng - 2
    lo, hi = hip.gram_group_rows(rb, re, win, g0)[0], hip.gram_group_rows(rb, re, win, g1 - 1)[1]
    c0 = int(np.searchsorted(bounds, lo, 'right')) - 1
    c1 = int(np.searchsorted(bounds, hi - 1, 'right')) - 1
    k = slice(c0, c1 + 1)
    st, got, s, _ = hip.dev_gram(cbuf, slots[k], sizes[k], bounds[k], rows[k], nc, np.int16, flags, rb, re, win, g0, g1, cols)
    assert st == [0] * (c1 - c0 + 1)
    for j, g in enumerate(range(g0, g1)):
        a, b = hip.gram_group_rows(rb, re, win, g)
        assert np.array_equal(got[j], exact_gram(x[a:b, cols])), g
        assert np.array_equal(s[j], x[a:b, cols].astype(np.int64).sum(0)), g


def test_cache_untouched_by_a_scan_resident_equals_cold_and_e_miss(tmp_cfg):
    nc, seconds, rate = 64, 6, 10000
    x = (np.random.RandomState(7).randn(seconds * rate, nc) * 1000).astype(np.int16)
    r = _file(tmp_cfg, x, rate=float(rate))
    keys = list(range(seconds))
    r[rate + 5:rate + 10]                                        # chunk 1 (and what is read ahead) resident
    cache = r._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert before[1] == nc
    warm = r.cov(window=7000)
    assert hip.cache_query(cache, keys).tolist() == before      # a whole-file scan changes nothing in the cache
    check_cov_result(warm, x, 0, x.shape[0], 7000)
    data = (tmp_cfg / 'd.cbin').read_bytes()
    offs = np.array(r.chunk_offsets[:-1])
    lens = np.diff(r.chunk_offsets)
    bounds = np.array(r.chunk_bounds)
    flags = r._flags()
    resident = [k for k, p in zip(keys, before) if p]
    lens_w = np.where(np.isin(keys, resident), 0, lens)
    n = x.shape[0]
    ng = hip.gram_groups(0, n, 3001)
    st_w, a, sa = hip.gram(cache, keys, bounds[:-1], data, offs, lens_w, np.diff(bounds), nc, np.int16, flags, 0, n, 3001, 0, ng, range(nc))
    st_c, b, sb = hip.gram(0, keys, bounds[:-1], data, offs, lens, np.diff(bounds), nc, np.int16, flags, 0, n, 3001, 0, ng, range(nc))
    assert st_w == st_c == [0] * seconds
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()
    assert hip.cache_query(cache, keys).tolist() == before
    cold = [k for k in keys if k not in resident][0]
    lens_bad = lens_w.copy()
    lens_bad[cold] = 0
    with pytest.raises(hip.HipError) as e:
        hip.gram(cache, keys, bounds[:-1], data, offs, lens_bad, np.diff(bounds), nc, np.int16, flags, 0, n, 3001, 0, ng, range(nc))
    assert e.value.code == hip.E_MISS
    r.close()


_PIECES_SCRIPT = '''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import mtscomp_amd
from mtscomp_amd import api, hip
r = mtscomp_amd.decompress(sys.argv[2], sys.argv[3], codec=api.HipCodec(devices=[0]), check_after_decompress=False)
n, b = r.n_samples, r.chunk_bounds
keys = list(range(len(b) - 1))
cache = r._cache_for(0)
out = {}
def run(tag):
    for i, (w, lo, hi) in enumerate(((None, 0, n), (4321, 1234, n - 77))):
        c = r.cov(lo, hi, window=w)
        for k in ('count', 'sum', 'gram', 'mean', 'cov'):
            out['%s_%s_%d' % (tag, k, i)] = c[k]
assert not any(hip.cache_query(cache, keys).tolist())
run('cold')
assert not any(hip.cache_query(cache, keys).tolist())             # (a scan inserts nothing)
r[b[3] + 5:b[4] + 7]               # chunks 3, 4 and 9: a resident run between missing chunks, missing runs after a resident chunk
r[b[9] + 1:b[9] + 3]
assert [k for k, p in zip(keys, hip.cache_query(cache, keys).tolist()) if p] == [3, 4, 9]
run('part')
np.savez(sys.argv[4], **out)
'''


@pytest.mark.parametrize('dtype', ['int16', 'float32'])
def test_cov_pieces_and_residency_do_not_change_the_result(tmp_cfg, dtype):
    """MTS_PIPE_BYTES unset (one piece) and two chunks a piece (>= 5 pieces), each cold and with chunks 3, 4 and 9 of 12 resident:
    every output of Reader.cov is the same bytes, and right by the oracle."""
    rows, nc = 12 * 3000, 40
    x = (np.random.RandomState(8).randn(rows, nc) * 300).astype(dtype)
    assert hip.gram_groups(1234, rows - 77, 4321) > 1 and 4321 < hip.GRAM_GROUP_ROWS        # the windowed call: several groups
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=3000., n_channels=nc, dtype=dtype,
                         do_time_diff=dtype != 'float32', check_after_compress=False)
    script = tmp_cfg / 'pieces.py'
    script.write_text(_PIECES_SCRIPT)
    outs = []
    for pipe in (None, str(2 * 3000 * nc * np.dtype(dtype).itemsize)):         # one piece; two chunks a piece: >= 5 pieces
        env = dict(os.environ)
        env.pop('MTS_PIPE_BYTES', None)
        env['HOME'] = str(tmp_cfg)
        env['MTSCOMP_READ_AHEAD'] = '0'                                        # (exactly the chunks touched become resident)
        if pipe:
            env['MTS_PIPE_BYTES'] = pipe
        p = tmp_cfg / ('o%d.npz' % len(outs))
        subprocess.run([sys.executable, str(script), str(ROOT), str(tmp_cfg / 'd.cbin'), str(tmp_cfg / 'd.ch'), str(p)], env=env,
                       check=True, timeout=300)
        outs.append(dict(np.load(p)))
    assert sorted(outs[0]) == sorted(outs[1]) and len(outs[0]) == 20
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
        if k.startswith('part_'):
            assert outs[1][k].tobytes() == outs[1]['cold_' + k[5:]].tobytes(), k
    for i, (w, lo, hi) in enumerate(((None, 0, rows), (4321, 1234, rows - 77))):
        got = type('B', (), {k: outs[1]['part_%s_%d' % (k, i)] for k in ('count', 'sum', 'gram', 'mean', 'cov')})
        check_cov_result(got, x, lo, hi, w)


def test_damaged_chunk(tmp_cfg):
    nc, rows = 16, 5 * 3000
    x = (np.random.RandomState(8).randn(rows, nc) * 1000).astype(np.int16)
    r = _file(tmp_cfg, x, rate=3000.)
    r.close()
    hdr = json.loads((tmp_cfg / 'd.ch').read_text())
    o = hdr['chunk_offsets']
    data = bytearray((tmp_cfg / 'd.cbin').read_bytes())
    data[o[2] + 30:o[2] + 60] = b'\x00' * 30
    (tmp_cfg / 'd.cbin').write_bytes(bytes(data))
    r = _open(tmp_cfg)
    with pytest.raises(IOError, match='#2'):
        r.cov(window=1000)
    got = r.cov(0, 6000)                                         # chunks 0 and 1 only
    check_cov_result(got, x, 0, 6000, None)
    b = np.array(hdr['chunk_bounds'])
    st, g, s = hip.gram(0, range(5), b[:-1], bytes(data), o[:-1], np.diff(o), np.diff(b), nc, np.int16, r._flags(), 0, rows, 1000, 0, 15,
                        range(nc))
    assert st == [0, 0, hip.CHUNK_CORRUPT, 0, 0]                 # only that chunk
    a = x.astype(np.int64)
    for w in list(range(6)) + list(range(9, 15)):
        assert np.array_equal(g[w], a[w * 1000:(w + 1) * 1000].T @ a[w * 1000:(w + 1) * 1000])
    r.close()


def test_c_abi_argument_errors():
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = np.arange(800, dtype=np.int16).reshape(200, nc)
    zs = hip.compress_chunks(x, [0, 100, 200], hip.make_flags(), 6)
    data = np.frombuffer(zs[0] + zs[1] + b'\0' * 16, dtype=np.uint8)
    dbuf = hip.DevBuffer(data.size + 256)
    dbuf.upload(data)
    keep = []
    outd = hip.DevBuffer(1 << 20)

    def call(dev, row0=(0, 100), rows=(100, 100), rb=0, re=200, window=10, g0=0, g1=20, cols=(0, 1), itemsize=2, flags=hip.make_flags()):
        a = [np.array(v, dtype=np.int64) for v in ([0, 1], list(row0), [0, len(zs[0])], [len(zs[0]), len(zs[1])], list(rows))]
        c = np.array(cols, dtype=np.int32)
        og, os_ = np.zeros(1 << 16, np.uint8), np.zeros(1 << 14, np.uint8)
        st = np.full(2, 99, np.int32)
        keep.append((a, c, og, os_, st))
        P = lambda v: v.ctypes.data_as(C.POINTER(C.c_long))  # noqa: E731
        if dev:
            rc = L.mts_dev_gram(0, None, dbuf.at(), P(a[2]), P(a[3]), P(a[1]), P(a[4]), 2, nc, itemsize, flags, rb, re, window, g0, g1, len(c),
                                c.ctypes.data_as(C.POINTER(C.c_int)), outd.at(), outd.at(1 << 19), st.ctypes.data_as(C.POINTER(C.c_int)))
        else:
            rc = L.mts_gram(0, 0, 2, P(a[0]), P(a[1]), data.ctypes.data_as(C.c_void_p), P(a[2]), P(a[3]), P(a[4]), nc, itemsize, flags, rb, re,
                            window, g0, g1, len(c), c.ctypes.data_as(C.POINTER(C.c_int)), og.ctypes.data_as(C.c_void_p),
                            os_.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.POINTER(C.c_int)))
        return rc, int(st[0])
    for dev in (False, True):
        assert call(dev) == (0, 0)
        assert call(dev, g0=5, g1=6, rb=30, re=170) == (0, 0)
        for bad in (dict(cols=()), dict(cols=(0, 4)), dict(cols=(-1,)), dict(window=0), dict(window=-3), dict(g0=3, g1=3),
                    dict(g0=5, g1=4), dict(g0=-1), dict(g1=21), dict(rb=50, re=20), dict(rb=10, re=10), dict(rb=-5),
                    dict(row0=(0, 101)), dict(row0=(50, 150)), dict(rb=0, re=300, g1=30), dict(rows=(0, 100)), dict(itemsize=3),
                    dict(flags=hip.FLAG_FLOAT, itemsize=2), dict(cols=tuple([0] * (hip.GRAM_MAX_COLS + 1)))):
            rc, st = call(dev, **bad)
            assert rc == E_ARG, (dev, bad)                         # MTS_E_ARG ...
            assert st == 99, (dev, bad)                            # ... before anything ran
