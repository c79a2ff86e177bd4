"""Reader.quantile / median / mad and mts_rank_hist / mts_dev_rank_hist on the MI355X: the radix-select kernel against
tests/select_oracle.py over the oracle's decode of the golden files, extremes (a constant column, two values, type limits, every int16
value once, window and chunk boundaries inside a tile, the first and last rank), column sets around the wave width, special floats in the
three key modes, the configs[1] recording in HBM, bit-identity across residency, a damaged chunk and argument errors.  Every comparison
is exact: by value for floats, by bytes for integers."""
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
from tests.select_oracle import (S, brute_round, check_all, check_quantile, empty_outputs, np_mad, np_median, round_add, same_values,
                                 walk_select)
from tests.test_golden import CASES, golden_cbin
from tests.test_gpu_window_stats import _hbm_recording, _oracle_decode

pytestmark = pytest.mark.gpu

E_ARG = -1
ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = sorted(n for n, c in CASES.items() if golden_cbin(c) is not None)
METHODS = ('linear', 'lower', 'higher', 'nearest', 'midpoint')


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
    for window in (1, 7, chunk_len, 3001, n + 5, None):
        for channels in (slice(None), slice(1, None, 3), shuffled):
            cols = _cols(channels, nc)
            if not cols:
                continue
            check_all(r, dec, 0, n, window, channels, cols, methods=METHODS if window == 7 else ('linear',))
    check_all(r, dec, -n // 2, -1, 1000, [nc - 1], [nc - 1])
    r.close()


def test_extremes(tmp_cfg):
    """A constant column (every wave of a workgroup on one counter), two values, the type's limits, a ramp, across window and chunk
    boundaries that fall inside a tile of the kernel, with the first and the last rank among the quantiles."""
    rows = 3 * 4096 + 1234
    rs = np.random.RandomState(1)
    x = np.zeros((rows, 6), np.int16)
    x[:, 0] = -1234
    x[:, 1] = np.where(rs.rand(rows) < 0.5, -7, 300)
    x[:, 2] = np.where(np.arange(rows) % 3 == 0, -32768, 32767)
    x[:, 3] = -32768
    x[:, 4] = 32767
    x[:, 5] = np.arange(rows) % 1000 - 500
    r = _file(tmp_cfg, x, rate=5000., chunk_duration=1.0)          # chunks of 5000 rows: boundaries inside tiles of 4096
    for window in (None, 4096, 4097, 5000, 5001, 999):
        check_all(r, x, 0, rows, window, slice(None), list(range(6)), q=(0.0, 0.5, 1.0), methods=('linear', 'nearest'))
    check_all(r, x, 4095, 2 * 4096 + 2, 4096, [0, 5], [0, 5], q=(0.0, 1.0))
    r.close()
    for dtype in ('uint8', 'int8', 'uint16', 'int32', 'uint32', 'int64', 'uint64'):
        info = np.iinfo(dtype)
        y = np.empty((2500, 3), dtype)
        y[:, 0] = info.min
        y[:, 1] = info.max
        y[:, 2] = np.where(rs.rand(2500) < 0.5, info.min, info.max)
        y[::7, 0] = info.max
        r = _file(tmp_cfg, y, chunk_duration=1.0)
        for window in (None, 1001):
            check_all(r, y, 0, 2500, window, slice(None), [0, 1, 2], q=(0.0, 0.5, 1.0))
        r.close()


def test_every_int16_value_once(tmp_cfg):
    v = np.arange(-32768, 32768, dtype=np.int64)
    x = np.stack([np.random.RandomState(2).permutation(v), v[::-1], v], axis=1).astype(np.int16)
    r = _file(tmp_cfg, x, rate=10000., chunk_duration=1.0)
    q = [0, 1 / 65535, 0.25, 0.5, 1 - 1 / 65535, 1]
    got = r.quantile(q)
    check_quantile(got, x, 0, 65536, None, q, 'linear')
    for k in (0, 1, 12345, 32767, 32768, 65534, 65535):            # rank k is the value k - 32768, in every column
        g = r.quantile(k / 65535, method='nearest')
        assert g.index[0] in (k, k - 1) and (g.quantile == k - 32768).all(), k
    assert (r.median() == -0.5).all() and (r.mad().mad == 16384).all()
    r.close()


@pytest.mark.parametrize('dtype', ['int16', 'float32'])
def test_column_counts(tmp_cfg, dtype):
    nc, rows = 385, 9001
    rs = np.random.RandomState(5)
    x = (rs.randn(rows, nc) * 3000).clip(-32768, 32767)
    x = x.astype(np.int16) if dtype == 'int16' else (x + 1000).astype(np.float32)
    r = _file(tmp_cfg, x, rate=3000., chunk_duration=1.0, do_time_diff=dtype == 'int16')
    dec = r[:]
    full = r.median()
    assert same_values(full, np_median(dec, 0, rows, None))
    for k in (1, 63, 64, 65, 385):
        cols = sorted(rs.choice(nc - 1, k - 1, replace=False).tolist()) + [nc - 1]
        rs.shuffle(cols)
        if k > 2:
            cols[1] = cols[0]                                      # a repeat
        check_all(r, dec, 0, rows, 4000, cols, cols, q=(0.0, 0.3, 1.0))
        assert same_values(r.median(channels=cols), np.ascontiguousarray(full[:, cols])), k
    r.close()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_special_floats(tmp_cfg, dtype):
    rs = np.random.RandomState(6)
    x = (rs.randn(9000, 7) * 10).astype(dtype)
    x[1000, 1] = np.nan
    x[1001, 1] = -np.nan
    x[3000, 2] = np.inf
    x[4500, 3] = -np.inf
    x[5000, 4], x[5001, 4] = np.inf, -np.inf
    x[:, 5] = 0
    x[::2, 5] = -0.0
    x[4500, 5] = 1.0
    x[:, 6] = np.where(rs.rand(9000) < 0.5, -0.0, 0.0)
    x[7, 6], x[8, 6] = np.finfo(dtype).tiny / 4, -np.finfo(dtype).max     # a subnormal and the largest negative number
    r = _file(tmp_cfg, x, do_time_diff=False)
    dec = r[:]
    assert np.array_equal(dec, x, equal_nan=True)
    cols = list(range(7))
    for window in (None, 2000, 1):
        check_all(r, dec, 0, 9000, window, slice(None), cols, methods=('linear', 'midpoint') if window else METHODS)
    q = [0, 0.5, 0.9999, 1]
    cen = rs.randn(5, 7) * 5
    cen[2, 0], cen[3, 2], cen[1, 3] = np.nan, np.inf, -np.inf        # NaN keys from the center; inf - inf
    for absolute in (False, True):
        got = r.quantile(q, window=2000, center=cen, absolute=absolute)
        check_quantile(got, dec, 0, 9000, 2000, q, 'linear', mode=2 if absolute else 1, center=cen)
    got = r.mad(window=2000, center=np.zeros(7))
    assert same_values(got.mad, np_mad(dec, 0, 9000, 2000, center=np.zeros(7)))
    lone = r.quantile(1.0, channels=1)                              # the window holds NaN: the result is NaN, upper is the NaN itself
    assert np.isnan(lone.quantile).all() and np.isnan(lone.upper).all() and lone.quantile.shape == (1,)
    assert np.isfinite(r.quantile(0.5, channels=1).lower).all() and np.isnan(r.median(channels=1)).all()
    r.close()


def test_integer_keys_with_center(tmp_cfg):
    rs = np.random.RandomState(9)
    for dtype in ('int16', 'uint8', 'int64'):
        info = np.iinfo(dtype)
        x = rs.randint(max(info.min, -(1 << 62)), min(info.max, 1 << 62), size=(6001, 5), dtype=np.int64).astype(dtype)
        r = _file(tmp_cfg, x, chunk_duration=1.0)
        cen = rs.randn(3, 5) * 40
        q = [0, 0.37, 1]
        for absolute in (False, True):
            got = r.quantile(q, window=2500, center=cen, absolute=absolute, method='higher')
            check_quantile(got, x, 0, 6001, 2500, q, 'higher', mode=2 if absolute else 1, center=cen)
        r.close()


def _dev_round(cbuf, slots, sizes, bounds, nc, flags, rb, re, window, cols, mode=0, center=None, chunks=slice(None)):
    rows = np.diff(bounds)
    k = chunks

    def fn(pref, shift):
        st, res, fn.out = hip.dev_rank_hist(cbuf, slots[k], sizes[k], bounds[:-1][k], rows[k], nc, np.int16, flags, rb, re, window, cols, mode,
                                            center, pref, shift, out=fn.out)
        assert st == [0] * len(rows[k])
        return res
    fn.out = None
    return fn


def test_config1_in_hbm_against_partition():
    """configs[1] (60 s x 385 int16) in HBM through mts_dev_rank_hist: a plain two-round walk for the median's ranks with windows of
    30000 rows and one window, against np.partition on the host; then a range inside chunks, shuffled columns, every other chunk."""
    nc = 385
    raw, cbuf, slots, sizes, bounds = _hbm_recording(nc=nc)
    x = raw.download(dtype=np.int16).reshape(-1, nc)
    n = x.shape[0]
    flags = hip.make_flags(True, False, 'F')
    for window in (30000, n):
        nw = n // window
        ranks = np.repeat(np.array([[(window - 1) // 2, window // 2]]), nw, axis=0)
        keys = walk_select(_dev_round(cbuf, slots, sizes, bounds, nc, flags, 0, n, window, np.arange(nc)), nw, nc, ranks, 16)
        got = hip.rank_values(keys, np.int16)
        for w in range(nw):
            part = np.partition(x[w * window:(w + 1) * window], [ranks[0, 0], ranks[0, 1]], axis=0)
            assert np.array_equal(got[w, 0], part[ranks[0, 0]]) and np.array_equal(got[w, 1], part[ranks[0, 1]]), (window, w)
    # one round on a lane's share of the chunks, a range that starts and ends inside chunks, shuffled columns: the partial histograms
    cols = np.random.RandomState(3).permutation(nc)[:70]
    rb, re, window = 12345, n - 777, 45678
    nw = -(-(re - rb) // window)
    pref = np.zeros((nw, S, 70), np.uint64)
    shift = np.full((nw, S, 70), 8, np.int32)
    shift[:, 1] = 0
    pref[:, 1] = 0x80                                             # selector 1: the items 0 .. 255
    res = _dev_round(cbuf, slots, sizes, bounds, nc, flags, rb, re, window, cols, chunks=slice(1, None, 2))(pref, shift)
    want = empty_outputs(nw, 70)
    count = np.zeros(nw, np.int64)
    for c in range(1, 60, 2):
        count += round_add(want, x[bounds[c]:bounds[c + 1], cols], int(bounds[c]), rb, re, window, 0, None, pref, shift.astype(np.int64))
    assert np.array_equal(res['count'], count)
    for key, w in zip(('hist', 'kmin', 'kmax'), want):
        assert res[key].tobytes() == w.tobytes(), key


def test_residency_bit_identity_cache_untouched_and_e_miss(tmp_cfg):
    nc, seconds, rate = 64, 6, 10000
    x = (np.random.RandomState(7).randn(seconds * rate, nc) * 1000).astype(np.int16)
    r = _file(tmp_cfg, x, rate=float(rate), codec=api.HipCodec(devices=[0]))
    keys = list(range(seconds))
    cache = r._cache_for(0)
    assert not any(hip.cache_query(cache, keys).tolist())
    q = [0.1, 0.5, 0.9]
    cold = r.quantile(q, window=7000)
    cold_mad = r.mad(window=7000)
    assert not any(hip.cache_query(cache, keys).tolist())         # a scan inserts nothing
    check_quantile(cold, x, 0, x.shape[0], 7000, q, 'linear')
    r[rate + 5:rate + 10]                                          # chunk 1 (and what is read ahead) resident
    before = hip.cache_query(cache, keys).tolist()
    assert before[1] == nc and not all(before)
    part = r.quantile(q, window=7000)
    part_mad = r.mad(window=7000)
    assert hip.cache_query(cache, keys).tolist() == before
    for k in keys:
        r[k * rate + 1:k * rate + 3]
    assert sum(map(bool, hip.cache_query(cache, keys).tolist())) > sum(map(bool, before))
    warm = r.quantile(q, window=7000)
    warm_mad = r.mad(window=7000)
    for a in (part, warm):
        for key in ('quantile', 'lower', 'upper', 'count'):
            assert a[key].tobytes() == cold[key].tobytes(), key
    assert part_mad.mad.tobytes() == warm_mad.mad.tobytes() == cold_mad.mad.tobytes()
    two = _open(tmp_cfg, api.HipCodec(devices=[0, 0]))            # two lanes on one device
    assert two.quantile(q, window=7000).quantile.tobytes() == cold.quantile.tobytes()
    two.close()
    # the C ABI: resident chunks without bytes equal the cold call; a chunk without bytes that is not resident is a miss
    r.close()
    r = _open(tmp_cfg, api.HipCodec(devices=[0]))
    r[rate + 5:rate + 10]
    cache = r._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    data = (tmp_cfg / 'd.cbin').read_bytes()
    offs, lens, bounds = np.array(r.chunk_offsets[:-1]), np.diff(r.chunk_offsets), np.array(r.chunk_bounds)
    lens_w = np.where(np.array(before) > 0, 0, lens)
    n = x.shape[0]
    nw = -(-n // 3001)
    pref = np.zeros((nw, S, nc), np.uint64)
    shift = np.full((nw, S, nc), 8, np.int32)
    shift[:, 1] = -1
    args = (bounds[:-1], data, offs)
    tail = (np.diff(bounds), nc, np.int16, r._flags(), 0, n, 3001, range(nc), 0, None, pref, shift)
    st_w, a = hip.rank_hist(cache, keys, *args, lens_w, *tail)
    st_c, b = hip.rank_hist(0, keys, *args, lens, *tail)
    assert st_w == st_c == [0] * seconds
    for key in ('hist', 'kmin', 'kmax', 'count'):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert (a['kmin'][:, 1] == hip.RANK_KEY_NONE).all() and not a['kmax'][:, 1].any() and not a['hist'][:, 1].any()
    assert hip.cache_query(cache, keys).tolist() == before
    miss = [k for k in keys if not before[k]][0]
    lens_bad = lens_w.copy()
    lens_bad[miss] = 0
    with pytest.raises(hip.HipError) as e:
        hip.rank_hist(cache, keys, *args, lens_bad, *tail)
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
        s = r.quantile([0, 0.37, 1], lo, hi, window=w)
        for k in ('count', 'quantile', 'lower', 'upper', 'index', 'frac'):
            out['%s_%s_%d' % (tag, k, i)] = s[k]
        m = r.mad(lo, hi, window=w)
        out['%s_center_%d' % (tag, i)], out['%s_mad_%d' % (tag, i)] = m.center, m.mad
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
def test_quantile_pieces_and_residency_do_not_change_the_result(tmp_cfg, dtype):
    """MTS_PIPE_BYTES unset (one piece) and two chunks a piece (>= 5 pieces), each cold and with chunks 3, 4 and 9 of 12 resident:
    every output of Reader.quantile and Reader.mad (mode != 0, a center uploaded) is the same bytes, and right by the oracle."""
    rows, nc = 12 * 3000, 40
    x = (np.random.RandomState(8).randn(rows, nc) * 300).astype(dtype)
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
    assert sorted(outs[0]) == sorted(outs[1]) and len(outs[0]) == 32
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
        if k.startswith('part_'):
            assert outs[1][k].tobytes() == outs[1]['cold_' + k[5:]].tobytes(), k
    for i, (w, lo, hi) in enumerate(((None, 0, rows), (4321, 1234, rows - 77))):
        got = type('B', (), {k: outs[1]['part_%s_%d' % (k, i)] for k in ('count', 'quantile', 'lower', 'upper', 'index', 'frac')})
        check_quantile(got, x, lo, hi, w, [0, 0.37, 1], 'linear')
        assert same_values(outs[1]['part_center_%d' % i], np_median(x, lo, hi, w))
        assert same_values(outs[1]['part_mad_%d' % i], np_mad(x, lo, hi, w))


def test_one_round_against_brute_force(tmp_cfg):
    """One call of the C ABI with two active selectors per cell, float keys in the three modes, against counting in Python."""
    rs = np.random.RandomState(11)
    x = (rs.randn(700, 3) * 4).astype(np.float32)
    x[5, 0], x[6, 0], x[7, 1], x[8, 1] = np.nan, -0.0, np.inf, 0.0
    r = _file(tmp_cfg, x, do_time_diff=False)
    data = (tmp_cfg / 'd.cbin').read_bytes()
    offs, lens, bounds = np.array(r.chunk_offsets[:-1]), np.diff(r.chunk_offsets), np.array(r.chunk_bounds)
    for mode, kb in ((0, 32), (1, 64), (2, 64)):
        cen = rs.randn(1, 3) if mode else None
        pref = np.zeros((1, S, 3), np.uint64)
        shift = np.zeros((1, S, 3), np.int32)
        shift[0, 0] = kb - 8
        shift[0, 1] = kb - 16
        pref[0, 1] = 0xC0 if mode == 0 else 0xBF                  # positive numbers of a common exponent range
        st, got = hip.rank_hist(0, [0], bounds[:-1], data, offs, lens, np.diff(bounds), 3, np.float32, r._flags(), 0, 700, 700, range(3), mode,
                                cen, pref, shift)
        assert st == [0]
        for j in range(3):
            h, kmin, kmax = brute_round(x[:, j], mode, None if cen is None else cen[0, j], [int(p) for p in pref[0, :, j]],
                                        [int(s) for s in shift[0, :, j]])
            assert got['hist'][0, :, :, j].tolist() == h and got['kmin'][0, :, j].tolist() == kmin and got['kmax'][0, :, j].tolist() == kmax
    r.close()


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
    for call in (lambda: r.median(window=1000), lambda: r.quantile(0.3), lambda: r.mad()):
        with pytest.raises(IOError, match='#2'):
            call()
    assert same_values(r.median(0, 6000), np_median(x, 0, 6000, None))    # chunks 0 and 1 only
    b = np.array(hdr['chunk_bounds'])
    pref = np.zeros((15, S, nc), np.uint64)
    shift = np.full((15, S, nc), 8, np.int32)
    st, got = hip.rank_hist(0, range(5), b[:-1], bytes(data), o[:-1], np.diff(o), np.diff(b), nc, np.int16, r._flags(), 0, rows, 1000, range(nc),
                            0, None, pref, shift)
    assert st == [0, 0, hip.CHUNK_CORRUPT, 0, 0]                 # only that chunk: its windows count nothing
    assert got['count'].tolist() == [1000] * 6 + [0] * 3 + [1000] * 6
    assert not got['hist'][6:9].any() and (got['hist'][:6].sum(axis=2) == 1000).all()
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
    outd = hip.DevBuffer(1 << 22)

    def call(dev, row0=(0, 100), rows=(100, 100), rb=0, re=200, window=10, cols=(0, 1), itemsize=2, flags=hip.make_flags(), mode=0, center=True,
             shift=8, prefix=0):
        a = [np.array(v, dtype=np.int64) for v in ([0, 1], list(row0), [0, len(zs[0])], [len(zs[0]), len(zs[1])], list(rows))]
        c = np.array(cols, dtype=np.int32)
        nw = max(-(-(re - rb) // window), 1) if window >= 1 else 1
        pre = np.full((nw, S, max(len(c), 1)), prefix, np.uint64)
        shf = np.full((nw, S, max(len(c), 1)), shift, np.int32)
        cen = np.zeros((nw, max(len(c), 1)))
        oh, ok_, ox = np.zeros(pre.size * 256, np.uint32), np.zeros(pre.size, np.uint64), np.zeros(pre.size, np.uint64)
        cnt = np.zeros(nw, np.int64)
        st = np.full(2, 99, np.int32)
        keep.append((a, c, pre, shf, cen, oh, ok_, ox, cnt, st))
        P = lambda v: v.ctypes.data_as(C.POINTER(C.c_long))  # noqa: E731
        U = lambda v: v.ctypes.data_as(C.POINTER(C.c_ulonglong))  # noqa: E731
        I = lambda v: v.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731,E741
        cp = cen.ctypes.data_as(C.POINTER(C.c_double)) if center else None
        if dev:
            rc = L.mts_dev_rank_hist(0, None, dbuf.at(), P(a[2]), P(a[3]), P(a[1]), P(a[4]), 2, nc, itemsize, flags, rb, re, window, len(c), I(c),
                                     mode, cp, U(pre), I(shf), outd.at(), outd.at(1 << 21), outd.at(3 << 20), P(cnt), I(st))
        else:
            rc = L.mts_rank_hist(0, 0, 2, P(a[0]), P(a[1]), data.ctypes.data_as(C.c_void_p), P(a[2]), P(a[3]), P(a[4]), nc, itemsize, flags, rb,
                                 re, window, len(c), I(c), mode, cp, U(pre), I(shf), oh.ctypes.data_as(C.POINTER(C.c_uint)), U(ok_), U(ox),
                                 P(cnt), I(st))
        return rc, int(st[0])
    for dev in (False, True):
        assert call(dev) == (0, 0)
        assert call(dev, rb=30, re=170, mode=2, shift=56) == (0, 0)
        assert call(dev, shift=-1) == (0, 0)
        for bad in (dict(cols=()), dict(cols=(0, 4)), dict(cols=(-1,)), dict(window=0), dict(window=-3), dict(rb=50, re=20), dict(rb=-5),
                    dict(row0=(0, 99)), dict(row0=(50, 150), re=120), dict(rows=(0, 100)), dict(itemsize=3),
                    dict(flags=hip.FLAG_FLOAT, itemsize=2), dict(mode=3), dict(mode=-1), dict(mode=1, center=False), dict(shift=9),
                    dict(shift=57, mode=1), dict(shift=0, prefix=256), dict(shift=8, prefix=1)):
            rc, st = call(dev, **bad)
            assert rc == E_ARG, (dev, bad)                         # MTS_E_ARG ...
            assert st == 99, (dev, bad)                            # ... before anything ran
