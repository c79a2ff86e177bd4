"""Reader.welch and mts_welch / mts_dev_welch on the MI355X: the FFT kernel against a float64 reference (welch_f64) within the
derived per-bin bound (welch_bound_bins) over the oracle's decode of every golden file and all ten item types at every nperseg, exact cases,
bit-identity across lanes, pieces, cache residency, repeats and columns, the two entry points, argument errors, a damaged chunk,
special float values and the configs[1] recording in HBM."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.codec_oracle import OracleCodec
from tests.test_gpu_window_stats import GOLDEN, CASES, _golden_reader, _hbm_recording, _oracle_decode
from tests.welch_oracle import assert_welch_close, psd_scale, welch_bound_bins, welch_f64

pytestmark = pytest.mark.gpu

RATE = 30000
E_ARG = -1                                                               # MTS_E_ARG
DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _check(r, dec, nperseg, start=0, stop=None, channels=slice(None), noverlap=None, window='hann', detrend='constant',
           scaling='density', dtype=np.float32):
    """Reader.welch against welch_f64 over `dec` (the oracle's decode) within welch_bound_bins; returns the largest error / bound."""
    f, got = r.welch(nperseg, start, stop, channels=channels, noverlap=noverlap, window=window, detrend=detrend, scaling=scaling, dtype=dtype)
    n, nc = dec.shape
    i0 = r._validate_index(start, 0)
    i1 = max(i0, r._validate_index(stop, n))
    cols = [channels % nc] if isinstance(channels, int) else list(range(*channels.indices(nc))) if isinstance(channels, slice) else \
        [int(c) % nc for c in channels]
    step = nperseg - (nperseg // 2 if noverlap is None else noverlap)
    taper = api.welch_window(window, nperseg)
    tot, _, n_seg, first = welch_f64(dec[:, cols], i0, i1, nperseg, step, taper, detrend == 'constant', dtype)
    k = psd_scale(nperseg, taper, scaling, r.sample_rate, n_seg)[:, None]
    assert got.dtype == np.float64 and f.shape == (nperseg // 2 + 1,)
    return assert_welch_close(got.reshape(tot.shape), tot * k, welch_bound_bins(tot, first, n_seg) * k)


def _file(tmp, x, rate=RATE, chunk_duration=1., **kw):
    raw = tmp / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'd.cbin', tmp / 'd.ch', sample_rate=rate, n_channels=x.shape[1], dtype=x.dtype,
                         chunk_duration=chunk_duration, check_after_compress=False, **kw)
    r = mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', check_after_decompress=False)
    ro = mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', codec=OracleCodec(), check_after_decompress=False)
    dec = ro[:]
    ro.close()
    return r, dec


@pytest.mark.parametrize('name', GOLDEN)
def test_golden_files(name, tmp_cfg):
    case = CASES[name]
    r, hdr = _golden_reader(tmp_cfg, case)
    dec = _oracle_decode(case)
    nc, n = hdr['n_channels'], hdr['shape'][0]
    shuffled = [int(c) for c in np.random.RandomState(len(name)).permutation(nc)] + [0, nc - 1, 0]
    worst = 0.0
    for nperseg in (16, 64, 256, 1024, 4096):
        if nperseg > n:
            continue
        for dtype in (np.float32, np.float64):
            worst = max(worst, _check(r, dec, nperseg, dtype=dtype))
            if n - n // 5 >= nperseg:
                worst = max(worst, _check(r, dec, nperseg, n // 5, None, shuffled, nperseg // 4, 'hamming', False, 'spectrum', dtype))
    print('%s: largest error / bound %.3g' % (name, worst))
    r.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_item_type_and_nperseg(tmp_cfg, dtype):
    rows, nc = 3 * 16384 + 1000, 19
    rs = np.random.RandomState(3)
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        x = (rs.randn(rows, nc) * 100 + 50).astype(dt)
    else:
        info = np.iinfo(dt)
        x = rs.randint(max(info.min, -2 ** 62), min(info.max, 2 ** 62), size=(rows, nc), dtype=np.int64).astype(dt)
    r, dec = _file(tmp_cfg, x, rate=700., chunk_duration=7000 / 700.)
    worst = {}
    for lg in range(4, 15):
        nperseg = 1 << lg
        for cdt in (np.float32, np.float64):
            worst[(nperseg, np.dtype(cdt).name)] = _check(r, dec, nperseg, 0, None if nperseg >= 1024 else 20000, dtype=cdt)
    print(dtype, 'largest error / bound:', max(worst.values()), max(worst, key=worst.get))
    r.close()


def test_exact_cases(tmp_cfg):
    """boxcar, no detrend, noverlap 0: an impulse a at each segment's first row gives a^2 in every bin; piecewise-constant segments
    give (nperseg v)^2 at bin 0 and 0 elsewhere (a segment misplaced by one row fails); constant segments detrended give 0."""
    nc = 4
    for nperseg in (16, 256, 1024, 16384):
        n_seg = 5
        rows = nperseg * n_seg + 3
        x = np.zeros((rows, nc), np.int16)
        a = np.arange(1, n_seg + 1) * 3 + 2                              # impulses
        x[np.arange(n_seg) * nperseg, 0] = a
        v = np.arange(n_seg) * 7 - 11                                    # piecewise constant
        x[:nperseg * n_seg, 1] = np.repeat(v, nperseg)
        x[nperseg * n_seg:, 1] = 1000
        x[:, 2] = -123
        x[:, 3] = np.repeat(v * 3, nperseg).tolist() + [5, 5, 5]
        r, _ = _file(tmp_cfg, x, rate=1000., chunk_duration=max(nperseg, 700) * 0.37 / 1000.)
        for cdt in (np.float32, np.float64):
            # spectrum scaling with a boxcar: sum / nperseg^2, interior bins doubled, / n_seg -- undone exactly below (powers of two
            # and n_seg = 5: the reference is formed with the same operations)
            _, p = r.welch(nperseg, 0, nperseg * n_seg, noverlap=0, window='boxcar', detrend=False, scaling='spectrum', dtype=cdt)
            k = np.full(nperseg // 2 + 1, 2.0 / float(nperseg) ** 2)
            k[0] = k[-1] = 1.0 / float(nperseg) ** 2
            s_imp = float(sum(int(q) ** 2 for q in a))
            want0 = np.zeros(nperseg // 2 + 1) + s_imp
            assert np.array_equal(p[:, 0], want0 * k / n_seg), cdt
            s_pc = float(sum((nperseg * int(q)) ** 2 for q in v))
            want1 = np.zeros(nperseg // 2 + 1)
            want1[0] = s_pc
            assert np.array_equal(p[:, 1], want1 * k / n_seg), cdt
            _, p = r.welch(nperseg, 0, nperseg * n_seg, noverlap=0, window='hann', detrend='constant', dtype=cdt)
            assert not p[:, [1, 2, 3]].any(), cdt
            _, p = r.welch(nperseg, 3, None, noverlap=nperseg // 2, window='hann', detrend='constant', dtype=cdt, channels=2)
            assert not p.any(), cdt
        r.close()


def test_chunk_edges_tiny_chunks_and_many_columns(tmp_cfg):
    rs = np.random.RandomState(5)
    nc = 150
    x = (rs.randn(9000, nc) * 300).astype(np.int16)
    r, dec = _file(tmp_cfg, x, rate=1000., chunk_duration=0.999)
    b = r.chunk_bounds
    cols = list(rs.randint(0, nc, size=97)) + [0, 0, nc - 1]               # > 64 columns, repeats, not a multiple of a tile
    for nperseg in (16, 256, 1024):
        for start in (b[2] - nperseg, b[2] - nperseg + 1, b[2] - nperseg - 1, b[1], b[1] + 1, b[1] - 1):
            for dtype in (np.float32, np.float64):
                _check(r, dec, nperseg, start, start + nperseg * 3 + 5, cols, 0, dtype=dtype)
                _check(r, dec, nperseg, start, None, slice(3, None, 7), nperseg - 1 if nperseg <= 256 else None, dtype=dtype)
    r.close()
    x = (rs.randn(3000, 5) * 30).astype(np.float32)
    r, dec = _file(tmp_cfg, x, rate=1000., chunk_duration=0.001 * 37)    # 37-row chunks: one segment spans many chunks
    for nperseg in (64, 1024, 2048):
        _check(r, dec, nperseg, 1, None, [4, 0, 4], nperseg // 8)
    r.close()
    for name in GOLDEN:
        if 'tiny' in name:
            r, hdr = _golden_reader(tmp_cfg, CASES[name])
            dec = _oracle_decode(CASES[name])
            _check(r, dec, 16, 0, None)
            _check(r, dec, min(256, 1 << int(np.log2(hdr['shape'][0]))), 1, None, dtype=np.float64)
            r.close()


def _tiny(tmp, nc=23, rows=8 * RATE // 3, seed=11):
    x = (np.random.RandomState(seed).randn(rows, nc) * 500).astype(np.int16)
    raw = tmp / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'd.cbin', tmp / 'd.ch', sample_rate=RATE, n_channels=nc, dtype=np.int16, chunk_duration=0.25,
                         check_after_compress=False)
    return x


def _open(tmp, codec=None):
    return mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', codec=codec, check_after_decompress=False)


def test_bit_identity_lanes_cache_repeats_columns(tmp_cfg):
    x = _tiny(tmp_cfg)
    one = _open(tmp_cfg, api.HipCodec(devices=[0]))
    two = _open(tmp_cfg, api.HipCodec(devices=[0, 0]))
    for nperseg, noverlap, dtype in [(16, 8, np.float32), (256, None, np.float32), (1024, 1023, np.float64), (4096, 0, np.float32),
                                     (64, 1, np.float64)]:
        _, a = one.welch(nperseg, 7, None, noverlap=noverlap, dtype=dtype)
        _, b = two.welch(nperseg, 7, None, noverlap=noverlap, dtype=dtype)
        assert a.tobytes() == b.tobytes()
        _, a2 = one.welch(nperseg, 7, None, noverlap=noverlap, dtype=dtype)
        assert a2.tobytes() == a.tobytes()
        for c in (0, 5, 22):
            _, s = one.welch(nperseg, 7, None, channels=[c], noverlap=noverlap, dtype=dtype)
            assert s.tobytes() == np.ascontiguousarray(a[:, [c]]).tobytes()
        one[one.chunk_bounds[1]:one.chunk_bounds[one.n_chunks // 2 + 1] + 10]  # half the chunks resident now
        resident = sum(int(q) >= one.n_channels for q in hip.cache_query(one._cache_for(0), list(range(one.n_chunks))))
        assert resident >= one.n_chunks // 2
        _, w = one.welch(nperseg, 7, None, noverlap=noverlap, dtype=dtype)
        assert w.tobytes() == a.tobytes()
    keys = list(range(one.n_chunks))
    cache = one._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(int(q) >= one.n_channels for q in before) >= one.n_chunks // 2
    one.welch(256)
    assert hip.cache_query(cache, keys).tolist() == before              # a scan leaves the cache as it was
    one.close()
    two.close()


def test_groups_split_over_lanes_and_calls(tmp_cfg, monkeypatch):
    """A recording of several groups (G * step >= 2^20 rows each): calls and lanes that start after the first group (seg_begin > 0)
    give the bits of one lane and one call, and the float64 reference within the bound."""
    rows, nc = 2_200_000, 3
    x = (np.random.RandomState(12).randn(rows, nc) * 400).astype(np.int16)
    raw = tmp_cfg / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', sample_rate=RATE, n_channels=nc, dtype=np.int16, chunk_duration=3.1,
                         check_after_compress=False)
    one = _open(tmp_cfg, api.HipCodec(devices=[0]))
    codec = api.HipCodec(devices=[0, 0])
    calls = []
    welch = codec.welch

    def recorded(*a, **kw):
        calls.append((kw.get('lane'), int(a[11]), int(a[12])))            # (lane, seg_begin, seg_end)
        return welch(*a, **kw)
    codec.welch = recorded
    two = _open(tmp_cfg, codec)
    for nperseg, noverlap, dtype in [(1024, None, np.float32), (16384, 0, np.float64), (256, 7, np.float32)]:
        step = nperseg - (nperseg // 2 if noverlap is None else noverlap)
        n_seg = (rows - 5 - nperseg) // step + 1
        G = hip.welch_group_segments(step)
        assert -(-n_seg // G) >= 2
        _, a = one.welch(nperseg, 5, None, noverlap=noverlap, dtype=dtype)
        calls.clear()
        _, b = two.welch(nperseg, 5, None, noverlap=noverlap, dtype=dtype)
        assert a.tobytes() == b.tobytes()
        assert {lane for lane, _, _ in calls} == {0, 1} and any(s0 > 0 for _, s0, _ in calls)
        assert all(s0 % G == 0 for _, s0, _ in calls)
        monkeypatch.setattr(api, 'WELCH_CALL_BYTES', 1)                     # one call per group
        calls.clear()
        _, c = two.welch(nperseg, 5, None, noverlap=noverlap, dtype=dtype)
        monkeypatch.setattr(api, 'WELCH_CALL_BYTES', 1 << 30)
        assert c.tobytes() == a.tobytes()
        assert len(calls) == -(-n_seg // G) and sorted(s0 for _, s0, _ in calls) == list(range(0, n_seg, G))
        if nperseg >= 1024:
            taper = api.welch_window('hann', nperseg)
            tot, _, _, first = welch_f64(x[:, [1]], 5, rows, nperseg, step, taper, True, dtype)
            k = psd_scale(nperseg, taper, 'density', RATE, n_seg)[:, None]
            print('%d %s: largest error / bound %.3g' % (nperseg, np.dtype(dtype).name,
                                                         assert_welch_close(a[:, [1]], tot * k, welch_bound_bins(tot, first, n_seg) * k)))
    one.close()
    two.close()


def test_pipe_bytes_do_not_change_the_result(tmp_cfg):
    _tiny(tmp_cfg)
    script = ("import sys, numpy as np, mtscomp_amd; sys.path.insert(0, %r); "
              "r = mtscomp_amd.decompress(%r, %r, check_after_decompress=False); "
              "np.save(sys.argv[1], np.stack([r.welch(256, 33)[1], r.welch(1024, 5, noverlap=1000, dtype=np.float64)[1][:129]]))") % (
        os.getcwd(), str(tmp_cfg / 'd.cbin'), str(tmp_cfg / 'd.ch'))
    outs = []
    for pipe in (None, str(200 * 1024), str(1500 * 1024)):
        env = dict(os.environ)
        env.pop('MTS_PIPE_BYTES', None)
        if pipe:
            env['MTS_PIPE_BYTES'] = pipe
        p = tmp_cfg / ('o%d.npy' % len(outs))
        subprocess.run([sys.executable, '-c', script, str(p)], env=env, check=True, timeout=300)
        outs.append(np.load(p))
    assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


def test_special_floats(tmp_cfg):
    rs = np.random.RandomState(6)
    x = rs.randn(6000, 6) * 10
    x[1000, 1] = np.nan
    x[3000, 2] = np.inf
    x[4500, 3] = -np.inf
    x[:, 4] = 1e-310                                                     # subnormals
    r, dec = _file(tmp_cfg, x.astype(np.float64), rate=1000., do_time_diff=False)
    for cdt in (np.float32, np.float64):
        for detrend in ('constant', False):
            _check(r, dec, 256, 0, None, noverlap=64, detrend=detrend, dtype=cdt)
    _, p = r.welch(256, noverlap=0, dtype=np.float64)
    assert not np.isfinite(p[:, 1]).all() and np.isfinite(p[:, [0, 5]]).all()
    r.close()


def test_dev_entry_equals_host_entry_and_errors(tmp_cfg):
    nc = 385
    raw, cbuf, slots, sizes, bounds = _hbm_recording(seconds=4, nc=nc)
    x = raw.download(dtype=np.int16).reshape(-1, nc)
    flags = hip.make_flags(True, False, 'F')
    rows = np.diff(bounds)
    cols = np.arange(nc)
    n = x.shape[0]
    data = cbuf.download(dtype=np.uint8)
    taper = api.welch_window('hann', 1024)
    n_seg = (n - 1024) // 512 + 1
    st, dev, _ = hip.dev_welch(cbuf, slots, sizes, bounds[:-1], rows, nc, np.int16, flags, 0, 0, n_seg, 1024, 512, taper, True, np.float32, cols)
    assert st == [0] * len(rows)
    st2, host = hip.welch(0, list(range(len(rows))), bounds[:-1], data.tobytes(), slots, sizes, rows, nc, np.int16, flags, 0, 0, n_seg, 1024,
                          512, taper, True, np.float32, cols)
    assert st2 == [0] * len(rows)
    assert dev.tobytes() == host.tobytes()
    tot, _, _, first = welch_f64(x, 0, n, 1024, 512, taper, True, np.float32)
    print('largest error / bound %.3g' % assert_welch_close(dev.sum(axis=0), tot, welch_bound_bins(tot, first, n_seg)))
    # MTS_E_ARG before anything runs, both entries
    L = hip.lib()
    lp = [np.ascontiguousarray(a, dtype=np.int64) for a in (slots, sizes, bounds[:-1], rows)]
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_long))  # noqa: E731
    out = hip.DevBuffer(1 << 20)
    hout = np.zeros(1 << 17)
    status = np.zeros(len(rows), np.int32)
    good = dict(nperseg=1024, step=512, seg_begin=0, seg_end=n_seg, csize=4, taper=taper, cols=np.arange(8, dtype=np.int32))
    bad = [dict(nperseg=1000), dict(nperseg=8), dict(nperseg=32768), dict(step=0), dict(step=1025), dict(csize=2),
           dict(taper=np.r_[taper[:-1], np.nan]), dict(cols=np.array([0, nc], np.int32)), dict(cols=np.array([-1], np.int32)),
           dict(seg_begin=1), dict(seg_end=0), dict(seg_end=n_seg + 100)]
    keys = np.arange(len(rows), dtype=np.int64)
    for b in bad:
        a = dict(good, **b)
        t = np.ascontiguousarray(a['taper'] if a['taper'].size == a['nperseg'] or 'taper' in b else np.ones(max(a['nperseg'], 1)),
                                 dtype=np.float64)
        if t.size < max(a['nperseg'], 16):
            t = np.ones(max(a['nperseg'], 16))
        cc = np.ascontiguousarray(a['cols'])
        rc = L.mts_dev_welch(0, None, cbuf.at(), P(lp[0]), P(lp[1]), P(lp[2]), P(lp[3]), len(rows), nc, 2, flags, 0, a['seg_begin'],
                             a['seg_end'], a['nperseg'], a['step'], t.ctypes.data_as(C.POINTER(C.c_double)), 1, a['csize'], cc.size,
                             cc.ctypes.data_as(C.POINTER(C.c_int)), out.at(), status.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == E_ARG, b
        rc = L.mts_welch(0, 0, len(rows), P(keys), P(lp[2]), data.ctypes.data_as(C.c_void_p), P(lp[0]), P(lp[1]), P(lp[3]), nc, 2, flags, 0,
                         a['seg_begin'], a['seg_end'], a['nperseg'], a['step'], t.ctypes.data_as(C.POINTER(C.c_double)), 1, a['csize'],
                         cc.size, cc.ctypes.data_as(C.POINTER(C.c_int)), hout.ctypes.data_as(C.c_void_p),
                         status.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == E_ARG, b
    # chunks not adjacent
    r1 = lp[2].copy()
    r1[2] += 1
    rc = L.mts_dev_welch(0, None, cbuf.at(), P(lp[0]), P(lp[1]), P(r1), P(lp[3]), len(rows), nc, 2, flags, 0, 0, n_seg, 1024, 512,
                         taper.ctypes.data_as(C.POINTER(C.c_double)), 1, 4, 8, good['cols'].ctypes.data_as(C.POINTER(C.c_int)), out.at(),
                         status.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == E_ARG
    # a damaged chunk is reported in the status
    bad_data = data.copy()
    bad_data[slots[2] + 40:slots[2] + 80] = 0xff
    st3, _ = hip.welch(0, list(range(len(rows))), bounds[:-1], bad_data.tobytes(), slots, sizes, rows, nc, np.int16, flags, 0, 0, n_seg, 1024,
                       512, taper, True, np.float32, cols)
    assert st3[2] != 0 and st3[0] == 0


def test_config1_in_hbm():
    nc = 385
    raw, cbuf, slots, sizes, bounds = _hbm_recording(nc=nc)
    x = raw.download(dtype=np.int16).reshape(-1, nc)
    n = x.shape[0]
    flags = hip.make_flags(True, False, 'F')
    rows = np.diff(bounds)
    taper = api.welch_window('hann', 1024)
    n_seg = (n - 1024) // 512 + 1
    out = None
    res = []
    for cdt in (np.float32, np.float64):
        st, got, out = hip.dev_welch(cbuf, slots, sizes, bounds[:-1], rows, nc, np.int16, flags, 0, 0, n_seg, 1024, 512, taper, True, cdt,
                                     np.arange(nc), out=out)
        assert st == [0] * len(rows)
        assert got.shape == (2, 513, nc)
        res.append(got.sum(axis=0))
        # a call that starts at the second group (seg_begin = G > 0): group 1 of the whole call, bit for bit, from both entries
        G = hip.welch_group_segments(512)
        st, g1, _ = hip.dev_welch(cbuf, slots, sizes, bounds[:-1], rows, nc, np.int16, flags, 0, G, n_seg, 1024, 512, taper, True, cdt,
                                  np.arange(nc))
        assert st == [0] * len(rows) and g1.shape == (1, 513, nc)
        assert g1[0].tobytes() == got[1].tobytes()
        first = int(np.searchsorted(bounds, G * 512, side='right')) - 1            # the chunks group 1 reads
        keys = list(range(first, len(rows)))
        data = cbuf.download(dtype=np.uint8)
        st, h1 = hip.welch(0, keys, bounds[first:-1], data.tobytes(), slots[first:], sizes[first:], rows[first:], nc, np.int16, flags, 0, G,
                           n_seg, 1024, 512, taper, True, cdt, np.arange(nc))
        assert st == [0] * len(keys)
        assert h1[0].tobytes() == got[1].tobytes()
    cols = np.arange(0, nc, 16)
    for cdt, got in zip((np.float32, np.float64), res):
        tot, _, _, first = welch_f64(x[:, cols], 0, n, 1024, 512, taper, True, cdt)
        print('configs[1] %s: largest error / bound %.3g' % (np.dtype(cdt).name,
                                                              assert_welch_close(got[:, cols], tot, welch_bound_bins(tot, first, n_seg))))
