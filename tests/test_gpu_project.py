"""Reader.project and mts_project / mts_dev_project on the MI355X: k_project against the float32 definition (bit for bit the fmaf
chain of tests/project_oracle.py) and, for float64, the bound derived there, over the oracle's decode: every tile edge of the shapes,
every item type and value family, independence of an output from its neighbours and from the split into calls, invariance under
pieces, residency, lanes and the two entry points, argument errors, a damaged chunk, and whitening end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from tests.codec_oracle import OracleCodec
from tests.project_oracle import (assert_project_within, assert_same_bits, project_chain_f32, project_chain_f64, project_reference)

pytestmark = pytest.mark.gpu


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def _make(tmp, x, name='d', **kw):
    """x as a recording in chunks of 100 rows -> (Reader on the device, the oracle's decode of the file)."""
    raw = tmp / (name + '.bin')
    x.tofile(raw)
    if x.dtype.kind == 'f':
        kw.setdefault('do_time_diff', False)                        # (floats: the stored bits are the items)
    mtscomp_amd.compress(raw, tmp / (name + '.cbin'), tmp / (name + '.ch'), sample_rate=100., n_channels=x.shape[1], dtype=x.dtype,
                         check_after_compress=False, **kw)
    ro = mtscomp_amd.decompress(tmp / (name + '.cbin'), tmp / (name + '.ch'), codec=OracleCodec(), check_after_decompress=False)
    dec = ro[:]                                                     # the reference: the oracle's decode, not the device's
    ro.close()
    r = mtscomp_amd.decompress(tmp / (name + '.cbin'), tmp / (name + '.ch'), check_after_decompress=False)
    assert r.chunk_bounds[1] == 100
    return r, dec


def _check(r, dec, w, off, cols, start=0, stop=None):
    """float32 bit for bit the chain, float64 within the bound, on rows [start, stop) -> (y32, y64)."""
    x = dec[start:stop][:, cols]
    y32 = r.project(w, start, stop, channels=cols, offset=off, dtype=np.float32)
    assert_same_bits(y32, project_chain_f32(x, off, w))
    y64 = r.project(w, start, stop, channels=cols, offset=off, dtype=np.float64)
    assert_project_within(y64, x, off, w, np.float64)
    return y32, y64


N_OUTS = (1, 15, 16, 17, 63, 64, 65, 130)
RANGES = ((0, 1), (0, 63), (37, 37 + 64), (99, 301))


@pytest.mark.parametrize('n_cols', [1, 3, 4, 5, 63, 64, 65, 385])
def test_shapes(tmp_cfg, n_cols):
    rs = np.random.RandomState(n_cols)
    rows, nc = 437, n_cols + 3                                      # (64-row tiles straddle the 100-row chunks; the last tile is short)
    x = rs.randint(-3000, 3000, size=(rows, nc)).astype(np.int16)
    r, dec = _make(tmp_cfg, x)
    assert np.array_equal(dec, x)
    cols = rs.permutation(nc)[:n_cols]
    for n_out in N_OUTS:
        w, off = rs.randn(n_cols, n_out), rs.randn(n_cols) * 100
        y32, y64 = _check(r, dec, w, off, cols)
        for a, b in RANGES:
            assert_same_bits(r.project(w, a, b, channels=cols, offset=off), y32[a:b])
            assert_same_bits(r.project(w, a, b, channels=cols, offset=off, dtype=np.float64), y64[a:b])
    r.close()


def _dyadic(rs, n_cols, n_out):
    return rs.randint(-8, 9, size=(n_cols, n_out)).astype(np.float64) / 16


@pytest.mark.parametrize('dtype', ['int8', 'int16', 'int32', 'int64', 'uint8', 'uint16', 'uint32', 'uint64', 'float32', 'float64'])
def test_every_item_type(tmp_cfg, dtype):
    dt = np.dtype(dtype)
    rs = np.random.RandomState(dt.num)
    rows, nc, n_cols, n_out = 330, 70, 67, 18
    cols = rs.permutation(nc)[:n_cols]
    fam = {}
    if dt.kind == 'f':
        fam['small'] = rs.randint(-100, 100, size=(rows, nc)).astype(dt)
        fam['randn'] = (rs.randn(rows, nc) * 100).astype(dt)
        sp = (rs.randn(rows, nc) * 10).astype(dt)
        sp[5, cols[3]], sp[120, cols[0]], sp[121, cols[0]], sp[250, cols[66]] = np.nan, np.inf, -np.inf, np.inf
        sp[7] = -0.0
        sp[300, ::2] = -0.0
        fam['special'] = sp
        if dt == np.float32:
            fam['subnormal'] = (rs.randn(rows, nc) * 1e-20).astype(dt)
    else:
        info = np.iinfo(dt)
        fam['small'] = rs.randint(max(info.min, -100), min(info.max, 100) + 1, size=(rows, nc)).astype(dt)
        if dt == np.uint64:
            fam['full'] = rs.randint(0, 2 ** 63 - 1, size=(rows, nc), dtype=np.int64).astype(dt) * 2 + 1
        else:
            fam['full'] = rs.randint(info.min, info.max, size=(rows, nc), dtype=np.int64).astype(dt)
        if dt == np.uint16:
            fam['midscale'] = rs.randint(32768 - 40, 32768 + 40, size=(rows, nc)).astype(dt)
    for name, x in fam.items():
        r, dec = _make(tmp_cfg, x, name)
        assert dec.tobytes() == x.tobytes()
        xs = dec[:, cols]
        for off in (None, rs.randint(-50, 50, size=n_cols).astype(np.float64)):
            if name == 'small':                                      # dyadic weights: exact in both types, no rounding anywhere
                w = _dyadic(rs, n_cols, n_out)
                want = project_reference(xs, off, w)[0].astype(np.float64)
                for odt in (np.float32, np.float64):
                    got = r.project(w, channels=cols, offset=off, dtype=odt)
                    assert np.array_equal(got, want.astype(odt)), (name, odt)
                assert_same_bits(r.project(w, channels=cols, offset=off), project_chain_f32(xs, off, w))
                continue
            w = rs.randn(n_cols, n_out) * (1e-20 if name == 'subnormal' else 1.0)
            w[rs.randint(0, n_cols, 40), rs.randint(0, n_out, 40)] = 0.0        # zero weights are not skipped
            if name == 'midscale' and off is not None:
                off = np.full(n_cols, 32768.0)                       # an offset near the data: the subtraction cancels
            if name == 'subnormal' and off is not None:
                off = off * 1e-21
            y32 = r.project(w, channels=cols, offset=off)
            assert_same_bits(y32, project_chain_f32(xs, off, w))
            if name == 'subnormal':
                assert (np.abs(y32[y32 != 0]) < np.finfo(np.float32).tiny).all() and (y32 != 0).mean() > 0.5
                continue
            y64 = r.project(w, channels=cols, offset=off, dtype=np.float64)
            if name == 'special':
                ref64 = project_chain_f64(xs, off, w)
                assert np.array_equal(np.isnan(y64), np.isnan(ref64)) and np.array_equal(y64[np.isinf(ref64)], ref64[np.isinf(ref64)])
                assert np.isnan(y32).any() and np.isinf(y32).any()
                fin = np.isfinite(xs).all(axis=1)
                assert_project_within(y64[fin], xs[fin], off, w, np.float64)
            else:
                assert_project_within(y64, xs, off, w, np.float64)
        r.close()


def test_an_output_does_not_depend_on_its_neighbours_or_the_calls(tmp_cfg):
    rs = np.random.RandomState(11)
    rows, nc = 520, 90
    x = (rs.randn(rows, nc) * 1000).astype(np.float32)
    r, dec = _make(tmp_cfg, x)
    cols = rs.permutation(nc)[:77]
    w, off = rs.randn(77, 130), rs.randn(77)
    for dt in (np.float32, np.float64):
        full = r.project(w, channels=cols, offset=off, dtype=dt)
        for k in (0, 15, 16, 63, 64, 77, 129):
            alone = r.project(w[:, k], channels=cols, offset=off, dtype=dt)
            assert alone.tobytes() == np.ascontiguousarray(full[:, k]).tobytes()
            moved = r.project(w[:, [5, 9, k, 3] + list(range(70))], channels=cols, offset=off, dtype=dt)
            assert np.ascontiguousarray(moved[:, 2]).tobytes() == alone.tobytes()
        for cut in (1, 63, 64, 65, 100, 257, 519):
            two = np.concatenate([r.project(w, 0, cut, channels=cols, offset=off, dtype=dt), r.project(w, cut, None, channels=cols, offset=off, dtype=dt)])
            assert two.tobytes() == full.tobytes()
    r.close()


def _invariance_recording(tmp):
    rs = np.random.RandomState(12)
    x = rs.randint(-30000, 30000, size=(650, 40)).astype(np.int16)
    w, off = rs.randn(40, 70), rs.randn(40) * 1000
    np.save(tmp / 'w.npy', w)
    np.save(tmp / 'off.npy', off)
    return x, w, off


_CHILD = """
import sys, numpy as np, mtscomp_amd
sys.path.insert(0, %r)
tmp, resident, out = sys.argv[1], sys.argv[2] == '1', sys.argv[3]
r = mtscomp_amd.decompress(tmp + '/d.cbin', tmp + '/d.ch', check_after_decompress=False)
if resident:
    for k in (1, 2, 5):
        r[r.chunk_bounds[k] + 3:r.chunk_bounds[k] + 4]
w, off = np.load(tmp + '/w.npy'), np.load(tmp + '/off.npy')
np.save(out, np.concatenate([r.project(w, 33, 640, offset=off, dtype=dt).astype(np.float64).ravel() for dt in (np.float32, np.float64)]))
"""


def test_pieces_and_residency_do_not_change_the_result(tmp_cfg):
    x, w, off = _invariance_recording(tmp_cfg)
    r, dec = _make(tmp_cfg, x)
    r.close()
    want = project_chain_f32(dec[33:640], off, w).ravel()
    outs = []
    for pipe in (None, str(2 * 100 * 40 * 2)):                       # unset, then two chunks to a piece
        for resident in ('0', '1'):
            env = dict(os.environ)
            env.pop('MTS_PIPE_BYTES', None)
            if pipe:
                env['MTS_PIPE_BYTES'] = pipe
            p = tmp_cfg / ('o%d.npy' % len(outs))
            subprocess.run([sys.executable, '-c', _CHILD % os.getcwd(), str(tmp_cfg), resident, str(p)], env=env, check=True, timeout=120)
            outs.append(np.load(p))
    assert all(o.tobytes() == outs[0].tobytes() for o in outs[1:])
    assert_same_bits(outs[0][:want.size].astype(np.float32), want)          # (the float32 half, widened exactly by the child)


def test_lanes_calls_and_repeats_give_identical_bytes(tmp_cfg, monkeypatch):
    x, w, off = _invariance_recording(tmp_cfg)
    r, dec = _make(tmp_cfg, x)
    lanes = [[0, 0]] + ([[0, 1]] if hip.device_count() >= 2 else [])
    for dt in (np.float32, np.float64):
        want = r.project(w, 33, 640, offset=off, dtype=dt)
        assert r.project(w, 33, 640, offset=off, dtype=dt).tobytes() == want.tobytes()
        for devices in lanes:
            two = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', codec=api.HipCodec(devices=devices), check_after_decompress=False)
            assert two.project(w, 33, 640, offset=off, dtype=dt).tobytes() == want.tobytes()
            two.close()
        monkeypatch.setattr(api, 'PROJECT_CALL_BYTES', 1)
        assert r.project(w, 33, 640, offset=off, dtype=dt).tobytes() == want.tobytes()
        monkeypatch.setattr(api, 'PROJECT_CALL_BYTES', 1 << 30)
        monkeypatch.setattr(api, 'PROJECT_OUT_BYTES', 70 * 70 * 8)
        assert r.project(w, 33, 640, offset=off, dtype=dt).tobytes() == want.tobytes()
        monkeypatch.setattr(api, 'PROJECT_OUT_BYTES', 1 << 30)
    # resident chunks are read in place and a scan inserts nothing
    keys = list(range(r.n_chunks))
    r[150:151]
    r[420:421]
    cache = r._cache_for(0)
    before = hip.cache_query(cache, keys).tolist()
    assert sum(b == 40 for b in before) >= 2
    assert_same_bits(r.project(w, 33, 640, offset=off), project_chain_f32(dec[33:640], off, w))
    assert hip.cache_query(cache, keys).tolist() == before
    r.close()


def _dev_chunks(tmp, r):
    data = np.frombuffer((tmp / 'd.cbin').read_bytes() + b'\0' * 256, dtype=np.uint8).copy()
    cbuf = hip.DevBuffer(data.nbytes)
    hip._check(hip.lib().mts_dev_copy(0, None, cbuf.at(), hip._ptr(data), data.nbytes, 0), 'mts_dev_copy')
    offs = np.array(r.chunk_offsets[:-1], np.int64)
    lens = np.diff(np.array(r.chunk_offsets, np.int64))
    return data, cbuf, offs, lens


def test_both_entry_points_and_chunk_status(tmp_cfg):
    x, w, off = _invariance_recording(tmp_cfg)
    r, dec = _make(tmp_cfg, x)
    data, cbuf, offs, lens = _dev_chunks(tmp_cfg, r)
    b = np.array(r.chunk_bounds, np.int64)
    flags, rows, cols = r._flags(), np.diff(b), np.arange(40)
    keep = np.arange(1, 6)
    for dt, chain in ((np.float32, project_chain_f32), (np.float64, None)):
        st_h, y_h = hip.project(0, keep, b[keep], data, offs[keep], lens[keep], rows[keep], 40, np.int16, flags, 133, 577, cols, off, w, dt)
        st_d, y_d, out = hip.dev_project(cbuf, offs[keep], lens[keep], b[keep], rows[keep], 40, np.int16, flags, 133, 577, cols, off, w, dt)
        assert st_h == st_d == [0] * 5
        assert y_h.tobytes() == y_d.tobytes() == r.project(w, 133, 577, offset=off, dtype=dt).tobytes()
        if chain:
            assert_same_bits(y_h, chain(dec[133:577], off, w))
        out.free()
    # a damaged chunk: its status through the C ABI, the others' rows as before; the Reader raises
    bad = data.copy()
    bad[offs[3] + 20:offs[3] + 50] = 0
    st, y = hip.project(0, keep, b[keep], bad, offs[keep], lens[keep], rows[keep], 40, np.int16, flags, 133, 577, cols, off, w, np.float32)
    assert st[2] != hip.CHUNK_OK and [s for i, s in enumerate(st) if i != 2] == [0] * 4
    assert_same_bits(y[:300 - 133], project_chain_f32(dec[133:300], off, w))
    assert_same_bits(y[400 - 133:], project_chain_f32(dec[400:577], off, w))
    r.close()
    (tmp_cfg / 'd.cbin').write_bytes(bad[:-256].tobytes())
    r = mtscomp_amd.decompress(tmp_cfg / 'd.cbin', tmp_cfg / 'd.ch', check_after_decompress=False)
    with pytest.raises(IOError, match='#3'):
        r.project(w, offset=off)
    r.project(w, 0, 300, offset=off)
    r.close()
    cbuf.free()


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_long))


@pytest.mark.parametrize('entry', ['host', 'dev'])
def test_c_abi_argument_errors(entry):
    hip.require_device()
    L = hip.lib()
    nc = 4
    x = np.arange(400, dtype=np.int16).reshape(100, nc)
    z = hip.compress_chunks(x, [0, 100], hip.make_flags(), 6)[0]
    data = np.frombuffer(z + b'\0' * 256, dtype=np.uint8).copy()
    cbuf = hip.DevBuffer(data.nbytes)
    hip._check(L.mts_dev_copy(0, None, cbuf.at(), hip._ptr(data), data.nbytes, 0), 'mts_dev_copy')
    d_out = hip.DevBuffer(1 << 16)
    keep = []

    def call(row0=0, rows=100, rb=10, re=60, cols=(0, 1, 3), off=(1.0, 2.0, 3.0), n_out=2, w=None, osz=4, itemsize=2, flags=hip.make_flags(),
             out=True, n_cols=None):
        a = [np.array(v, dtype=np.int64) for v in ([0], [row0], [0], [len(z)], [rows])]
        c = np.array(cols, dtype=np.int32)
        n_cols = len(c) if n_cols is None else n_cols
        wt = np.ones((max(n_cols, 1), max(n_out, 1))) if w is None else np.array(w, dtype=np.float64)
        o = None if off is None else np.array(off, dtype=np.float64)
        host_out = np.zeros(1 << 16, np.uint8)
        st = np.full(1, 99, np.int32)
        keep.append((a, c, wt, o, host_out, st))
        mid = (nc, itemsize, flags, rb, re, n_cols, c.ctypes.data_as(C.POINTER(C.c_int)), None if o is None else o.ctypes.data_as(C.POINTER(C.c_double)),
               n_out, wt.ctypes.data_as(C.POINTER(C.c_double)), osz)
        if entry == 'host':
            rc = L.mts_project(0, 0, 1, _lp(a[0]), _lp(a[1]), hip._ptr(data), _lp(a[2]), _lp(a[3]), _lp(a[4]), *mid,
                               hip._ptr(host_out) if out else None, st.ctypes.data_as(C.POINTER(C.c_int)))
        else:
            rc = L.mts_dev_project(0, None, cbuf.at(), _lp(a[2]), _lp(a[3]), _lp(a[1]), _lp(a[4]), 1, *mid, d_out.at() if out else None,
                                   st.ctypes.data_as(C.POINTER(C.c_int)))
        return rc, int(st[0]), L.mts_last_error().decode(), host_out

    rc, st, _, host_out = call()
    assert (rc, st) == (0, 0)
    got = np.empty((50, 2), np.float32)
    if entry == 'host':
        got = host_out[:got.nbytes].view(np.float32).reshape(50, 2)
    else:
        hip._check(L.mts_dev_copy(0, None, hip._ptr(got), d_out.at(), got.nbytes, 1), 'mts_dev_copy')
    assert_same_bits(got, project_chain_f32(x[10:60][:, [0, 1, 3]], [1.0, 2.0, 3.0], np.ones((3, 2))))
    assert call(rb=40, re=40, out=False)[:2] == (0, 0)                # an empty range: MTS_OK, nothing written
    assert call(off=None)[:2] == (0, 0)
    nan_w, inf_w = np.ones((3, 2)), np.ones((3, 2))
    nan_w[2, 1], inf_w[0, 0] = np.nan, -np.inf
    for bad, word in ((dict(cols=(), n_cols=0), 'columns'), (dict(cols=[0] * 1025), 'columns'), (dict(n_out=0), 'outputs'), (dict(n_out=1025), 'outputs'),
                      (dict(w=nan_w), 'not finite'), (dict(w=inf_w), 'not finite'), (dict(off=(1.0, np.nan, 0.0)), 'not finite'),
                      (dict(off=(np.inf, 0.0, 0.0)), 'not finite'), (dict(osz=2), 'itemsize'), (dict(osz=16), 'itemsize'),
                      (dict(cols=(0, 4, 1)), 'out of range'), (dict(cols=(-1, 0, 1)), 'out of range'), (dict(rb=-1), 'rows'), (dict(rb=50, re=20), 'rows'),
                      (dict(out=False), 'output buffer'), (dict(row0=20), 'cover'), (dict(rows=50), 'cover'), (dict(re=101), 'cover'),
                      (dict(rows=0), 'chunk 0'), (dict(itemsize=3), 'itemsize'), (dict(flags=hip.FLAG_FLOAT, itemsize=2), 'float items')):
        rc, st, msg, _ = call(**bad)
        assert rc == -1, bad                                        # MTS_E_ARG ...
        assert word in msg, (bad, msg)                              # ... with its message ...
        assert st == 99, bad                                        # ... before anything ran
    d_out.free()
    cbuf.free()


def test_whitening_end_to_end(tmp_cfg):
    rs = np.random.RandomState(13)
    mix = rs.randn(24, 24)
    x = (rs.randn(600, 24) @ mix * 300 + rs.randn(24) * 500).astype(np.int16)
    r, dec = _make(tmp_cfg, x)
    c = r.cov()
    W = api.whitening_weights(c.cov[0], 1e-6)
    y = r.project(W, offset=c.mean[0], dtype=np.float64)
    assert_project_within(y, dec, c.mean[0], W, np.float64)
    cy = np.cov(y, rowvar=False)
    assert np.abs(cy - np.eye(24)).max() < 1e-6                     # whitened: unit covariance
    r.close()
