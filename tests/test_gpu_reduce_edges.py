"""window_stats and decimate on the MI355X at the edges of their kernels, against references that do not share the kernels'
arithmetic (tests/stats_oracle.py: exact fsum / Python-int sums and a bound from the reduction depth; tests/decimate_oracle.py:
an integer FIR on exactly representable inputs, and a copy of k_decimate's launch plan that picks the cases and checks that
every branch ran):
  * window_stats: all ten item types (every k_stats_tiles / k_stats_combine instantiation) with full-range, constant min / max,
    alternating and special float columns; the tiling edges (tiles of 512 rows, the 32-row unrolled body and its tail, column
    groups of 64 with duplicate picks across them, 1- to 1537-row chunks, windows that start and end inside chunks); several
    MTS_PIPE_BYTES pieces with some chunks resident;
  * decimate: every dec_plan branch for float32 and float64 output, n_out at and beside tile multiples, supports that start
    and end on chunk boundaries and one row beside them, chunks shorter than both L and q, edge='zeros' inside a chunk, the
    device entry, an empty valid range; 8-byte integers near 2^63 / 2^64 and float32 subnormals."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import mtscomp_amd
from mtscomp_amd import api, hip
from oracle import oracle as O
from tests.codec_oracle import OracleCodec
from tests.decimate_oracle import (DECIMATE_PLAN_CASES, PLAN_BRANCHES, assert_within_bound, dyadic_taps, exact_tap_budget,
                                   fir_decimate, fir_decimate_exact, fir_decimate_f64, plan_branches, plan_n_outs)
from tests.stats_oracle import assert_stats_equal, assert_stats_exact_bound, numpy_window_stats

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


@pytest.fixture
def tmp_cfg(tmp_path, monkeypatch):
    monkeypatch.setattr(api, 'CONFIG_PATH', tmp_path / '.mtscomp')
    api.set_codec(None)
    return tmp_path


def value_families(dtype, rows, nc, rs):
    """Columns 0..3: constant min, constant max, alternating min / max, uniform over the full range (integers; uint64 >= 2^63 and
    int64 near -2^63 included), or (floats) subnormals with +-0, +-inf and NaN, magnitudes whose squares overflow (float64) or
    reach 1e74 (float32), +-0 with a few normals; the rest uniform / normal."""
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        fi = np.finfo(dt)
        x = (rs.randn(rows, nc) * 100).astype(dt)
        x[:, 0] = (rs.randint(-1000, 1000, rows) * fi.smallest_subnormal).astype(dt)
        x[::7, 0] = -0.0
        x[rows // 3, 0], x[rows // 2, 0], x[2 * rows // 3, 0] = np.inf, -np.inf, np.nan
        x[:, 1] = (rs.randn(rows) * (1e200 if dt == np.float64 else 1e37)).astype(dt)
        x[:, 2] = np.where(np.arange(rows) % 2, fi.max, fi.min)          # alternating: the sum cancels, the squares overflow for float64
        x[:, 3] = np.where(rs.rand(rows) < 0.99, 0.0, rs.randn(rows)).astype(dt) * np.where(rs.rand(rows) < 0.5, -1, 1).astype(dt)
        return x
    info = np.iinfo(dt)
    lo, hi = np.array(info.min, dt), np.array(info.max, dt)
    if dt.itemsize == 8:
        x = rs.randint(int(lo), int(hi) + (dt.kind == 'u'), size=(rows, nc), dtype=dt)
        x[:rows // 4, 3] = hi - rs.randint(0, 1000, rows // 4).astype(dt)                # next to the top
        x[rows // 4:rows // 2, 3] = lo + rs.randint(0, 1000, rows // 2 - rows // 4).astype(dt)   # next to the bottom
    else:
        x = rs.randint(int(lo), int(hi) + 1, size=(rows, nc), dtype=np.int64).astype(dt)
    x[:, 0] = lo
    x[:, 1] = hi
    x[:, 2] = np.where(np.arange(rows) % 2, hi, lo)
    return x


def _file(tmp, x, sample_rate, chunk_duration=1.0):
    raw = tmp / 'd.bin'
    x.tofile(raw)
    mtscomp_amd.compress(raw, tmp / 'd.cbin', tmp / 'd.ch', sample_rate=float(sample_rate), n_channels=x.shape[1], dtype=x.dtype,
                         chunk_duration=chunk_duration, do_time_diff=x.dtype.kind != 'f', check_after_compress=False)
    r = mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', check_after_decompress=False)
    ro = mtscomp_amd.decompress(tmp / 'd.cbin', tmp / 'd.ch', codec=OracleCodec(), check_after_decompress=False)
    dec = ro[:]                                                         # the reference: the oracle's decode, never the device's
    ro.close()
    assert np.array_equal(dec, x, equal_nan=True)                       # (no time diff for floats: the values come back as they are)
    return r, dec


def _chunks(x, bounds, flags):
    """The chunks of x cut at `bounds`, compressed: (one byte buffer, offsets, lengths); the oracle decodes them back to x."""
    z = hip.compress_chunks(x, bounds, flags, 6)
    for i in (0, len(z) // 2, len(z) - 1):
        rc, a = O.decompress_chunk(z[i], bounds[i + 1] - bounds[i], x.shape[1], x.dtype.name, flags)
        assert rc == 0 and np.array_equal(a, x[bounds[i]:bounds[i + 1]], equal_nan=True)
    lens = np.array([len(c) for c in z], np.int64)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    return b''.join(z) + b'\0' * 16, offs, lens


def _as_reader_result(res):
    """The C ABI's partials as Reader.window_stats completes them (sumsq as float64, mean, rms)."""
    cnt = res['count']
    sumsq = res['sumsq'].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return dict(count=cnt, min=res['min'], max=res['max'], sum=res['sum'], sumsq=sumsq,
                    mean=res['sum'].astype(np.float64) / cnt[:, None], rms=np.sqrt(sumsq / cnt[:, None]))


# ---- window statistics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_window_stats_every_item_type(tmp_cfg, dtype):
    rows, nc, rate = 2600, 6, 700                                      # chunks of 700 rows, the last of 500
    x = value_families(dtype, rows, nc, np.random.RandomState(DTYPES.index(dtype)))
    r, dec = _file(tmp_cfg, x, rate)
    b = r.chunk_bounds
    checked = 0
    for window, start, stop, channels in ((None, 0, rows, slice(None)), (513, 0, rows, slice(None)), (700, 5, rows - 3, [5, 0, 3, 0]),
                                          (31, 690, 1450, slice(None)), (1, 695, 705, [2, 1])):
        got = r.window_stats(window, start, stop, channels=channels)
        cols = list(range(nc))[channels] if isinstance(channels, slice) else channels
        w = window or stop - start
        assert_stats_equal(got, numpy_window_stats(dec, w, start, stop, cols), dtype)
        checked += assert_stats_exact_bound(got, dec, b, start, stop, w, cols)
    # the device entry on the same chunks: the same bits
    flags = r._flags()
    data = (tmp_cfg / 'd.cbin').read_bytes()
    offs, lens = np.array(r.chunk_offsets[:-1]), np.diff(r.chunk_offsets)
    cbuf = hip.DevBuffer(len(data) + 256)
    cbuf.upload(np.frombuffer(data, np.uint8))
    bb = np.array(b)
    st_h, h = hip.window_stats(0, range(len(lens)), bb[:-1], data, offs, lens, np.diff(bb), nc, dtype, flags, 0, rows, 513, range(nc))
    st_d, d, out = hip.dev_window_stats(cbuf, offs, lens, bb[:-1], np.diff(bb), nc, dtype, flags, 0, rows, 513, range(nc))
    assert st_h == st_d == [0] * len(lens)
    for key in ('count', 'min', 'max', 'sum', 'sumsq'):
        assert h[key].tobytes() == d[key].tobytes(), key
    assert_stats_exact_bound(d, dec, b, 0, rows, 513, range(nc))
    out.free()
    cbuf.free()
    r.close()
    print('%s: %d (window, column) sums within the exact bound' % (dtype, checked))


CHUNK_ROWS = [1, 31, 32, 33, 511, 512, 513, 1537, 1, 1, 33, 512, 2, 1537]


@pytest.mark.parametrize('nc', [1, 63, 64, 65, 129])
@pytest.mark.parametrize('dtype', ['float32', 'int64', 'uint16'])
def test_window_stats_tiling_edges(dtype, nc):
    bounds = np.concatenate(([0], np.cumsum(CHUNK_ROWS))).astype(np.int64)
    rows = int(bounds[-1])
    rs = np.random.RandomState(nc)
    x = value_families(dtype, rows, nc, rs) if nc >= 4 else value_families(dtype, rows, 4, rs)[:, 3:3 + nc].copy()
    ints = np.dtype(dtype).kind != 'f'
    flags = hip.make_flags(ints, ints and nc > 1, 'F')                  # (no diffs for floats: their decode is the input)
    cdata, offs, lens = _chunks(x, bounds, flags)
    cbuf = hip.DevBuffer(len(cdata) + 256)
    cbuf.upload(np.frombuffer(cdata, np.uint8))
    # duplicate picks that cross the 64-column groups
    cols = [nc - 1, 0, min(63, nc - 1), min(64, nc - 1), 0, nc - 1] + [int(c) for c in rs.randint(0, nc, 70)]
    starts_stops = [(0, rows), (bounds[4] + 7, bounds[8] - 5), (bounds[1] - 1, bounds[3] + 1), (bounds[7] + 100, bounds[7] + 1537 + 40)]
    for window in (1, 31, 32, 33, 512, 513, 1536, 1538, None):
        for start, stop in starts_stops:
            start, stop = int(start), int(stop)
            if window == 1 and stop - start > 200:
                stop = start + 200                                    # (window 1: every result is one item)
            w = window or stop - start
            keep = [i for i in range(len(lens)) if bounds[i] < stop and bounds[i + 1] > start]
            args = (bounds[keep], np.diff(bounds)[keep], nc, dtype, flags, start, stop, w)
            st, res = hip.window_stats(0, keep, bounds[keep], cdata, offs[keep], lens[keep], np.diff(bounds)[keep], nc, dtype, flags,
                                       start, stop, w, cols)
            assert st == [0] * len(keep)
            assert_stats_equal(_as_reader_result(res), numpy_window_stats(x, w, start, stop, cols), dtype)
            assert_stats_exact_bound(res, x, bounds, start, stop, w, cols)
            if window in (31, 513, None):
                st_d, d, out = hip.dev_window_stats(cbuf, offs[keep], lens[keep], *args, cols)
                assert st_d == st
                for key in res:
                    assert res[key].tobytes() == d[key].tobytes(), key
                out.free()
    cbuf.free()


_PIECES_SCRIPT = '''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import mtscomp_amd
r = mtscomp_amd.decompress(sys.argv[2], sys.argv[3], check_after_decompress=False)
n = r.n_samples
r[r.chunk_bounds[2] + 3:r.chunk_bounds[2] + 5]                   # some chunks resident in the cache, the others decoded
r[r.chunk_bounds[6]:r.chunk_bounds[6] + 1]
out = {}
for i, (w, a, b) in enumerate(((997, 0, n), (3000, 1234, n - 77), (None, 5, n - 5))):
    s = r.window_stats(w, a, b)
    for k in ('count', 'min', 'max', 'sum', 'sumsq'):
        out['%s_%d' % (k, i)] = s[k]
np.savez(sys.argv[4], **out)
'''


@pytest.mark.parametrize('dtype', ['int16', 'float32'])
def test_window_stats_pieces_do_not_change_the_result(tmp_cfg, dtype):
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
        if pipe:
            env['MTS_PIPE_BYTES'] = pipe
        p = tmp_cfg / ('o%d.npz' % len(outs))
        subprocess.run([sys.executable, str(script), str(ROOT), str(tmp_cfg / 'd.cbin'), str(tmp_cfg / 'd.ch'), str(p)], env=env,
                       check=True, timeout=300)
        outs.append(dict(np.load(p)))
    assert sorted(outs[0]) == sorted(outs[1])
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    b = list(range(0, rows + 1, 3000))
    got = {k: outs[1][k + '_1'] for k in ('sum', 'sumsq')}
    assert_stats_exact_bound(got, x, b, 1234, rows - 77, 3000, range(nc))


# ---- decimation ---------------------------------------------------------------------------------------------------------------------
def _tiny_chunked_recording(rs, rows=15000, nc=130):
    """int16 items in [-2047, 2047] (exact in float32 with sum |k| <= 2^13), chunks of 1 to 1537 rows, runs of tiny ones."""
    sizes, total = [], 0
    while total < rows:
        n = int(rs.choice([1, 1, 2, 3, 5, 17, 64, 300, 1000, 1537]))
        sizes += [n] if n > 5 else [n] * int(rs.randint(1, 9))
        total = sum(sizes)
    bounds = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    x = np.clip(np.cumsum(rs.randint(-300, 301, size=(int(bounds[-1]), nc)), axis=0), -2047, 2047).astype(np.int16)
    x[rs.randint(0, x.shape[0], 50), rs.randint(0, nc, 50)] = 2047
    x[rs.randint(0, x.shape[0], 50), rs.randint(0, nc, 50)] = -2047
    return x, bounds


def test_decimate_every_plan_branch(capsys):
    rs = np.random.RandomState(20261016)
    x, bounds = _tiny_chunked_recording(rs)
    rows, nc = x.shape
    flags = hip.make_flags(True, True, 'F')
    cdata, offs, lens = _chunks(x, bounds, flags)
    cbuf = hip.DevBuffer(len(cdata) + 256)
    cbuf.upload(np.frombuffer(cdata, np.uint8))
    n_rows = np.diff(bounds)
    reached, calls, exact_calls = set(), 0, 0
    col_counts = [1, 2, 63, 64, 65, 130]
    for ci, (q, n_taps, f) in enumerate(DECIMATE_PLAN_CASES):
        for oi, n_out in enumerate(plan_n_outs(n_taps, q, f)):
            mode = (ci * 3 + oi) % 6
            span = (n_out - 1) * q                                     # newest row of the last output - that of the first
            d = mode % 3 - 1
            if mode < 3:                                               # the lowest row of the support at a boundary, or beside it
                ok = [int(b) for b in bounds[1:-1] if b + d + n_taps - 1 + span < rows and b + d >= 0]
                first = rs.choice(ok) + d + n_taps - 1
            else:                                                      # the newest row of the last output at a boundary, or beside it
                ok = [int(b) for b in bounds[1:-1] if b + d - span - (n_taps - 1) >= 0 and b + d < rows]
                first = rs.choice(ok) + d - span
            first = int(first)
            lo, hi = first - (n_taps - 1), first + span + 1
            if (ci + oi) % 2:                                          # edge='zeros' inside a chunk
                vb, ve = lo + int(rs.randint(1, max(2, (hi - lo) // 2))), hi - int(rs.randint(0, q))
                vb += int(vb in bounds)
                ve = max(ve, vb + 1)
            else:
                vb, ve = 0, rows
            c0 = int(np.searchsorted(bounds, max(lo, vb), 'right') - 1)
            c1 = int(np.searchsorted(bounds, min(hi, ve) - 1, 'right') - 1)
            keep = np.arange(c0, c1 + 1)
            n_cols = col_counts[(ci + 2 * oi) % len(col_counts)]
            cols = rs.permutation(nc)[:n_cols] if n_cols < nc else rs.permutation(nc)
            if n_cols > 3:
                cols[-1] = cols[0]                                     # (a duplicate pick)
            xs = x[:, cols]
            k, s, taps = dyadic_taps(rs, n_taps, exact_tap_budget(2047, f))
            st, got = hip.decimate(0, keep, bounds[keep], cdata, offs[keep], lens[keep], n_rows[keep], nc, np.int16, flags, vb, ve, first,
                                   n_out, q, taps, f, cols)
            assert st == [0] * keep.size
            where = dict(q=q, n_taps=n_taps, dtype=f, n_out=n_out, first=first, vb=vb, ve=ve, n_cols=n_cols)
            want = fir_decimate(xs, 0, vb, ve, first, n_out, q, taps, f)
            exact = fir_decimate_exact(xs, 0, vb, ve, first, n_out, q, k, s, f)
            assert got.tobytes() == exact.tobytes(), (where, np.argwhere(got != exact)[:5])
            assert got.tobytes() == want.tobytes(), where
            calls += 1
            exact_calls += 1
            reached |= plan_branches(n_taps, q, f, n_out)
            if (n_rows[keep] < min(n_taps, q)).any():
                reached.add('chunk<L,q')
            if oi == 0:                                                # the device entry: the same bits; taps that round
                st_d, got_d, out = hip.dev_decimate(cbuf, offs[keep], lens[keep], bounds[keep], n_rows[keep], nc, np.int16, flags, vb, ve,
                                                    first, n_out, q, taps, f, cols)
                assert st_d == st and got_d.tobytes() == got.tobytes(), where
                out.free()
                taps_r = rs.randn(n_taps)
                st, got = hip.decimate(0, keep, bounds[keep], cdata, offs[keep], lens[keep], n_rows[keep], nc, np.int16, flags, vb, ve,
                                       first, n_out, q, taps_r, f, cols)
                assert got.tobytes() == fir_decimate(xs, 0, vb, ve, first, n_out, q, taps_r, f).tobytes(), where
                y64, a = fir_decimate_f64(xs, vb, ve, first, n_out, q, taps_r)
                assert_within_bound(got, y64, a, n_taps, f)
                calls += 1
    # an empty valid range on the device entry: zeros, whatever the output buffer held
    out = hip.DevBuffer(64 * 130 * 8 + 256)
    out.upload(np.full(64 * 130, np.nan))
    for f in ('float32', 'float64'):
        st, y, _ = hip.dev_decimate(cbuf, offs[:3], lens[:3], bounds[:3], n_rows[:3], nc, np.int16, flags, 1, 1, 5, 64, 2, [0.5, 0.25, 1.0],
                                    f, np.arange(nc), out=out)
        assert y.dtype == np.dtype(f) and y.shape == (64, nc) and not np.any(y) and not np.signbit(y).any()
        calls += 1
    out.free()
    cbuf.free()
    missing = (PLAN_BRANCHES | {'chunk<L,q'}) - reached
    with capsys.disabled():
        print('\ndec_plan branches reached (%d calls, %d exact): %s' % (calls, exact_calls, ' '.join(sorted(reached))))
    assert not missing, sorted(missing)


@pytest.mark.parametrize('dtype', ['int64', 'uint64'])
def test_decimate_8_byte_items_near_the_top(tmp_cfg, dtype):
    rows, nc = 2000, 5
    rs = np.random.RandomState(11)
    info = np.iinfo(dtype)
    lo, hi = np.array(info.min, dtype), np.array(info.max, dtype)
    x = np.empty((rows, nc), dtype)
    x[:, 0] = hi - rs.randint(0, 1 << 12, rows).astype(dtype)                    # rounds up to 2^63 / 2^64 in float32 and float64
    x[:, 1] = lo + rs.randint(0, 1 << 12, rows).astype(dtype)
    x[:, 2] = np.array(1 << (53 if dtype == 'int64' else 63), dtype) + rs.randint(0, 1 << 12, rows).astype(dtype)   # (ties to even)
    x[:, 3] = rs.randint(int(lo), int(hi), rows, dtype=dtype)
    x[:, 4] = np.where(np.arange(rows) % 2, hi, lo)
    r, dec = _file(tmp_cfg, x, 600)
    for f in (np.float32, np.float64):
        for q, taps, start, stop, edge in ((3, [1.0], 0, None, 'zeros'), (2, [0.5, -0.25, 0.125], 7, 1999, 'recording'),
                                          (5, rs.randn(33), 100, 1800, 'recording'), (1, [2.0 ** -70], 0, None, 'zeros')):
            got = r.decimate(q, start, stop, taps=taps, edge=edge, dtype=f)
            i0, i1 = start, rows if stop is None else stop
            t = np.asarray(taps, np.float64)
            vb, ve = (i0, i1) if edge == 'zeros' else (0, rows)
            want = fir_decimate(dec, 0, vb, ve, i0 + (t.size - 1) // 2, got.shape[0], q, t, f)
            assert got.tobytes() == want.tobytes(), (f, q, np.argwhere(got != want)[:5])
            y64, a = fir_decimate_f64(dec, vb, ve, i0 + (t.size - 1) // 2, got.shape[0], q, t)
            assert_within_bound(got, y64, a, t.size, f)
        one = r.decimate(1, taps=[1.0], dtype=f)                       # taps [1]: the conversion alone, as numpy's astype
        assert one.tobytes() == dec.astype(f).tobytes()
    r.close()


def test_decimate_float32_subnormals(tmp_cfg):
    rows, nc = 3000, 4
    rs = np.random.RandomState(12)
    tiny = np.finfo(np.float32).tiny
    x = (rs.randn(rows, nc) * tiny * 4).astype(np.float32)              # normals near the bottom and subnormals
    x[:, 1] = (rs.randint(-50, 50, rows) * np.finfo(np.float32).smallest_subnormal).astype(np.float32)
    x[::5, 2] = -0.0
    assert (np.abs(x[:, 0]) < tiny).sum() > rows // 10
    r, dec = _file(tmp_cfg, x, 1000)
    for q, taps in ((2, [0.5, 0.25, 0.125, -0.375]), (3, [2.0 ** -10, 1.0, -2.0 ** -20]), (1, [0.75]), (4, rs.randn(17) * 0.01)):
        for f in (np.float32, np.float64):
            got = r.decimate(q, taps=taps, edge='recording', dtype=f)
            t = np.asarray(taps, np.float64)
            want = fir_decimate(dec, 0, 0, rows, (t.size - 1) // 2, got.shape[0], q, t, f)
            assert got.tobytes() == want.tobytes(), (q, f, np.argwhere(got != want)[:5])
            if f == np.float32:
                assert np.any((got != 0) & (np.abs(got) < tiny)), 'no subnormal result'
    r.close()
