"""Randomised parity of the reduction extensions on a GPU box: random recordings (all ten item types, channel counts, chunk
durations down to one row, time / spatial diff, chunk order, value families) compressed with mtscomp_amd.compress, read back
through Reader.window_stats and Reader.decimate with random cache states (MTSCOMP_DEVICE_CACHE_GB, a random prefix read so
that some chunks are resident), one lane or two on device 0, random windows / ranges / channels, q from 1 to 400, taps None
or random (1 to 8192 of them, dyadic and exact in the output type or not), both edges and both output types.  Every result
is compared with references over the oracle's decode (never the device's): window_stats with assert_stats_equal and the
exact fsum / Python-int bound; decimate bit for bit with the numpy restatement in the output type, bit for bit with the
integer FIR where the inputs are exactly representable, and within the float64 bound.

    python tools/fuzz_reduce_gpu.py [seed] [seconds]
"""
import os
import sys
import tempfile
import time
import traceback
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import mtscomp_amd  # noqa: E402
from mtscomp_amd import api  # noqa: E402
from tests.codec_oracle import OracleCodec  # noqa: E402
from tests.decimate_oracle import (assert_within_bound, dyadic_taps, exact_tap_budget, fir_decimate, fir_decimate_exact,  # noqa: E402
                                   fir_decimate_f64)
from tests.stats_oracle import assert_stats_equal, assert_stats_exact_bound, numpy_window_stats  # noqa: E402

DTYPES = ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64', 'float32', 'float64']


def values(r, dt, nt, nc):
    """One of: a random walk, small integers (exact for the integer FIR), the full range, constant / alternating extremes,
    float specials."""
    kind = r.randint(0, 5)
    if kind == 0:
        x = np.cumsum(r.randint(-50, 51, size=(nt, nc)), axis=0)
    elif kind == 1:
        x = r.randint(-2047, 2048, size=(nt, nc))
    elif dt.kind == 'f':
        x = r.randn(nt, nc) * 10. ** r.randint(-40, 40)
        if kind == 3:
            x[r.randint(0, nt, 3), r.randint(0, nc, 3)] = r.choice([np.nan, np.inf, -np.inf, -0.0])
        return x.astype(dt), kind
    else:
        info = np.iinfo(dt)
        lo, hi = np.array(info.min, dt), np.array(info.max, dt)
        if kind == 2:
            return r.randint(int(lo), int(hi) + (dt.kind == 'u' or dt.itemsize < 8), size=(nt, nc), dtype=dt if dt.itemsize == 8 else np.int64).astype(dt), kind
        x = np.empty((nt, nc), dt)
        x[:] = lo if kind == 3 else hi
        x[::2] = hi if kind == 3 else lo
        return x, kind
    if dt.kind == 'u':
        x = x - x.min()
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        x = np.clip(x, max(int(info.min), -2 ** 62), min(int(info.max), 2 ** 62))
    return x.astype(dt), kind


def channels(r, nc):
    k = r.randint(0, 4)
    if k == 0:
        return slice(None)
    if k == 1:
        return int(r.randint(-nc, nc))
    if k == 2:
        return slice(int(r.randint(0, nc)), None, int(r.randint(1, 4)))
    return [int(c) for c in r.randint(0, nc, size=r.randint(1, 100))]


def cols_of(ch, nc):
    if isinstance(ch, int):
        return [ch % nc], True
    if isinstance(ch, slice):
        return list(range(*ch.indices(nc))), False
    return list(ch), False


def limit(rd, a, b, nt, step, n_cols, cap):
    """(a, b) or a shorter range from the same start with at most `cap` // n_cols steps (the references run on the host)."""
    i0 = rd._validate_index(a, 0)
    i1 = max(i0, rd._validate_index(b, nt))
    n = max(1, cap // max(1, n_cols))
    return (a, b) if -(-(i1 - i0) // step) <= n else (i0, i0 + n * step)


def check_stats(rd, dec, r, nt, nc, ctx):
    window = None if r.randint(0, 6) == 0 else int(r.choice([1, 2, 31, 32, 33, 100, 511, 512, 513, 1000, 4000, 30001]))
    a, b = sorted(int(v) for v in r.randint(-nt - 3, nt + 3, size=2))
    ch = channels(r, nc)
    n_cols = len(cols_of(ch, nc)[0])
    a, b = limit(rd, a, b, nt, window or nt + 1, n_cols, 20000)          # (window, column) results
    a, b = limit(rd, a, b, nt, 1, n_cols, 400000)                        # items
    ctx['case'] = ('window_stats', window, a, b, ch)
    got = rd.window_stats(window, a, b, channels=ch)
    i0, i1 = got.start, got.stop
    cols, squeeze = cols_of(ch, nc)
    w = window or max(i1 - i0, 1)
    if cols:
        assert_stats_equal(got, numpy_window_stats(dec, w, i0, i1, cols), dec.dtype, squeeze=squeeze)
        if i1 > i0:
            assert_stats_exact_bound(got, dec, rd.chunk_bounds, i0, i1, w, cols, parts=rd._n_lanes(), squeeze=squeeze)


def check_decimate(rd, dec, r, nt, nc, small_ints, ctx):
    q = int(r.choice([1, 2, 3, 5, 12, 40, 97, 128, 129, 255, 256, 257, 400])) if r.randint(0, 2) else int(r.randint(1, 401))
    a, b = sorted(int(v) for v in r.randint(-nt - 3, nt + 3, size=2))
    ch = channels(r, nc)
    edge = ['zeros', 'recording'][r.randint(0, 2)]
    f = [np.float32, np.float64][r.randint(0, 2)]
    exact = None
    kt = r.randint(0, 3)
    if kt == 0 and q > 1:
        taps = None
    else:
        n_taps = int(r.choice([1, 2, 3, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1000, 8192])) if r.randint(0, 2) else int(r.randint(1, 8193))
        if kt == 1 and small_ints:
            k, s, taps = dyadic_taps(r, n_taps, exact_tap_budget(max(1, int(np.abs(dec.astype(np.int64)).max())), f))
            exact = (k, s)
        else:
            taps = r.randn(n_taps)
    n_taps = 20 * q + 1 if taps is None else len(taps)
    if len(cols_of(ch, nc)[0]) * n_taps > 2_000_000:
        ch = [int(c) for c in r.randint(0, nc, size=2)]
    a, b = limit(rd, a, b, nt, q, len(cols_of(ch, nc)[0]) * n_taps, 30_000_000)      # (output, column, tap) products
    ctx['case'] = ('decimate', q, a, b, ch, edge, f.__name__, 'default' if taps is None else len(taps), 'exact' if exact else '')
    got = rd.decimate(q, a, b, channels=ch, taps=taps, edge=edge, dtype=f)
    i0 = rd._validate_index(a, 0)
    i1 = max(i0, rd._validate_index(b, nt))
    t = api.decimate_taps(q) if taps is None else np.asarray(taps, np.float64)
    cols, squeeze = cols_of(ch, nc)
    if not cols:
        return
    got = got.reshape(-1, len(cols))
    vb, ve = (i0, i1) if edge == 'zeros' else (0, nt)
    first, n_out = i0 + (t.size - 1) // 2, -(-(i1 - i0) // q)
    assert got.shape == (n_out, len(cols)) and got.dtype == f
    x = dec[:, cols]
    want = fir_decimate(x, 0, vb, ve, first, n_out, q, t, f)
    assert got.tobytes() == want.tobytes() or np.array_equal(got, want, equal_nan=True), 'restatement'
    if exact:
        assert got.tobytes() == fir_decimate_exact(x, 0, vb, ve, first, n_out, q, exact[0], exact[1], f).tobytes(), 'exact'
    with np.errstate(invalid='ignore'):
        big = np.abs(np.where(np.isfinite(x), x, 0)).max(initial=0) * np.abs(t).sum() >= np.finfo(f).max / 4
    if not big:                                            # (float64 items beyond float32's range: the restatement alone)
        y64, amp = fir_decimate_f64(x, vb, ve, first, n_out, q, t)
        assert_within_bound(got, y64, amp, t.size, f)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    budget = float(sys.argv[2]) if len(sys.argv) > 2 else 60.
    r = np.random.RandomState(seed)
    tmp = Path(tempfile.mkdtemp(prefix='mtsfuzz_'))
    api.CONFIG_PATH = tmp / '.mtscomp'
    t0 = time.time()
    files = calls = bad = 0
    while time.time() - t0 < budget:
        dt = np.dtype(r.choice(DTYPES))
        nc = int(r.choice([1, 2, 3, 16, 63, 64, 65, 130, 385]))
        rate = float(r.choice([100., 1000., 2500.]))
        chunk_duration = float(r.choice([0.01, 0.05, 0.5, 1., 3.]))
        nt = int(r.choice([1, 7, 500, 4000, 12000]) * r.uniform(0.5, 1.5)) + 1
        if nc * nt > 2_000_000:
            nt = 2_000_000 // nc
        arr, kind = values(r, dt, nt, nc)
        raw, out, meta = tmp / 'd.bin', tmp / 'd.cbin', tmp / 'd.ch'
        arr.tofile(raw)
        os.environ['MTSCOMP_DEVICE_CACHE_GB'] = str(r.choice(['8', '0', '0.00005', '0.001']))
        kw = dict(chunk_duration=chunk_duration, do_spatial_diff=bool(r.randint(0, 2)) and dt.kind != 'f',
                  do_time_diff=bool(r.randint(0, 4) > 0), chunk_order=str(r.choice(['F', 'C'])))
        mtscomp_amd.compress(raw, out, meta, sample_rate=rate, n_channels=nc, dtype=dt, check_after_compress=False, **kw)
        ro = mtscomp_amd.decompress(out, meta, codec=OracleCodec(), check_after_decompress=False)
        dec = ro[:]                                        # the reference: the oracle's decode
        ro.close()
        lanes = [[0], [0, 0]][r.randint(0, 2)]
        rd = mtscomp_amd.decompress(out, meta, codec=api.HipCodec(devices=lanes), check_after_decompress=False)
        if r.randint(0, 2):
            rd[:int(r.randint(0, nt + 1))]                 # a prefix read: some chunks resident
        small = dt.kind in 'iu' and kind in (0, 1) or (dt.kind == 'f' and kind == 1)
        small = small and np.array_equal(dec, np.round(dec)) and int(np.abs(dec.astype(np.float64)).max(initial=0)) < 2 ** 20
        files += 1
        for _ in range(10):
            ctx = {}
            try:
                if r.randint(0, 2):
                    check_stats(rd, dec, r, nt, nc, ctx)
                else:
                    check_decimate(rd, dec, r, nt, nc, small, ctx)
                print('ok', dt, (nt, nc), kw, lanes, ctx['case'], flush=True)
            except AssertionError:
                bad += 1
                print('MISMATCH', dt, (nt, nc), kw, os.environ['MTSCOMP_DEVICE_CACHE_GB'], lanes, ctx.get('case'), flush=True)
                traceback.print_exc(limit=3)
            calls += 1
        rd.close()
        for p in (raw, out, meta):
            p.unlink()
    print('reduce fuzz seed %d: %d files, %d calls, %d mismatches' % (seed, files, calls, bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
