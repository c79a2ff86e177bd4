"""Per-window statistics on the device against what a user does today; prints one JSON line.

  device  the configs[1] recording in HBM (60 s x 385 int16 of the synthetic generator, compressed on the device):
          mts_dev_window_stats (windows of 30000 and 3001 rows) against mts_dev_decompress_chunks of the same chunks, in one
          process, the runs alternated, after warm-ups.  Both inflate every chunk; the difference is the reduction.
  file    a `--seconds` s .cbin on tmpfs: Reader.window_stats(30000) against the status quo -- Reader slices of 30 chunks at a
          time reduced with numpy to the same fields (min, max, int64 sum, exact sum of squares per 30000-row window) -- over the
          first `--quo-seconds` s of the same file.  Both as raw (decoded) GB/s.

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--device-only keeps that run short)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
import mtscomp_amd  # noqa: E402
from mtscomp_amd import hip  # noqa: E402

RATE, NC = 30000, 385


def device_part(reps, warmup):
    n = 60
    chunk_bytes = RATE * NC * 2
    raw = hip.DevBuffer(n * chunk_bytes)
    hip.dev_synth_int16(raw, 0, 0, n * RATE, NC, 0)
    cb = (hip.compress_bound(chunk_bytes) + 255) // 256 * 256
    cbuf, back = hip.DevBuffer(n * cb), hip.DevBuffer(n * chunk_bytes)
    bounds = np.arange(n + 1, dtype=np.int64) * RATE
    slots = np.arange(n, dtype=np.int64) * cb
    sizes = np.zeros(n, dtype=np.int64)
    flags = hip.make_flags(True, False, 'F')
    hip.dev_compress_chunks(raw, NC, 2, bounds, flags, 6, cbuf, slots, sizes)
    raw.free()
    rows = np.diff(bounds)
    ooffs = np.arange(n, dtype=np.int64) * chunk_bytes
    status = np.zeros(n, dtype=np.int32)
    cols = np.arange(NC)
    out = {}

    def decode():
        hip.dev_decompress_chunks(cbuf, slots, sizes, rows, NC, 2, flags, back, ooffs, status)
        assert not status.any()

    def stats(window):
        st, _, out[window] = hip.dev_window_stats(cbuf, slots, sizes, bounds[:-1], rows, NC, np.int16, flags, 0, n * RATE, window, cols,
                                                  out=out.get(window))
        assert st == [0] * n
    runs = {'decode': decode, 'stats_30000': lambda: stats(30000), 'stats_3001': lambda: stats(3001)}
    times = {k: [] for k in runs}
    for _ in range(warmup):
        for f in runs.values():
            f()
    for _ in range(reps):
        for k, f in runs.items():                                       # alternated
            hip.dev_sync(0)
            t0 = time.perf_counter()
            f()
            hip.dev_sync(0)
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    decoded = n * chunk_bytes
    res = {'workload': '60 s x 385 int16 (configs[1], %.2f GB decoded, %.2f GB compressed) in HBM; %d alternated runs after %d warm-ups, median'
                       % (decoded / 1e9, sizes.sum() / 1e9, reps, warmup),
           'decode_ms': round(med['decode'], 3)}
    for w in (30000, 3001):
        k = 'stats_%d' % w
        res[k + '_ms'] = round(med[k], 3)
        res[k + '_over_decode'] = round(med[k] / med['decode'], 4)
        res[k + '_raw_GBps'] = round(decoded / med[k] / 1e6, 1)
    res['decode_raw_GBps'] = round(decoded / med['decode'] / 1e6, 1)
    res['spread_ms'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    return res


def quo_stats(r, start, stop, window=RATE, chunks_per_slice=30):
    """The status quo: Reader slices of 30 chunks, numpy per window -- the same fields window_stats returns."""
    nw = -(-(stop - start) // window)
    mn = np.empty((nw, r.n_channels), r.dtype)
    mx = np.empty_like(mn)
    sm = np.empty((nw, r.n_channels), np.int64)
    sq = np.empty((nw, r.n_channels), np.float64)
    step = chunks_per_slice * window
    for a in range(start, stop, step):
        x = r[a:min(a + step, stop)]
        for b in range(0, x.shape[0], window):
            w = (a - start + b) // window
            seg = x[b:b + window]
            s64 = seg.astype(np.int64)
            mn[w], mx[w], sm[w], sq[w] = seg.min(0), seg.max(0), s64.sum(0), (s64 * s64).sum(0).astype(np.float64)
    return mn, mx, sm, sq


def file_part(seconds, quo_seconds):
    tmp = Path(tempfile.mkdtemp(prefix='mtsstats_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        raw_bytes = n_samples * NC * 2
        r.window_stats(RATE, 0, 2 * RATE)                               # warm-up (code objects, workspaces, pinned pieces)
        t_ws = []
        for _ in range(2):
            t0 = time.perf_counter()
            s = r.window_stats(RATE)
            t_ws.append(time.perf_counter() - t0)
        q = quo_seconds * RATE
        t0 = time.perf_counter()
        mn, mx, sm, sq = quo_stats(r, 0, q)
        t_quo = time.perf_counter() - t0
        nq = q // RATE
        same = bool(np.array_equal(mn, s.min[:nq]) and np.array_equal(mx, s.max[:nq]) and np.array_equal(sm, s.sum[:nq]) and
                    np.array_equal(sq, s.sumsq[:nq]))
        r.close()
        ws_rate = raw_bytes / min(t_ws) / 1e9
        quo_rate = q * NC * 2 / t_quo / 1e9
        return {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), windows of 30000 rows' % (seconds, raw_bytes / 1e9, cbytes / 1e9),
                'window_stats_s': [round(t, 3) for t in t_ws], 'window_stats_raw_GBps': round(ws_rate, 2),
                'status_quo': 'Reader slices of 30 chunks + numpy, first %d s of the file' % quo_seconds,
                'status_quo_s': round(t_quo, 3), 'status_quo_raw_GBps': round(quo_rate, 2),
                'speedup': round(ws_rate / quo_rate, 2), 'results_identical': same}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seconds', type=int, default=600)
    ap.add_argument('--quo-seconds', type=int, default=600)
    ap.add_argument('--device-only', action='store_true', help='the device comparison alone (for the rocprofv3 run)')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'window_stats_bench', 'device': device_part(a.reps, a.warmup)}
    if not a.device_only:
        line['file'] = file_part(a.seconds, min(a.quo_seconds, a.seconds))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
