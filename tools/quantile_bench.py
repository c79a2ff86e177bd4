"""Order statistics on the device against what a user does today; prints one JSON line.

  device  the configs[1] recording in HBM (60 s x 385 int16 of the synthetic generator, compressed on the device; --const: every
          item the same value instead, the worst case for counter contention): one round of mts_dev_rank_hist -- mode 0 with
          windows of 30000 rows and one window over the range, mode 2 (float64 keys) with windows of 30000 -- against
          mts_dev_window_stats and mts_dev_decompress_chunks of the same chunks, in one process, the runs alternated, after
          warm-ups.  All of them inflate every chunk; the difference is the kernel behind it.
  file    a `--seconds` s .cbin on tmpfs: Reader.mad(window=30000) and Reader.median(), cold (nothing resident) and with every chunk
          resident in the device cache, against the status quo -- Reader[:] and np.median on the host.  The results must be
          identical.  The rounds (passes over the chunks: the decodes a cold scan pays) are reported per call.

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--device-only keeps that run short), counters from
a run of their own."""
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


def device_part(reps, warmup, const):
    n = 60
    chunk_bytes = RATE * NC * 2
    raw = hip.DevBuffer(n * chunk_bytes)
    if const:
        raw.upload(np.full(n * RATE * NC, 1234, np.int16))
    else:
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

    def rank(window, mode):
        nw = -(-n * RATE // window)
        pref = np.zeros((nw, hip.RANK_SELECTORS, NC), np.uint64)
        shift = np.full((nw, hip.RANK_SELECTORS, NC), -1, np.int32)
        shift[:, 0] = hip.rank_key_bits(np.int16, mode) - hip.RANK_BITS          # the first, prefix-free round: one selector, every item
        key = ('rank', window, mode)
        st, _, out[key] = hip.dev_rank_hist(cbuf, slots, sizes, bounds[:-1], rows, NC, np.int16, flags, 0, n * RATE, window, cols, mode,
                                            0.0 if mode else None, pref, shift, out=out.get(key), fetch=False)
        assert st == [0] * n
    runs = {'decode': decode, 'stats_30000': lambda: stats(30000), 'rank_30000': lambda: rank(30000, 0),
            'rank_one_window': lambda: rank(n * RATE, 0), 'rank_30000_abs': lambda: rank(30000, 2)}
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
    res = {'workload': '60 s x 385 int16 (%s, %.2f GB decoded, %.2f GB compressed) in HBM; %d alternated runs after %d warm-ups, median'
                       % ('every item 1234' if const else 'configs[1]', decoded / 1e9, sizes.sum() / 1e9, reps, warmup),
           'decode_ms': round(med['decode'], 3)}
    for k in runs:
        if k != 'decode':
            res[k + '_ms'] = round(med[k], 3)
            res[k + '_over_decode'] = round(med[k] / med['decode'], 4)
    res['spread_ms'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    return res


def file_part(seconds):
    tmp = Path(tempfile.mkdtemp(prefix='mtsquant_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    os.environ['MTSCOMP_DEVICE_CACHE_GB'] = '8'
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        raw_bytes = n_samples * NC * 2

        def timed(r, fn):
            t0 = time.perf_counter()
            v = fn()
            return v, round(time.perf_counter() - t0, 3)
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        r.median(0, 2 * RATE)                                            # warm-up (code objects, workspaces, pinned pieces)
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed)' % (seconds, raw_bytes / 1e9, cbytes / 1e9)}
        mad, res['mad_30000_cold_s'] = timed(r, lambda: r.mad(window=RATE))
        med, res['median_cold_s'] = timed(r, lambda: r.median())
        mad1, res['mad_one_window_cold_s'] = timed(r, lambda: r.mad())
        res['mad_30000_rounds'], res['mad_one_window_rounds'] = mad.rounds, mad1.rounds
        res['median_rounds'] = r.quantile(0.5, method='midpoint').rounds        # (what median() is; not timed)
        res['median_30000_rounds'] = r.quantile(0.5, window=RATE, method='midpoint').rounds
        r.close()
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        t0 = time.perf_counter()
        x = r[:]
        t_read = time.perf_counter() - t0
        t0 = time.perf_counter()
        q_med = np.concatenate([np.median(x[:, c:c + 55].astype(np.float64), axis=0) for c in range(0, NC, 55)])[None]
        t_med = time.perf_counter() - t0
        t0 = time.perf_counter()
        q_mad = np.empty((seconds, NC))
        for w in range(seconds):
            xf = x[w * RATE:(w + 1) * RATE].astype(np.float64)
            q_mad[w] = np.median(np.abs(xf - np.median(xf, axis=0)), axis=0)
        t_mad = time.perf_counter() - t0
        res['status_quo'] = 'Reader[:] (%.3f s) + np.median on the host' % t_read
        res['status_quo_median_s'] = round(t_read + t_med, 3)
        res['status_quo_mad_30000_s'] = round(t_read + t_mad, 3)
        for k in range(r.n_chunks):                                      # every chunk resident in the device cache
            r[r.chunk_bounds[k] + 1:r.chunk_bounds[k] + 3]
        resident = sum(int(p) > 0 for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks))))
        res['chunks_resident'] = '%d of %d' % (resident, r.n_chunks)
        mad_w, res['mad_30000_resident_s'] = timed(r, lambda: r.mad(window=RATE))
        med_w, res['median_resident_s'] = timed(r, lambda: r.median())
        r.close()
        res['results_identical'] = bool(np.array_equal(med, q_med) and np.array_equal(mad.mad, q_mad) and np.array_equal(med_w, q_med) and
                                        np.array_equal(mad_w.mad, q_mad) and mad1.mad.shape == (1, NC))
        res['speedup_mad_30000_cold'] = round(res['status_quo_mad_30000_s'] / res['mad_30000_cold_s'], 2)
        res['speedup_median_cold'] = round(res['status_quo_median_s'] / res['median_cold_s'], 2)
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--device-only', action='store_true', help='the device comparison alone (for the rocprofv3 runs)')
    ap.add_argument('--const', action='store_true', help='the device comparison on a recording whose items are all the same value')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'quantile_bench', 'device': device_part(a.reps, a.warmup, a.const)}
    if not a.device_only:
        line['file'] = file_part(a.seconds)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
