"""Template events on the device against what a user does today; prints one JSON line (and writes it to --out).

  device  the configs[1] recording in HBM (60 s x 385 int16 of the synthetic generator, compressed on the device):
          mts_dev_match_templates against mts_dev_correlate on the same chunks -- the decode-to-result times to compare -- with 101
          high-pass taps, the median reference and templates of 61 rows x 385 columns, 8 and 128 of them, threshold[k] = 4 standard
          deviations of the first 2 s of column k of the scores, exclude = 60; in one process, the runs alternated, after warm-ups.
  reader  the same recording as a .cbin on tmpfs: Reader.match_templates cold (nothing resident) and resident (every chunk in the
          device cache) for both K with the event counts, and on the first --host-seconds alone against the host path in the same
          run: Reader.correlate over the rows and their neighbours, then the numpy peak pick of the definition
          (tests/tmatch_oracle.events_of_scores) -- the events compared for equality.

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--device-only keeps that run short); --kernel-stats
merges that run's kernel_stats.csv into the line."""
import argparse
import csv
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
from mtscomp_amd import api, hip  # noqa: E402
from tests.tmatch_oracle import events_of_scores  # noqa: E402

RATE, NC, T, BEFORE, EXCLUDE, SIGMAS = 30000, 385, 61, 20, 60, 4.0
CASES = [8, 128]
TAPS = api.highpass_taps(300, RATE, 101)


def _templates(k):
    return (np.random.RandomState(k).randn(k, T, NC) / np.sqrt(T * NC)).astype(np.float32)


def _threshold(score):
    return (SIGMAS * score.astype(np.float64).std(axis=0)).astype(np.float32)


def device_part(reps, warmup):
    n = 60
    chunk_bytes = RATE * NC * 2
    raw = hip.DevBuffer(n * chunk_bytes)
    hip.dev_synth_int16(raw, 0, 0, n * RATE, NC, 0)
    cb = (hip.compress_bound(chunk_bytes) + 255) // 256 * 256
    cbuf = hip.DevBuffer(n * cb)
    bounds = np.arange(n + 1, dtype=np.int64) * RATE
    slots = np.arange(n, dtype=np.int64) * cb
    sizes = np.zeros(n, dtype=np.int64)
    flags = hip.make_flags(True, False, 'F')
    hip.dev_compress_chunks(raw, NC, 2, bounds, flags, 6, cbuf, slots, sizes)
    raw.free()
    rows = np.diff(bounds)
    cols = np.arange(NC)
    table = (cbuf, slots, sizes, bounds[:-1], rows, NC, np.int16, flags)
    out, found = {}, {}
    tpls = {k: _templates(k) for k in CASES}                            # (made once: the timed closures hold device calls alone)
    thr = {}
    for k in CASES:                                                     # the first 2 s of the scores, from their first three chunks
        st, y, o = hip.dev_correlate(cbuf, slots[:3], sizes[:3], bounds[:3], rows[:3], NC, np.int16, flags, 0, n * RATE, 0, 2 * RATE, TAPS, cols, 1,
                                     BEFORE, tpls[k])
        assert st == [0] * 3
        thr[k] = _threshold(y)
        o.free()

    def cor(k):
        st, _, out['c', k] = hip.dev_correlate(*table, 0, n * RATE, 0, n * RATE, TAPS, cols, 1, BEFORE, tpls[k], out=out.get(('c', k)), download=False)
        assert st == [0] * n

    def tm(k):
        st, found[k], _, out['m', k] = hip.dev_match_templates(*table, 0, n * RATE, 0, n * RATE, TAPS, cols, 1, BEFORE, tpls[k], thr[k], EXCLUDE,
                                                               1 << 20, out=out.get(('m', k)), download=False)
        assert st == [0] * n
    runs = {}
    for k in CASES:
        runs['correlate_k%d' % k] = lambda k=k: cor(k)
        runs['match_templates_k%d' % k] = lambda k=k: tm(k)
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
    res = {'workload': '60 s x 385 int16 (configs[1], %.2f GB decoded, %.2f GB compressed) in HBM, 385 columns, 101 taps, median reference, '
                       'T = %d, threshold %.0f sigma of the first 2 s, exclude %d; %d alternated runs after %d warm-ups, median'
                       % (n * chunk_bytes / 1e9, sizes.sum() / 1e9, T, SIGMAS, EXCLUDE, reps, warmup)}
    for k in CASES:
        c, m = 'correlate_k%d' % k, 'match_templates_k%d' % k
        res[c + '_ms'] = round(med[c], 3)
        res[m + '_ms'] = round(med[m], 3)
        res[m + '_minus_correlate_ms'] = round(med[m] - med[c], 3)
        res[m + '_events'] = int(found[k])
        res[m + '_event_bytes'] = 16 * int(found[k])
        res[c + '_result_bytes'] = 4 * n * RATE * k
    res['spread_ms'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    return res


def reader_part(seconds, host_seconds):
    tmp = Path(tempfile.mkdtemp(prefix='mtstm_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        kw = dict(before=BEFORE, taps=TAPS, reference='median')
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), 385 columns, 101 taps, median reference, T = %d, '
                           'threshold %.0f sigma of the first 2 s, exclude %d' % (seconds, n_samples * NC * 2 / 1e9, cbytes / 1e9, T, SIGMAS, EXCLUDE),
               'cases': {}}
        hs = min(host_seconds, seconds) * RATE
        evs, thr = {}, {}
        for k in CASES:
            tpl = _templates(k)
            thr[k] = _threshold(r.correlate(tpl, 0, min(2, seconds) * RATE, **kw))
            r.match_templates(tpl, thr[k], 0, RATE, exclude=EXCLUDE, **kw)        # warm-up (code objects, workspaces)
            t_cold = []
            for _ in range(2):
                t0 = time.perf_counter()
                evs[k] = r.match_templates(tpl, thr[k], exclude=EXCLUDE, **kw)
                t_cold.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            first = r.match_templates(tpl, thr[k], 0, hs, exclude=EXCLUDE, **kw)
            t_dev = time.perf_counter() - t0
            # what a user does today: the scores of the rows and their neighbours across the bus, then the peak pick on the host
            t0 = time.perf_counter()
            score = r.correlate(tpl, 0, min(n_samples, hs + EXCLUDE), **kw)
            t_cor = time.perf_counter() - t0
            row, which, val = events_of_scores(score, 0, 0, hs, thr[k], EXCLUDE)
            t_host = time.perf_counter() - t0
            same = (first.sample.tobytes(), first.template.tobytes(), first.score.tobytes()) == (row.tobytes(), which.tobytes(), val.tobytes())
            res['cases']['k%d' % k] = {'events': int(evs[k].sample.size), 'cold_s': [round(t, 3) for t in t_cold],
                                       'first_%ds_events' % host_seconds: int(first.sample.size),
                                       'first_%ds_s' % host_seconds: round(t_dev, 4),
                                       'first_%ds_correlate_then_numpy_s' % host_seconds: round(t_host, 4),
                                       'first_%ds_correlate_alone_s' % host_seconds: round(t_cor, 4),
                                       'first_%ds_events_equal_numpy' % host_seconds: bool(same)}
            del score
        for c in range(r.n_chunks):                                      # every chunk into the device cache
            r[r.chunk_bounds[c]:r.chunk_bounds[c] + 1]
        res['resident_chunks'] = int(sum(int(p) >= NC for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks)))))
        res['n_chunks'] = r.n_chunks
        for k in CASES:
            tpl = _templates(k)
            t_warm, t_cor = [], []
            for _ in range(2):
                t0 = time.perf_counter()
                ev = r.match_templates(tpl, thr[k], exclude=EXCLUDE, **kw)
                t_warm.append(time.perf_counter() - t0)
            for _ in range(2):
                t0 = time.perf_counter()
                y = r.correlate(tpl, **kw)
                t_cor.append(time.perf_counter() - t0)
                del y
            c = res['cases']['k%d' % k]
            c['resident_s'] = [round(t, 3) for t in t_warm]
            c['correlate_resident_s'] = [round(t, 3) for t in t_cor]
            c['cold_equals_resident'] = bool((ev.sample.tobytes(), ev.template.tobytes(), ev.score.tobytes()) ==
                                             (evs[k].sample.tobytes(), evs[k].template.tobytes(), evs[k].score.tobytes()))
        r.close()
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def kernel_stats(path):
    """The kernels of the device part out of a rocprofv3 kernel_stats.csv: calls, average and total milliseconds."""
    keep = ('k_tmatch_best', 'k_tmatch_mask', 'k_tmatch_emit', 'k_detect_count', 'k_detect_scan', 'k_correlate', 'k_decimate', 'k_row_median')
    res = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row['Name'].split('(')[0].replace('void ', '').replace('mts::', '')
            if name.split('<')[0] in keep:
                res[name] = {'calls': int(row['Calls']), 'avg_ms': round(float(row['AverageNs']) / 1e6, 4),
                             'total_ms': round(float(row['TotalDurationNs']) / 1e6, 3)}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--host-seconds', type=int, default=2)
    ap.add_argument('--device-only', action='store_true', help='the device comparison alone (for the rocprofv3 run)')
    ap.add_argument('--kernel-stats', help='a kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --device-only, merged into the line')
    ap.add_argument('--kernel-stats-how', default='', help='how that run was made (recorded beside its numbers)')
    ap.add_argument('--out', help='also write the line to this file')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'match_templates_bench', 'device': device_part(a.reps, a.warmup)}
    if not a.device_only:
        line['reader'] = reader_part(a.seconds, a.host_seconds)
    if a.kernel_stats:
        line['kernel_trace'] = {'how': a.kernel_stats_how, 'kernels': kernel_stats(a.kernel_stats)}
    print(json.dumps(line))
    if a.out:
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
