"""Template peeling on the device against what a user does today; prints one JSON line (and writes it to --out).

  device  the configs[1] recording in HBM (60 s x 385 int16 of the synthetic generator, compressed on the device):
          mts_dev_match_residual against mts_dev_match_templates on the same chunks, in the same run -- the difference is the
          subtraction's cost -- with 101 high-pass taps, the median reference and templates of 61 rows x 385 columns, 8 and 128 of
          them, threshold[k] = 4 standard deviations of the first 2 s of column k of the scores, exclude = 60.  The subtracted list is
          the first pass's own events with their least-squares amplitudes; the second pass's event count is recorded beside the
          first's.  In one process, the runs alternated, after warm-ups.
  reader  the same recording as a .cbin on tmpfs: Reader.residual of the first --host-seconds cold (nothing resident) and resident
          (every chunk in the device cache) against the host doing the same in the same run: Reader[:] of the rows and the filter's
          halo, the numpy filter, the median and the subtraction loop (tests/residual_oracle.residual) -- the bytes compared for
          equality.

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--device-only keeps that run short); --kernel-stats
merges that run's kernel_stats.csv into the line: k_subtract beside k_row_median, which reads and writes the same slabs."""
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
from tests.residual_oracle import residual  # noqa: E402

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
    thr, sub = {}, {}
    for k in CASES:                                                     # the first 2 s of the scores, from their first three chunks
        st, y, o = hip.dev_correlate(cbuf, slots[:3], sizes[:3], bounds[:3], rows[:3], NC, np.int16, flags, 0, n * RATE, 0, 2 * RATE, TAPS, cols, 1,
                                     BEFORE, tpls[k])
        assert st == [0] * 3
        thr[k] = _threshold(y)
        o.free()
        # the first pass's own events, with their fitted amplitudes: the list that the second pass subtracts
        st, n_ev, (row, tpl, val), o = hip.dev_match_templates(*table, 0, n * RATE, 0, n * RATE, TAPS, cols, 1, BEFORE, tpls[k], thr[k], EXCLUDE, 1 << 20)
        assert st == [0] * n and n_ev == row.size
        o.free()
        sub[k] = (row, tpl, api.template_amplitudes(val, tpl, tpls[k]))

    def tm(k):
        st, found['m', k], _, out['m', k] = hip.dev_match_templates(*table, 0, n * RATE, 0, n * RATE, TAPS, cols, 1, BEFORE, tpls[k], thr[k], EXCLUDE,
                                                                    1 << 20, out=out.get(('m', k)), download=False)
        assert st == [0] * n

    def mr(k):
        st, found['r', k], _, out['r', k] = hip.dev_match_residual(*table, 0, n * RATE, 0, n * RATE, TAPS, cols, 1, BEFORE, tpls[k], thr[k], EXCLUDE,
                                                                   1 << 20, *sub[k], out=out.get(('r', k)), download=False)
        assert st == [0] * n
    runs = {}
    for k in CASES:
        runs['match_templates_k%d' % k] = lambda k=k: tm(k)
        runs['match_residual_k%d' % k] = lambda k=k: mr(k)
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
                       'T = %d, threshold %.0f sigma of the first 2 s, exclude %d, the first pass\'s events subtracted; %d alternated runs after '
                       '%d warm-ups, median' % (n * chunk_bytes / 1e9, sizes.sum() / 1e9, T, SIGMAS, EXCLUDE, reps, warmup)}
    for k in CASES:
        m, r = 'match_templates_k%d' % k, 'match_residual_k%d' % k
        res[m + '_ms'] = round(med[m], 3)
        res[r + '_ms'] = round(med[r], 3)
        res[r + '_minus_match_templates_ms'] = round(med[r] - med[m], 3)
        res[m + '_events'] = int(found['m', k])
        res[r + '_subtracted_events'] = int(sub[k][0].size)
        res[r + '_second_pass_events'] = int(found['r', k])
    res['spread_ms'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    return res


def reader_part(seconds, host_seconds):
    tmp = Path(tempfile.mkdtemp(prefix='mtsres_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        kw = dict(before=BEFORE, taps=TAPS, reference='median')
        k = CASES[0]
        tpl = _templates(k)
        hs = min(host_seconds, seconds) * RATE
        half = (TAPS.size - 1) // 2
        thr = _threshold(r.correlate(tpl, 0, min(2, seconds) * RATE, **kw))
        ev = r.match_templates(tpl, thr, exclude=EXCLUDE, **kw)
        sub = (ev.sample, ev.template, api.template_amplitudes(ev.score, ev.template, tpl))
        r.residual(*sub, tpl, 0, min(RATE, hs), **kw)                    # warm-up (code objects, workspaces)
        t_cold = []
        for _ in range(2):
            t0 = time.perf_counter()
            cold = r.residual(*sub, tpl, 0, hs, **kw)
            t_cold.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        whole = r.residual(*sub, tpl, **kw)
        t_whole = time.perf_counter() - t0
        same_whole = bool(whole[:hs].tobytes() == cold.tobytes())
        del whole
        # what a user does today: the rows and the filter's halo across the bus, then numpy
        t0 = time.perf_counter()
        hi = min(n_samples, hs + half)
        x = r[0:hi]
        t_read = time.perf_counter() - t0
        near = sub[0] < hs + T
        host = residual(x, 0, 0, n_samples, 0, hs, TAPS, 1, BEFORE, tpl, *(v[near] for v in sub))
        t_host = time.perf_counter() - t0
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), 385 columns, 101 taps, median reference, %d '
                           'templates of T = %d, the %d events of the first pass subtracted' % (seconds, n_samples * NC * 2 / 1e9, cbytes / 1e9, k, T,
                                                                                                int(ev.sample.size)),
               'first_%ds_cold_s' % host_seconds: [round(t, 4) for t in t_cold],
               'first_%ds_host_s' % host_seconds: round(t_host, 3), 'first_%ds_host_read_alone_s' % host_seconds: round(t_read, 4),
               'first_%ds_equals_host' % host_seconds: bool(host.tobytes() == cold.tobytes()),
               'whole_file_cold_s': round(t_whole, 3), 'whole_file_result_bytes': int(4 * n_samples * NC), 'whole_equals_first': same_whole}
        del x, host
        second = r.match_templates(tpl, thr, exclude=EXCLUDE, subtract=sub, **kw)
        res['first_pass_events'], res['second_pass_events'] = int(ev.sample.size), int(second.sample.size)
        for c in range(r.n_chunks):                                      # every chunk into the device cache
            r[r.chunk_bounds[c]:r.chunk_bounds[c] + 1]
        res['resident_chunks'] = int(sum(int(p) >= NC for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks)))))
        res['n_chunks'] = r.n_chunks
        t_warm = []
        for _ in range(2):
            t0 = time.perf_counter()
            warm = r.residual(*sub, tpl, 0, hs, **kw)
            t_warm.append(time.perf_counter() - t0)
        res['first_%ds_resident_s' % host_seconds] = [round(t, 4) for t in t_warm]
        res['cold_equals_resident'] = bool(warm.tobytes() == cold.tobytes())
        r.close()
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def kernel_stats(path):
    """The kernels of the device part out of a rocprofv3 kernel_stats.csv: calls, average and total milliseconds."""
    keep = ('k_subtract', 'k_row_median', 'k_correlate', 'k_decimate', 'k_tmatch_best', 'k_tmatch_mask', 'k_tmatch_emit')
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
    line = {'tool': 'residual_bench', 'device': device_part(a.reps, a.warmup)}
    if not a.device_only:
        line['reader'] = reader_part(a.seconds, a.host_seconds)
    if a.kernel_stats:
        line['kernel_trace'] = {'how': a.kernel_stats_how, 'kernels': kernel_stats(a.kernel_stats)}
    print(json.dumps(line))
    if a.out:
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
