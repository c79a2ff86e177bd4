"""Order statistics of the filtered rows on the device against what a user does today; prints one JSON line and, with --out, writes it.

  reader  the configs[1] recording (60 s x 385 int16 of the synthetic generator) as a .cbin on tmpfs, highpass_taps(300, 30000, 101) and
          the median reference: Reader.mad(center=0.0) and Reader.mad() over the whole range and with window=30000, cold (nothing
          resident) and with every chunk resident, 3 alternated runs each with identical results asserted, the medians; against
            - the host path on the first --host-seconds s: Reader[:], numpy FIR, row median, np.median, equal values asserted;
            - residual([], ...) + np.median for the whole file (2.77 GB of float32 across the bus).
  device  one round of mts_dev_filtered_rank_hist (mode 0 and mode 2, windows of 30000 rows) against mts_dev_detect and
          mts_dev_rank_hist on the same chunks in HBM, in one process, the runs alternated, after warm-ups.

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
from mtscomp_amd import api, hip  # noqa: E402

RATE, NC = 30000, 385
RUNS = 3


def device_part(reps, warmup, seconds, sweep=()):
    n = seconds
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
    taps = api.highpass_taps(300, RATE, 101)
    cols = np.arange(NC)
    N = n * RATE
    out = {}
    chunks = (cbuf, slots, sizes, bounds[:-1], rows, NC, np.int16, flags)

    def selectors(dtype, mode):
        pref = np.zeros((n, hip.RANK_SELECTORS, NC), np.uint64)
        shift = np.full((n, hip.RANK_SELECTORS, NC), -1, np.int32)
        shift[:, 0] = hip.rank_key_bits(dtype, mode) - hip.RANK_BITS          # the first, prefix-free round: one selector, every item
        return (mode, 0.0 if mode else None, pref, shift)

    def detect():
        st, _, _, out['det'] = hip.dev_detect(*chunks, 0, N, 0, N, taps, cols, 60.0, 0, 1, 0, 0, N * NC // 256, out=out.get('det'), download=False)
        assert st == [0] * n

    def rank(mode):
        key = ('rank', mode)
        st, _, out[key] = hip.dev_rank_hist(*chunks, 0, N, RATE, cols, *selectors(np.int16, mode), out=out.get(key), fetch=False)
        assert st == [0] * n

    def zrank(mode, reference=1, block_rows=None):
        key = ('zrank', mode)
        if block_rows:                                                  # (read by every call)
            os.environ['MTS_ZRANK_BLOCK_ROWS'] = str(block_rows)
        st, _, out[key] = hip.dev_filtered_rank_hist(*chunks, 0, N, taps, cols, reference, 0, N, RATE, 0, N, *selectors(np.float32, mode),
                                                     out=out.get(key), fetch=False)
        os.environ.pop('MTS_ZRANK_BLOCK_ROWS', None)
        assert st == [0] * n
    runs = {'detect_median': detect, 'rank_30000': lambda: rank(0), 'rank_30000_abs': lambda: rank(2), 'filtered_rank_30000': lambda: zrank(0),
            'filtered_rank_30000_abs': lambda: zrank(2), 'filtered_rank_30000_plain': lambda: zrank(0, 0)}
    for h in sweep:                                                     # the rows of a workgroup, beside the default
        runs['filtered_rank_30000_block_rows_%d' % h] = lambda h=h: zrank(0, 1, h)
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
    res = {'workload': '%d s x 385 int16 in HBM, 101 taps; detect: median reference, threshold 60, no exclusion; one prefix-free round of '
                       'the select on windows of 30000 rows; %d alternated runs after %d warm-ups, median' % (n, reps, warmup)}
    for k, v in times.items():
        res[k + '_ms'] = round(float(np.median(v)), 3)
    res['spread_ms'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    res['filtered_rank_over_detect'] = round(res['filtered_rank_30000_ms'] / res['detect_median_ms'], 3)
    return res


def host_noise(x, n, taps):
    """median(|z|) of the file rows [0, n) on the host, x holding the rows [0, n + half) (fewer at the end of the recording): the
    float32 FIR in the kernel's order with zeros outside the recording, the row median, np.median."""
    tf = np.asarray(taps, np.float64).astype(np.float32)
    L = len(tf)
    half = (L - 1) // 2
    pad = np.zeros((n + L - 1, x.shape[1]), np.float32)                  # file row r at pad[r + L - 1 - half]
    pad[L - 1 - half:L - 1 - half + len(x)] = x
    acc = np.zeros((n, x.shape[1]), np.float32)
    for j in range(L):
        acc = acc + tf[j] * pad[L - 1 - j:L - 1 - j + n]
    s = np.sort(acc, axis=1)
    nc = x.shape[1]
    m = s[:, (nc - 1) // 2] if nc % 2 else np.float32(0.5) * (s[:, nc // 2 - 1] + s[:, nc // 2])
    z = acc - m[:, None]
    return np.median(np.abs(z.astype(np.float64)), axis=0)


def reader_part(seconds, host_seconds):
    tmp = Path(tempfile.mkdtemp(prefix='mtsfquant_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    os.environ['MTSCOMP_DEVICE_CACHE_GB'] = '8'
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        taps = api.highpass_taps(300, RATE, 101)
        kw = dict(taps=taps, reference='median')
        calls = {'mad_center0': lambda r: r.mad(center=0.0, **kw), 'mad': lambda r: r.mad(**kw),
                 'mad_center0_30000': lambda r: r.mad(center=0.0, window=RATE, **kw), 'mad_30000': lambda r: r.mad(window=RATE, **kw)}

        def timed_runs(r):
            """RUNS alternated runs of every call -> (median seconds, the first results, rounds); identical results asserted."""
            t, first = {k: [] for k in calls}, {}
            for _ in range(RUNS):
                for k, f in calls.items():
                    t0 = time.perf_counter()
                    got = f(r)
                    t[k].append(time.perf_counter() - t0)
                    assert first.setdefault(k, got).mad.tobytes() == got.mad.tobytes(), k
            return {k: round(float(np.median(v)), 3) for k, v in t.items()}, first, {k: int(v.rounds) for k, v in first.items()}
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        r.mad(0, 2 * RATE, center=0.0, **kw)                                # warm-up (code objects, workspaces, pinned pieces)
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), highpass_taps(300, 30000, 101), median '
                           'reference; medians of %d alternated runs' % (seconds, n_samples * NC * 2 / 1e9, cbytes / 1e9, RUNS)}
        res['cold_s'], cold, res['rounds'] = timed_runs(r)
        # the host path on the first host_seconds s (with the rows beyond them that the filter reads)
        hs = min(host_seconds, seconds)
        t0 = time.perf_counter()
        x = r[:hs * RATE + (len(taps) - 1) // 2]
        t_read = time.perf_counter() - t0
        t0 = time.perf_counter()
        want = host_noise(x, hs * RATE, taps)
        t_host = time.perf_counter() - t0
        got = r.mad(0, hs * RATE, center=0.0, **kw)
        res['host_path'] = {'seconds_of_recording': hs, 'read_s': round(t_read, 3), 'fir_median_sort_s': round(t_host, 3),
                            'total_s': round(t_read + t_host, 3), 'equal_values': bool(np.array_equal(got.mad[0], want))}
        assert res['host_path']['equal_values']
        t0 = time.perf_counter()
        res['host_path']['device_same_rows_s'] = (r.mad(0, hs * RATE, center=0.0, **kw), round(time.perf_counter() - t0, 3))[1]
        # residual([], ...) for the whole file + np.median on the host
        k0 = np.zeros((1, 1, NC), np.float32)
        t0 = time.perf_counter()
        zf = r.residual([], [], [], k0, before=0, **kw)
        t_res = time.perf_counter() - t0
        t0 = time.perf_counter()
        via = np.concatenate([np.median(np.abs(zf[:, c:c + 55]).astype(np.float64), axis=0) for c in range(0, NC, 55)])
        t_med = time.perf_counter() - t0
        res['residual_path'] = {'residual_s': round(t_res, 3), 'np_median_s': round(t_med, 3), 'total_s': round(t_res + t_med, 3),
                                'bytes_across_the_bus': int(zf.nbytes), 'equal_values': bool(np.array_equal(via, cold['mad_center0'].mad[0]))}
        assert res['residual_path']['equal_values']
        del zf
        for k in range(r.n_chunks):                                      # every chunk resident in the device cache
            r[r.chunk_bounds[k] + 1:r.chunk_bounds[k] + 3]
        resident = sum(int(p) > 0 for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks))))
        res['chunks_resident'] = '%d of %d' % (resident, r.n_chunks)
        res['resident_s'], warm, _ = timed_runs(r)
        r.close()
        res['results_identical'] = all(cold[k].mad.tobytes() == warm[k].mad.tobytes() for k in calls)
        assert res['results_identical']
        res['speedup_over_residual_path'] = round(res['residual_path']['total_s'] / res['cold_s']['mad_center0'], 2)
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--host-seconds', type=int, default=2)
    ap.add_argument('--device-only', action='store_true', help='the device comparison alone (for the rocprofv3 run)')
    ap.add_argument('--block-rows', type=int, nargs='*', default=[], help='also time the filtered round with these rows per workgroup')
    ap.add_argument('--out', help='also write the JSON line to this file')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'filtered_quantile_bench', 'device': device_part(a.reps, a.warmup, a.seconds, a.block_rows)}
    if not a.device_only:
        line['reader'] = reader_part(a.seconds, a.host_seconds)
    text = json.dumps(line)
    print(text)
    if a.out:
        Path(a.out).write_text(text + '\n')


if __name__ == '__main__':
    main()
