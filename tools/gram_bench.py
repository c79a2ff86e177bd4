"""Channel covariance on the device against what a user does today; prints one JSON line.

  device  the configs[1] recording in HBM (60 s x 385 int16 of the synthetic generator, compressed on the device): mts_dev_gram with
          385 and 64 columns, window None and 30000, against mts_dev_decompress_chunks of the same chunks, in one process, the runs
          alternated, after warm-ups.  Both inflate every chunk; the difference is the Gram matrices.
  reader  the same recording as a .cbin on tmpfs: Reader.cov() cold (nothing resident) and resident (every chunk in the device cache),
          against Reader[:] plus the exact host Gram (float64 BLAS over blocks of 2^20 rows, as tests/gram_oracle.py) and np.cov.

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


def host_gram(x):
    """x.astype(int64).T @ x.astype(int64) by float64 BLAS over blocks of 2^20 rows (exact for int16)."""
    out = np.zeros((x.shape[1], x.shape[1]), np.int64)
    for r in range(0, x.shape[0], 1 << 20):
        b = x[r:r + (1 << 20)].astype(np.float64)
        out += (b.T @ b).astype(np.int64)
    return out


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
    total = n * RATE
    out = {}

    def decode():
        hip.dev_decompress_chunks(cbuf, slots, sizes, rows, NC, 2, flags, back, ooffs, status)
        assert not status.any()

    def gram(nc, window):
        key = (nc, window)
        w = window or total
        st, _, _, out[key] = hip.dev_gram(cbuf, slots, sizes, bounds[:-1], rows, NC, np.int16, flags, 0, total, w, 0,
                                          hip.gram_groups(0, total, w), np.arange(nc), out=out.get(key), download=False)
        assert st == [0] * n
    runs = {'decode': decode}
    for nc in (385, 64):
        for window in (None, 30000):
            runs['c%d_w%s' % (nc, window or 'all')] = (lambda c=nc, w=window: gram(c, w))
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
    res = {'workload': '60 s x 385 int16 (configs[1], %.2f GB decoded, %.2f GB compressed) in HBM; %d alternated runs after %d warm-ups, '
                       'median' % (decoded / 1e9, sizes.sum() / 1e9, reps, warmup),
           'decode_ms': round(med['decode'], 3)}
    for k in runs:
        if k != 'decode':
            res['gram_%s_ms' % k] = round(med[k], 3)
            res['gram_%s_over_decode' % k] = round(med[k] / med['decode'], 4)
    res['spread_ms'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    return res


def reader_part(seconds):
    tmp = Path(tempfile.mkdtemp(prefix='mtsgram_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        r.cov(0, 2 * RATE)                                               # warm-up (code objects, workspaces)
        t_cold = []
        for _ in range(2):
            t0 = time.perf_counter()
            c = r.cov()
            t_cold.append(time.perf_counter() - t0)
        for k in range(r.n_chunks):                                      # every chunk into the device cache
            r[r.chunk_bounds[k]:r.chunk_bounds[k] + 1]
        resident = int(sum(int(p) >= NC for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks)))))
        t_warm = []
        for _ in range(2):
            t0 = time.perf_counter()
            c2 = r.cov()
            t_warm.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        x = r[:]
        t_read = time.perf_counter() - t0
        t0 = time.perf_counter()
        g = host_gram(x)
        t_gram = time.perf_counter() - t0
        t0 = time.perf_counter()
        cv = np.cov(x, rowvar=False)
        t_npcov = time.perf_counter() - t0
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), Reader.cov(), every column'
                           % (seconds, n_samples * NC * 2 / 1e9, cbytes / 1e9),
               'cold_s': [round(t, 3) for t in t_cold], 'resident_s': [round(t, 3) for t in t_warm],
               'resident_chunks': resident, 'n_chunks': r.n_chunks,
               'cold_equals_resident': bool(c.gram.tobytes() == c2.gram.tobytes()),
               'host_read_s': round(t_read, 3), 'host_blas_gram_s': round(t_gram, 3), 'host_np_cov_s': round(t_npcov, 3),
               'speedup_vs_read_plus_blas_gram': round((t_read + t_gram) / min(t_cold), 1),
               'gram_equals_host_int64': bool(np.array_equal(c.gram[0], g)),
               'max_abs_diff_vs_np_cov': float(np.abs(c.cov[0] - cv).max())}
        r.close()
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--device-only', action='store_true', help='the device comparison alone (for the rocprofv3 run)')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'gram_bench', 'device': device_part(a.reps, a.warmup)}
    if not a.device_only:
        line['reader'] = reader_part(a.seconds)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
