"""Channel-mixing matrix products on the device against what a user does today; prints one JSON line (and writes it to --out).

  device  the configs[1] recording in HBM (60 s x 385 int16 of the synthetic generator, compressed on the device):
          mts_dev_project with a full 385-column matrix to n_out = 8 and 385 outputs, float32 and float64, against
          mts_dev_decompress_chunks of the same chunks, in one process, the runs alternated, after warm-ups.  Both inflate every
          chunk; the difference is the product.  The operations (2 * rows * n_cols * n_out) are counted from the shapes.
  reader  the same recording as a .cbin on tmpfs: Reader.project cold (nothing resident) and resident (every chunk in the device
          cache) for the same four cases, against Reader[:] followed by numpy.matmul on the host in the same run.

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
CASES = [(8, 'float32'), (385, 'float32'), (8, 'float64'), (385, 'float64')]


def _weights(n_out):
    return np.random.RandomState(n_out).randn(NC, n_out) / np.sqrt(NC)


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
    off = np.linspace(-5, 5, NC)
    out = {}

    def decode():
        hip.dev_decompress_chunks(cbuf, slots, sizes, rows, NC, 2, flags, back, ooffs, status)
        assert not status.any()

    def proj(n_out, dt):
        st, _, out[n_out, dt] = hip.dev_project(cbuf, slots, sizes, bounds[:-1], rows, NC, np.int16, flags, 0, n * RATE, cols, off, _weights(n_out),
                                                dt, out=out.get((n_out, dt)), download=False)
        assert st == [0] * n
    runs = {'decode': decode}
    for n_out, dt in CASES:
        runs['n%d_%s' % (n_out, dt)] = lambda n_out=n_out, dt=dt: proj(n_out, dt)
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
    res = {'workload': '60 s x 385 int16 (configs[1], %.2f GB decoded, %.2f GB compressed) in HBM, 385 columns with an offset; '
                       '%d alternated runs after %d warm-ups, median' % (decoded / 1e9, sizes.sum() / 1e9, reps, warmup),
           'decode_ms': round(med['decode'], 3)}
    for n_out, dt in CASES:
        k = 'n%d_%s' % (n_out, dt)
        res['project_%s_ms' % k] = round(med[k], 3)
        res['project_%s_over_decode' % k] = round(med[k] / med['decode'], 4)
        res['project_%s_gflop' % k] = round(2.0 * n * RATE * NC * n_out / 1e9, 2)       # counted from the shapes, not measured
    res['spread_ms'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    return res


def reader_part(seconds):
    tmp = Path(tempfile.mkdtemp(prefix='mtsprj_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        off = np.linspace(-5, 5, NC)
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), 385 columns with an offset'
                           % (seconds, n_samples * NC * 2 / 1e9, cbytes / 1e9), 'cases': {}}
        ys = {}
        for n_out, dt in CASES:
            w = _weights(n_out)
            r.project(w, 0, 2 * RATE, offset=off, dtype=dt)              # warm-up (code objects, workspaces)
            t_cold = []
            for _ in range(2):
                t0 = time.perf_counter()
                ys[n_out, dt] = r.project(w, offset=off, dtype=dt)
                t_cold.append(time.perf_counter() - t0)
            res['cases']['n%d_%s' % (n_out, dt)] = {'cold_s': [round(t, 3) for t in t_cold]}
        for k in range(r.n_chunks):                                      # every chunk into the device cache
            r[r.chunk_bounds[k]:r.chunk_bounds[k] + 1]
        res['resident_chunks'] = int(sum(int(p) >= NC for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks)))))
        res['n_chunks'] = r.n_chunks
        for n_out, dt in CASES:
            w = _weights(n_out)
            t_warm = []
            for _ in range(2):
                t0 = time.perf_counter()
                y2 = r.project(w, offset=off, dtype=dt)
                t_warm.append(time.perf_counter() - t0)
            c = res['cases']['n%d_%s' % (n_out, dt)]
            c['resident_s'] = [round(t, 3) for t in t_warm]
            c['cold_equals_resident'] = bool(y2.tobytes() == ys[n_out, dt].tobytes())
        # the host path in the same run: read everything, then numpy
        t0 = time.perf_counter()
        x = r[:]
        t_read = time.perf_counter() - t0
        res['host_read_s'] = round(t_read, 3)
        for n_out, dt in CASES:
            w = _weights(n_out).astype(dt)
            t0 = time.perf_counter()
            yh = np.matmul(x.astype(dt) - off.astype(dt), w)
            t_mm = time.perf_counter() - t0
            c = res['cases']['n%d_%s' % (n_out, dt)]
            c['host_matmul_s'] = round(t_mm, 3)
            c['speedup_vs_read_plus_matmul'] = round((t_read + t_mm) / min(c['cold_s']), 1)
            c['max_abs_diff_vs_host'] = float(np.abs(yh - ys[n_out, dt]).max())
            c['max_abs_host'] = float(np.abs(yh).max())
            del yh
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
    ap.add_argument('--out', help='also write the line to this file')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'project_bench', 'device': device_part(a.reps, a.warmup)}
    if not a.device_only:
        line['reader'] = reader_part(a.seconds)
    print(json.dumps(line))
    if a.out:
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
