"""Welch power spectral density on the device against what a user does today; prints one JSON line.

  device  the configs[1] recording in HBM (60 s x 385 int16 of the synthetic generator, compressed on the device):
          mts_dev_welch at nperseg 256, 1024 and 4096 (noverlap nperseg / 2, hann, constant detrend), float32 and float64, against
          mts_dev_decompress_chunks of the same chunks, in one process, the runs alternated, after warm-ups.  Both inflate every
          chunk; the difference is the spectra.
  reader  the same recording as a .cbin on tmpfs: Reader.welch(1024) cold (nothing resident) and resident (every chunk in the
          device cache), against scipy.signal.welch(Reader[:], fs, nperseg=1024, axis=0) on the host (when scipy is there).

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

    def welch(nperseg, cdt):
        taper = api.welch_window('hann', nperseg)
        n_seg = (n * RATE - nperseg) // (nperseg // 2) + 1
        key = (nperseg, cdt)
        st, _, out[key] = hip.dev_welch(cbuf, slots, sizes, bounds[:-1], rows, NC, np.int16, flags, 0, 0, n_seg, nperseg, nperseg // 2, taper,
                                        True, cdt, cols, out=out.get(key), download=False)
        assert st == [0] * n
    runs = {'decode': decode}
    for nperseg in (256, 1024, 4096):
        for cdt in ('float32', 'float64'):
            runs['n%d_%s' % (nperseg, cdt)] = (lambda p=nperseg, c=cdt: welch(p, c))
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
    res = {'workload': '60 s x 385 int16 (configs[1], %.2f GB decoded, %.2f GB compressed) in HBM, noverlap nperseg / 2, hann, '
                       'constant detrend; %d alternated runs after %d warm-ups, median' % (decoded / 1e9, sizes.sum() / 1e9, reps, warmup),
           'decode_ms': round(med['decode'], 3)}
    for k in runs:
        if k != 'decode':
            res['welch_%s_ms' % k] = round(med[k], 3)
            res['welch_%s_over_decode' % k] = round(med[k] / med['decode'], 4)
    res['spread_ms'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    return res


def reader_part(seconds):
    tmp = Path(tempfile.mkdtemp(prefix='mtswelch_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        r.welch(1024, 0, 2 * RATE)                                       # warm-up (code objects, workspaces)
        t_cold = []
        for _ in range(2):
            t0 = time.perf_counter()
            _, y = r.welch(1024)
            t_cold.append(time.perf_counter() - t0)
        for k in range(r.n_chunks):                                      # every chunk into the device cache
            r[r.chunk_bounds[k]:r.chunk_bounds[k] + 1]
        resident = int(sum(int(p) >= NC for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks)))))
        t_warm = []
        for _ in range(2):
            t0 = time.perf_counter()
            _, y2 = r.welch(1024)
            t_warm.append(time.perf_counter() - t0)
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), nperseg 1024, noverlap 512, hann, float32'
                           % (seconds, n_samples * NC * 2 / 1e9, cbytes / 1e9),
               'cold_s': [round(t, 3) for t in t_cold], 'resident_s': [round(t, 3) for t in t_warm],
               'resident_chunks': resident, 'n_chunks': r.n_chunks, 'cold_equals_resident': bool(y.tobytes() == y2.tobytes())}
        try:
            from scipy import signal
        except ImportError:
            signal = None
        if signal is not None:
            t0 = time.perf_counter()
            x = r[:]
            t_read = time.perf_counter() - t0
            t0 = time.perf_counter()
            _, ys = signal.welch(x, fs=r.sample_rate, nperseg=1024, axis=0)
            t_sp = time.perf_counter() - t0
            res.update({'scipy_read_s': round(t_read, 3), 'scipy_welch_s': round(t_sp, 3),
                        'speedup_vs_read_plus_scipy': round((t_read + t_sp) / min(t_cold), 1),
                        'max_rel_diff_vs_scipy': float((np.abs(ys - y) / np.maximum(np.abs(ys), 1e-300)).max())})
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
    line = {'tool': 'welch_bench', 'device': device_part(a.reps, a.warmup)}
    if not a.device_only:
        line['reader'] = reader_part(a.seconds)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
