"""Template scores on the device against what a user does today; prints one JSON line (and writes it to --out).

  device  the configs[1] recording in HBM (60 s x 385 int16 of the synthetic generator, compressed on the device): mts_dev_correlate
          with 101 high-pass taps, the median reference and templates of 61 rows x 385 columns, 8 and 128 of them, against
          mts_dev_detect on the same chunks (the two share the decode, the filter and the median; the thresholds are out of reach, so
          detect's own kernels emit nothing) and mts_dev_project to 385 float32 outputs (k_project<short, float>, the yardstick of
          the matrix kernel), in one process, the runs alternated, after warm-ups.  The operations (2 * rows * n_cols * T * K, and
          2 * rows * n_cols * n_out) are counted from the shapes.
  reader  the same recording as a .cbin on tmpfs: Reader.correlate cold (nothing resident) and resident (every chunk in the device
          cache) for both K, and on the first --host-seconds alone against the host path in the same run, before any chunk is made
          resident: Reader[...], the same filter, np.median and a float32 matmul over shifted views (compared within 1e-5 of the largest score: the host's BLAS
          order is not the definition's).

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

RATE, NC, T, BEFORE = 30000, 385, 61, 20
CASES = [8, 128]
TAPS = api.highpass_taps(300, RATE, 101)


def _templates(k):
    return (np.random.RandomState(k).randn(k, T, NC) / np.sqrt(T * NC)).astype(np.float32)


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
    out = {}

    def detect():
        st, n_ev, _, out['det'] = hip.dev_detect(*table, 0, n * RATE, 0, n * RATE, TAPS, cols, 1e30, 0, 1, 30, 5, 4096, out=out.get('det'),
                                                 download=False)
        assert st == [0] * n and n_ev == 0

    w = np.random.RandomState(385).randn(NC, 385) / np.sqrt(NC)
    tpls = {k: _templates(k) for k in CASES}                            # (made once: the timed closures hold device calls alone)

    def project():
        st, _, out['prj'] = hip.dev_project(*table, 0, n * RATE, cols, None, w, np.float32, out=out.get('prj'), download=False)
        assert st == [0] * n

    def cor(k):
        st, _, out[k] = hip.dev_correlate(*table, 0, n * RATE, 0, n * RATE, TAPS, cols, 1, BEFORE, tpls[k], out=out.get(k), download=False)
        assert st == [0] * n
    runs = {'detect': detect, 'project_n385_float32': project}
    for k in CASES:
        runs['correlate_k%d' % k] = lambda k=k: cor(k)
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
                       'T = %d; %d alternated runs after %d warm-ups, median' % (n * chunk_bytes / 1e9, sizes.sum() / 1e9, T, reps, warmup),
           'detect_ms': round(med['detect'], 3), 'project_n385_float32_ms': round(med['project_n385_float32'], 3),
           'project_n385_float32_gflop': round(2.0 * n * RATE * NC * 385 / 1e9, 2)}
    for k in CASES:
        name = 'correlate_k%d' % k
        res[name + '_ms'] = round(med[name], 3)
        res[name + '_minus_detect_ms'] = round(med[name] - med['detect'], 3)
        res[name + '_gflop'] = round(2.0 * n * RATE * NC * T * k / 1e9, 2)             # counted from the shapes, not measured
    res['spread_ms'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    return res


def _host_scores(x, i0, i1, k):
    """The host path for rows [i0, i1) of the recording x (rows from 0): float32 filter, median, matmul over shifted views."""
    half = (TAPS.size - 1) // 2
    a, b = i0 - BEFORE, i1 - BEFORE + T - 1
    lo, hi = max(a, 0), min(b, x.shape[0])
    xf = np.zeros((hi - lo + TAPS.size - 1, x.shape[1]), np.float32)
    s0, s1 = max(0, lo + half - (TAPS.size - 1)), min(x.shape[0], hi + half)
    xf[s0 - (lo + half - (TAPS.size - 1)):s1 - (lo + half - (TAPS.size - 1))] = x[s0:s1]
    y = np.zeros((hi - lo, x.shape[1]), np.float32)
    for j, t in enumerate(TAPS.astype(np.float32)):
        y += t * xf[TAPS.size - 1 - j:TAPS.size - 1 - j + hi - lo]
    y -= np.median(y, axis=1)[:, None]
    z = np.zeros((b - a, x.shape[1]), np.float32)
    z[lo - a:hi - a] = y
    s = np.zeros((i1 - i0, k.shape[0]), np.float32)
    for tau in range(T):
        s += z[tau:tau + i1 - i0] @ k[:, tau, :].T
    return s


def reader_part(seconds, host_seconds):
    tmp = Path(tempfile.mkdtemp(prefix='mtscor_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        kw = dict(before=BEFORE, taps=TAPS, reference='median')
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), 385 columns, 101 taps, median reference, T = %d'
                           % (seconds, n_samples * NC * 2 / 1e9, cbytes / 1e9, T), 'cases': {}}
        ys = {}
        hs = min(host_seconds, seconds) * RATE
        for k in CASES:
            tpl = _templates(k)
            r.correlate(tpl, 0, RATE, **kw)                              # warm-up (code objects, workspaces)
            t_cold = []
            for _ in range(2):
                t0 = time.perf_counter()
                ys[k] = r.correlate(tpl, **kw)
                t_cold.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            r.correlate(tpl, 0, hs, **kw)
            res['cases']['k%d' % k] = {'cold_s': [round(t, 3) for t in t_cold], 'cold_first_%ds_s' % host_seconds: round(time.perf_counter() - t0, 3)}
        # the host path in the same run, on the first host_seconds: read the rows and their halo (nothing made resident yet: a cold
        # user's read), filter, median, matmul
        for k in CASES:
            tpl = _templates(k)
            t0 = time.perf_counter()
            x = r[:min(n_samples, hs + T + TAPS.size)]
            yh = _host_scores(x, 0, hs, tpl)
            t_host = time.perf_counter() - t0
            c = res['cases']['k%d' % k]
            c['host_first_%ds_s' % host_seconds] = round(t_host, 3)
            c['speedup_vs_host_first_%ds' % host_seconds] = round(t_host / c['cold_first_%ds_s' % host_seconds], 1)
            c['max_abs_diff_vs_host'] = float(np.abs(yh - ys[k][:hs]).max())
            c['max_abs_host'] = float(np.abs(yh).max())
            c['within_1e-5_of_host'] = bool(c['max_abs_diff_vs_host'] <= 1e-5 * c['max_abs_host'])
            del yh
        for c in range(r.n_chunks):                                      # every chunk into the device cache
            r[r.chunk_bounds[c]:r.chunk_bounds[c] + 1]
        res['resident_chunks'] = int(sum(int(p) >= NC for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks)))))
        res['n_chunks'] = r.n_chunks
        for k in CASES:
            tpl = _templates(k)
            t_warm = []
            for _ in range(2):
                t0 = time.perf_counter()
                y2 = r.correlate(tpl, **kw)
                t_warm.append(time.perf_counter() - t0)
            c = res['cases']['k%d' % k]
            c['resident_s'] = [round(t, 3) for t in t_warm]
            c['cold_equals_resident'] = bool(y2.tobytes() == ys[k].tobytes())
            del y2
        r.close()
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
    ap.add_argument('--out', help='also write the line to this file')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'correlate_bench', 'device': device_part(a.reps, a.warmup)}
    if not a.device_only:
        line['reader'] = reader_part(a.seconds, a.host_seconds)
    print(json.dumps(line))
    if a.out:
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
