"""The covariance of the filtered rows on the device against what a user does today and against the existing kernels; prints one JSON
line and, with --out, writes it.

  reader  the configs[1] recording (60 s x 385 int16 of the synthetic generator) as a .cbin on tmpfs, highpass_taps(300, 30000, 101) and
          the median reference: Reader.cov(taps=, reference=) with window=None and window=30000, cold (nothing resident) and with every
          chunk resident, 3 alternated runs each with identical bytes asserted, the medians; against residual([], ...) for the whole
          file (2.77 GB of float32 across the bus) + float64 z.T @ z on the host, held to the bound of tests/gram_oracle.py.
  device  mts_dev_filtered_gram (window=None and 30000) against mts_dev_detect and mts_dev_gram on the same chunks in HBM, in one
          process, the runs alternated, after warm-ups.
  pair    (--pair-seconds S) the first S seconds: z from mts_dev_residual, compressed on the device as a float32 recording, and
          mts_dev_gram of it -- k_gram<float> + k_gram_colsum on the rows that k_zgram reads --, identical bytes asserted.

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


def _synth_chunks(n):
    """n seconds of the synthetic recording compressed in HBM -> the chunk table of the device entries."""
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
    return (cbuf, slots, sizes, bounds[:-1], np.diff(bounds), NC, np.int16, flags)


def _timed(runs, reps, warmup):
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
    res = {k + '_ms': round(float(np.median(v)), 3) for k, v in times.items()}
    res['spread_ms'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
    return res


def device_part(reps, warmup, seconds):
    n = seconds
    chunks = _synth_chunks(n)
    taps = api.highpass_taps(300, RATE, 101)
    cols = np.arange(NC)
    N = n * RATE
    out = {}

    def detect():
        st, _, _, out['det'] = hip.dev_detect(*chunks, 0, N, 0, N, taps, cols, 60.0, 0, 1, 0, 0, N * NC // 256, out=out.get('det'), download=False)
        assert st == [0] * n

    def gram(window):
        key = ('gram', window)
        st, _, _, out[key] = hip.dev_gram(*chunks, 0, N, window, 0, hip.gram_groups(0, N, window), cols, out=out.get(key), download=False)
        assert st == [0] * n

    def zgram(window, reference=1):
        key = ('zgram', window)
        st, _, _, out[key] = hip.dev_filtered_gram(*chunks, 0, N, taps, cols, reference, 0, N, window, 0, hip.gram_groups(0, N, window),
                                                   out=out.get(key), download=False)
        assert st == [0] * n
    runs = {'detect_median': detect, 'gram_whole': lambda: gram(N), 'gram_30000': lambda: gram(RATE), 'filtered_gram_whole': lambda: zgram(N),
            'filtered_gram_30000': lambda: zgram(RATE), 'filtered_gram_whole_plain': lambda: zgram(N, 0)}
    res = {'workload': '%d s x 385 int16 in HBM, 101 taps; detect: median reference, threshold 60, no exclusion; Gram matrices of one '
                       'window over everything and of windows of 30000 rows; %d alternated runs after %d warm-ups, median' % (n, reps, warmup)}
    res.update(_timed(runs, reps, warmup))
    res['filtered_gram_over_detect'] = round(res['filtered_gram_whole_ms'] / res['detect_median_ms'], 3)
    res['fp64_mfma_gflop'] = round(2.0 * N * (7 * 8 // 2) * 64 * 64 / 1e9, 1)   # 28 pairs of 64 x 64 tiles, 2 flop a product
    for b in out.values():
        b.free()
    chunks[0].free()
    return res


def pair_part(reps, warmup, seconds):
    """k_zgram beside k_gram<float> + k_gram_colsum on a float32 recording that holds the same rows."""
    n = seconds
    chunks = _synth_chunks(n)
    taps = api.highpass_taps(300, RATE, 101)
    cols = np.arange(NC)
    N = n * RATE
    st, _, zbuf = hip.dev_residual(*chunks, 0, N, 0, N, taps, cols, 1, 0, np.zeros((1, 1, NC), np.float32), [], [], [], download=False)
    assert st == [0] * n
    chunk_bytes = RATE * NC * 4
    cb = (hip.compress_bound(chunk_bytes) + 255) // 256 * 256
    zc = hip.DevBuffer(n * cb)
    bounds = np.arange(n + 1, dtype=np.int64) * RATE
    slots, sizes = np.arange(n, dtype=np.int64) * cb, np.zeros(n, dtype=np.int64)
    zflags = hip.make_flags(False, False, 'F')
    hip.dev_compress_chunks(zbuf, NC, 4, bounds, zflags, 1, zc, slots, sizes)
    zbuf.free()
    zchunks = (zc, slots, sizes, bounds[:-1], np.diff(bounds), NC, np.float32, zflags)
    ng = hip.gram_groups(0, N, N)
    st, G, S, o1 = hip.dev_filtered_gram(*chunks, 0, N, taps, cols, 1, 0, N, N, 0, ng)
    st2, Gz, Sz, o2 = hip.dev_gram(*zchunks, 0, N, N, 0, ng, cols)
    assert st == [0] * n and st2 == [0] * n
    same = bool(G.tobytes() == Gz.tobytes() and S.tobytes() == Sz.tobytes())
    assert same
    runs = {'filtered_gram_of_int16': lambda: hip.dev_filtered_gram(*chunks, 0, N, taps, cols, 1, 0, N, N, 0, ng, out=o1, download=False),
            'gram_of_float32_z': lambda: hip.dev_gram(*zchunks, 0, N, N, 0, ng, cols, out=o2, download=False)}
    res = {'workload': '%d s x 385: mts_dev_filtered_gram of the int16 chunks and mts_dev_gram of a float32 recording in HBM that holds '
                       'their z (both inflate their chunks; the second filters nothing)' % n, 'identical_bytes': same}
    res.update(_timed(runs, reps, warmup))
    for b in (o1, o2, zc, chunks[0]):
        b.free()
    return res


def reader_part(seconds):
    sys.path.insert(0, str(ROOT))
    from tests.gram_oracle import gram_bound, tree_height
    tmp = Path(tempfile.mkdtemp(prefix='mtsfgram_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    os.environ['MTSCOMP_DEVICE_CACHE_GB'] = '8'
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        taps = api.highpass_taps(300, RATE, 101)
        kw = dict(taps=taps, reference='median')
        calls = {'cov_whole': lambda r: r.cov(**kw), 'cov_30000': lambda r: r.cov(window=RATE, **kw)}

        def timed_runs(r):
            t, first = {k: [] for k in calls}, {}
            for _ in range(RUNS):
                for k, f in calls.items():
                    t0 = time.perf_counter()
                    got = f(r)
                    t[k].append(time.perf_counter() - t0)
                    ref = first.setdefault(k, got)
                    assert ref.gram.tobytes() == got.gram.tobytes() and ref.sum.tobytes() == got.sum.tobytes(), k
            return {k: round(float(np.median(v)), 3) for k, v in t.items()}, first
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        r.cov(0, 2 * RATE, **kw)                                            # warm-up (code objects, workspaces, pinned pieces)
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), highpass_taps(300, 30000, 101), median '
                           'reference; medians of %d alternated runs' % (seconds, n_samples * NC * 2 / 1e9, cbytes / 1e9, RUNS)}
        res['cold_s'], cold = timed_runs(r)
        # what a user does today: residual([], ...) for the whole file + float64 z.T @ z on the host
        k0 = np.zeros((1, 1, NC), np.float32)
        t0 = time.perf_counter()
        zf = r.residual([], [], [], k0, before=0, **kw)
        t_res = time.perf_counter() - t0
        t0 = time.perf_counter()
        via, absg = np.zeros((NC, NC)), np.zeros((NC, NC))
        for a in range(0, len(zf), 1 << 18):                                # (blocks: the float64 copy of the whole z is 5.5 GB)
            zd = zf[a:a + (1 << 18)].astype(np.float64)
            via += zd.T @ zd
        t_mm = time.perf_counter() - t0
        for a in range(0, len(zf), 1 << 18):
            zd = np.abs(zf[a:a + (1 << 18)].astype(np.float64))
            absg += zd.T @ zd
        h = tree_height(len(zf))
        within = bool((np.abs(cold['cov_whole'].gram[0] - via) <= gram_bound(h, absg, len(zf)) + gram_bound(len(zf), absg)).all())
        res['residual_path'] = {'residual_s': round(t_res, 3), 'matmul_s': round(t_mm, 3), 'total_s': round(t_res + t_mm, 3),
                                'bytes_across_the_bus': int(zf.nbytes), 'within_bound': within}
        assert within
        del zf
        for k in range(r.n_chunks):                                      # every chunk resident in the device cache
            r[r.chunk_bounds[k] + 1:r.chunk_bounds[k] + 3]
        resident = sum(int(p) > 0 for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks))))
        res['chunks_resident'] = '%d of %d' % (resident, r.n_chunks)
        res['resident_s'], warm = timed_runs(r)
        r.close()
        res['results_identical'] = all(cold[k].gram.tobytes() == warm[k].gram.tobytes() and cold[k].sum.tobytes() == warm[k].sum.tobytes()
                                       for k in calls)
        assert res['results_identical']
        res['speedup_over_residual_path'] = round(res['residual_path']['total_s'] / res['cold_s']['cov_whole'], 2)
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--pair-seconds', type=int, default=0, help='also compare with mts_dev_gram of a float32 recording holding z of this many seconds')
    ap.add_argument('--device-only', action='store_true', help='the device comparisons alone (for the rocprofv3 run)')
    ap.add_argument('--out', help='also write the JSON line to this file')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'filtered_gram_bench', 'device': device_part(a.reps, a.warmup, a.seconds)}
    if a.pair_seconds:
        line['pair'] = pair_part(a.reps, a.warmup, a.pair_seconds)
    if not a.device_only:
        line['reader'] = reader_part(a.seconds)
    text = json.dumps(line)
    print(text)
    if a.out:
        Path(a.out).write_text(text + '\n')


if __name__ == '__main__':
    main()
