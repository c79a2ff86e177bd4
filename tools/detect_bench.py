"""Peak detection on the device against what a user does today; prints one JSON line and writes it to --out.

  reader  the configs[1] recording (60 s x 385 int16 of the synthetic generator) as a .cbin on tmpfs, highpass_taps(300, 30000, 101),
          exclude 30, spread 5, sign 'neg', threshold 5 * mad / 0.6745 of the raw channels.  In one process, the runs alternated,
          medians of --reps runs:
            detect (median reference) cold and resident, detect (no reference) resident,
            Reader.decimate(1, taps=the same, edge='recording') resident on the same range: the part of the job the device could
            already do, with its 4 bytes per sample across the bus.
          The condition: resident detect without a reference is not slower than resident decimate(1).
          The host path on the first --host-seconds: decimate(1)'s rows, np.median per row, the vectorised restatement of the
          neighbourhood test (tests/detect_oracle.py); its event list is compared with the device's for equality.
  device  --device-only: mts_dev_detect on the recording's chunks in HBM, with and without the reference (for the run under
          `rocprofv3 --kernel-trace --stats`, which gives the kernel times)."""
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
EXCLUDE, SPREAD = 30, 5


def device_part(reps, warmup, seconds):
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
    cap = n * RATE * NC // 256
    state = {'out': None, 'n': {}}

    def det(reference):
        st, n_ev, _, state['out'] = hip.dev_detect(cbuf, slots, sizes, bounds[:-1], rows, NC, np.int16, flags, 0, n * RATE, 0, n * RATE, taps, cols,
                                                   60.0, 0, reference, EXCLUDE, SPREAD, cap, out=state['out'], download=False)
        assert st == [0] * n
        state['n'][reference] = n_ev
    runs = {'detect_median': lambda: det(1), 'detect_plain': lambda: det(0)}
    times = {k: [] for k in runs}
    for _ in range(warmup):
        for f in runs.values():
            f()
    for _ in range(reps):
        for k, f in runs.items():
            hip.dev_sync(0)
            t0 = time.perf_counter()
            f()
            hip.dev_sync(0)
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {'workload': '%d s x 385 int16 in HBM, mts_dev_detect, 101 taps, exclude %d, spread %d, threshold 60; %d runs after %d warm-ups, median'
                       % (n, EXCLUDE, SPREAD, reps, warmup)}
    for k, v in times.items():
        res[k + '_ms'] = round(float(np.median(v)), 3)
    res['events'] = {'median': state['n'].get(1), 'plain': state['n'].get(0)}
    return res


def reader_part(seconds, host_seconds, reps):
    from tests.detect_oracle import events_of
    tmp = Path(tempfile.mkdtemp(prefix='mtsdet_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, seconds, tmp, NC)
        cold_r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        cold_r._dev_cache_bytes = 0                                       # never resident: every call decodes
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        taps = api.highpass_taps(300, RATE, 101)
        t0 = time.perf_counter()
        thr = 5 * r.mad(center=0.0).mad[0] / 0.6745
        t_mad = time.perf_counter() - t0
        thr = np.maximum(thr, 1.0)
        kw = dict(taps=taps, exclude=EXCLUDE, spread=SPREAD)
        for k in range(r.n_chunks):                                      # every chunk into the device cache
            r[r.chunk_bounds[k]:r.chunk_bounds[k] + 1]
        resident = int(sum(int(p) >= NC for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks)))))
        keep = {}
        runs = {'detect_median_cold': lambda: keep.__setitem__('cold', cold_r.detect(thr, reference='median', **kw)),
                'detect_median_resident': lambda: keep.__setitem__('med', r.detect(thr, reference='median', **kw)),
                'detect_plain_resident': lambda: keep.__setitem__('plain', r.detect(thr, **kw)),
                'decimate1_resident': lambda: keep.__setitem__('rows', r.decimate(1, taps=taps, edge='recording').shape)}
        for f in runs.values():                                          # warm-up (code objects, workspaces)
            f()
        times = {k: [] for k in runs}
        for _ in range(reps):
            for k, f in runs.items():                                    # alternated
                t0 = time.perf_counter()
                f()
                times[k].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), highpass_taps(300, 30000, 101), exclude %d, '
                           'spread %d, sign neg, threshold 5 * mad / 0.6745 per channel; medians of %d alternated runs in one process'
                           % (seconds, n_samples * NC * 2 / 1e9, cbytes / 1e9, EXCLUDE, SPREAD, reps),
               'mad_s': round(t_mad, 3), 'resident_chunks': resident, 'n_chunks': r.n_chunks,
               'events_median': int(keep['med'].sample.size), 'events_plain': int(keep['plain'].sample.size),
               'cold_equals_resident': bool(all(keep['cold'][k].tobytes() == keep['med'][k].tobytes() for k in ('sample', 'channel', 'amplitude')))}
        for k, v in med.items():
            res[k + '_s'] = round(v, 4)
        res['spread_s'] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}
        res['condition_plain_resident_not_slower_than_decimate1'] = bool(med['detect_plain_resident'] <= med['decimate1_resident'])
        # the host path on the first host_seconds: the device's filtered rows, numpy's median, the restated neighbourhood test
        hs = min(host_seconds, seconds)
        if hs > 0:
            stop = hs * RATE
            t0 = time.perf_counter()
            y = r.decimate(1, 0, min(n_samples, stop + EXCLUDE), taps=taps, edge='recording')
            t_rows = time.perf_counter() - t0
            t0 = time.perf_counter()
            z = y - np.median(y, axis=1)[:, None]
            t_med = time.perf_counter() - t0
            t0 = time.perf_counter()
            want = events_of(z, 0, 0, stop, thr.astype(np.float32), 0, EXCLUDE, SPREAD)
            t_ev = time.perf_counter() - t0
            got = r.detect(thr, 0, stop, reference='median', **kw)
            res['host'] = {'seconds': hs, 'decimate1_s': round(t_rows, 3), 'np_median_s': round(t_med, 3), 'neighbourhood_s': round(t_ev, 3),
                           'events': int(want[0].size),
                           'equals_device': bool(got.sample.tobytes() == want[0].tobytes() and got.channel.tobytes() == want[1].tobytes()
                                                 and got.amplitude.tobytes() == want[2].tobytes())}
        r.close()
        cold_r.close()
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--host-seconds', type=int, default=60, help='rows of the host path (0: none)')
    ap.add_argument('--device-only', action='store_true', help='mts_dev_detect alone (for the rocprofv3 run)')
    ap.add_argument('--out', default=None, help='also write the line here (profiles/detect.json)')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'detect_bench'}
    if a.device_only:
        line['device'] = device_part(a.reps, a.warmup, a.seconds)
    else:
        line['reader'] = reader_part(a.seconds, a.host_seconds, a.reps)
    print(json.dumps(line))
    if a.out:
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
