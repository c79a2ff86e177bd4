"""Spike snippets on the device against what a user does today; prints one JSON line and writes it to --out.

  reader  the configs[1] recording (60 s x 385 int16 of the synthetic generator) as a .cbin on tmpfs.  The events are those of
          detect(5 * mad / 0.6745, taps=highpass_taps(300, 30000), reference='median', exclude=30, spread=5), mad the per-channel median
          of |z| over the first second of the filtered, referenced rows (the noise level of the band the events live in; the raw
          channels' mad is dominated by the slow drift and finds no event in this recording).  In one process, the runs alternated,
          medians of --reps runs:
            waveforms(neighbours=8, 20 before, 41 after, the same taps and reference) cold and resident, and resident without the
            snippets (the extrema alone).
          The host path on the first --host-seconds: Reader[:] across the bus, then the same filter, median and gather in numpy
          (tests/waveforms_oracle.py); its snippets are compared with the device's for equality.
          The gap sweep: a sparse list, resident, at MTS_WAVEFORMS_GAP_ROWS 1024, 4096, 16384 and -1 (never cut), with the slabs
          each setting gives.
  reader_dense  the same at --dense-sigma (3.5) instead of 5: the synthetic generator has no spikes, so the 5 sigma list is a few
          dozen noise peaks a minute; 3.5 sigma gives the event density of a real recording.  Its sparse list is every
          --sparse-th event.
  device  mts_dev_waveforms against mts_dev_detect on the recording's chunks in HBM: they share the filter and the median, so the
          difference is the yardstick for the gather kernel; and the gather kernels' own time (MTS_WAVEFORMS_TIME: events around each
          launch) with the bytes they write per second."""
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
BEFORE, AFTER, K = 20, 41, 8
GAPS = (1024, 4096, 16384, -1)


def _note(*what):
    print('waveforms_bench:', *what, file=sys.stderr, flush=True)


def _median_times(runs, reps):
    for k, f in runs.items():                                            # warm-up (code objects, workspaces)
        t0 = time.perf_counter()
        f()
        _note('warm-up', k, '%.3f s' % (time.perf_counter() - t0))
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():                                        # alternated
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    return {k: float(np.median(v)) for k, v in times.items()}, {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}


def spike_threshold(r, taps):
    """5 * mad / 0.6745 per channel, mad the median of |z| over the first second of the filtered, referenced rows."""
    z = r.decimate(1, 0, RATE, taps=taps, edge='recording')
    z = z - np.median(z, axis=1)[:, None]
    return np.maximum(5 * np.median(np.abs(z), axis=0) / 0.6745, 1.0).astype(np.float32)


def device_part(reps, warmup, seconds, thr):
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
    table = (cbuf, slots, sizes, bounds[:-1], rows, NC, np.int16, flags, 0, n * RATE)
    st, n_ev, ev, det_out = hip.dev_detect(*table, 0, n * RATE, taps, cols, thr, 0, 1, EXCLUDE, SPREAD, cap)
    assert st == [0] * n and n_ev <= cap
    _note('device: %d events' % n_ev)
    ev_row, ev_col0 = ev[0], ev[1].astype(np.int64) - K
    state = {'out': None}

    def wav(want_wave):
        st, _, state['out'] = hip.dev_waveforms(*table, taps, cols, 1, ev_row, ev_col0, BEFORE, AFTER, 2 * K + 1, want_wave, out=state['out'],
                                                download=False)
        assert st == [0] * n

    def det():
        st, got, _, _ = hip.dev_detect(*table, 0, n * RATE, taps, cols, thr, 0, 1, EXCLUDE, SPREAD, cap, out=det_out, download=False)
        assert st == [0] * n and got == n_ev
    runs = {'dev_waveforms': lambda: wav(True), 'dev_waveforms_extrema_only': lambda: wav(False), 'dev_detect': det}
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
    res = {'workload': '%d s x 385 int16 in HBM, 101 taps, median reference; the %d events of mts_dev_detect (the thresholds of the reader part, exclude %d, spread %d), '
                       'snippets of %d x %d; %d runs after %d warm-ups, median' % (n, n_ev, EXCLUDE, SPREAD, BEFORE + AFTER, 2 * K + 1, reps, warmup),
           'events': int(n_ev)}
    for k, v in times.items():
        res[k + '_ms'] = round(float(np.median(v)), 3)
    res['waveforms_minus_detect_ms'] = round(res['dev_waveforms_ms'] - res['dev_detect_ms'], 3)
    os.environ['MTS_WAVEFORMS_TIME'] = '1'
    try:
        gather = {}
        for name, want_wave in (('with_snippets', True), ('extrema_only', False)):
            us = []
            for _ in range(reps):
                wav(want_wave)
                plan = hip.waveforms_last_plan(0)
                us.append(plan['gather_us'])
            nbytes = int(n_ev) * (4 * (BEFORE + AFTER) * (2 * K + 1) * want_wave + 16)
            gather[name] = {'kernel_ms': round(float(np.median(us)) / 1e3, 3), 'bytes_written': nbytes,
                            'gb_written_per_s': round(nbytes / max(float(np.median(us)), 1.0) / 1e3, 2), 'slabs': plan['slabs']}
        res['gather'] = gather
    finally:
        os.environ.pop('MTS_WAVEFORMS_TIME', None)
    return res


def reader_part(tmp, r, thr, n_samples, cbytes, seconds, host_seconds, reps, sparse):
    from tests.waveforms_oracle import waveforms as host_waveforms
    if True:
        cold_r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        cold_r._dev_cache_bytes = 0                                       # never resident: every call decodes
        taps = api.highpass_taps(300, RATE, 101)
        for k in range(r.n_chunks):                                      # every chunk into the device cache
            r[r.chunk_bounds[k]:r.chunk_bounds[k] + 1]
        resident = int(sum(int(p) >= NC for p in hip.cache_query(r._cache_for(0), list(range(r.n_chunks)))))
        t0 = time.perf_counter()
        ev = r.detect(thr, taps=taps, reference='median', exclude=EXCLUDE, spread=SPREAD)
        t_detect = time.perf_counter() - t0
        _note('%d events, detect %.3f s' % (ev.sample.size, t_detect))
        kw = dict(before=BEFORE, after=AFTER, neighbours=K, taps=taps, reference='median')
        keep = {}
        runs = {'waveforms_cold': lambda: keep.__setitem__('cold', cold_r.waveforms(ev.sample, ev.channel, **kw)),
                'waveforms_resident': lambda: keep.__setitem__('res', r.waveforms(ev.sample, ev.channel, **kw)),
                'extrema_only_resident': lambda: keep.__setitem__('bare', r.waveforms(ev.sample, ev.channel, waveforms=False, **kw))}
        med, spread = _median_times(runs, reps)
        res = {'workload': '%d s x 385 int16 .cbin on tmpfs (%.2f GB raw, %.2f GB compressed), the %d events of detect(thresholds %.1f .. %.1f: sigma * mad / 0.6745 of the filtered first second, '
                           'highpass_taps(300, 30000, 101), median reference, exclude %d, spread %d), snippets of %d x %d; medians of %d '
                           'alternated runs in one process' % (seconds, n_samples * NC * 2 / 1e9, cbytes / 1e9, ev.sample.size, thr.min(), thr.max(), EXCLUDE, SPREAD,
                                                               BEFORE + AFTER, 2 * K + 1, reps),
               'events': int(ev.sample.size), 'resident_chunks': resident, 'n_chunks': r.n_chunks, 'detect_resident_s': round(t_detect, 4),
               'result_bytes': int(keep['res'].waveforms.nbytes),
               'cold_equals_resident': bool(keep['cold'].waveforms.tobytes() == keep['res'].waveforms.tobytes()),
               'centre_equals_amplitude': bool(keep['res'].waveforms[np.arange(ev.sample.size), BEFORE, K].tobytes() == ev.amplitude.tobytes()),
               'extrema_only_equal': bool(all(keep['bare'][w][k].tobytes() == keep['res'][w][k].tobytes()
                                              for w in ('trough', 'peak') for k in ('value', 'index')))}
        for k, v in med.items():
            res[k + '_s'] = round(v, 4)
        res['spread_s'] = spread
        # the host path on the first host_seconds: the rows across the bus, then filter, median and gather in numpy
        hs = min(host_seconds, seconds)
        if hs > 0:
            stop = hs * RATE
            pick = ev.sample < stop - AFTER - 50                         # (their support lies inside the rows read)
            t0 = time.perf_counter()
            x = r[:stop]
            t_rows = time.perf_counter() - t0
            t0 = time.perf_counter()
            want = host_waveforms(x, 0, 0, n_samples, taps, 1, ev.sample[pick], ev.channel[pick] - K, BEFORE, AFTER, 2 * K + 1)
            t_host = time.perf_counter() - t0
            t0 = time.perf_counter()
            got = r.waveforms(ev.sample[pick], ev.channel[pick], **kw)
            t_dev = time.perf_counter() - t0
            res['host'] = {'seconds': hs, 'events': int(pick.sum()), 'read_rows_s': round(t_rows, 3), 'numpy_filter_median_gather_s': round(t_host, 3),
                           'device_same_events_s': round(t_dev, 4), 'equals_device': bool(got.waveforms.tobytes() == want[0].tobytes())}
        # the gap sweep on a sparse list: every sparse-th event
        sel = np.arange(0, ev.sample.size, max(1, sparse))
        s_sample, s_channel = ev.sample[sel], ev.channel[sel]
        sweep_runs, slabs = {}, {}

        def at_gap(gap):
            os.environ['MTS_WAVEFORMS_GAP_ROWS'] = str(gap)
            keep['gap'] = r.waveforms(s_sample, s_channel, **kw)
            slabs[str(gap)] = hip.waveforms_last_plan(0)['slabs']
        for gap in GAPS:
            sweep_runs[str(gap)] = lambda gap=gap: at_gap(gap)
        try:
            g_med, g_spread = _median_times(sweep_runs, reps)
        finally:
            os.environ.pop('MTS_WAVEFORMS_GAP_ROWS', None)
        res['gap_sweep'] = {'events': int(sel.size), 'median_rows_between_events': float(np.median(np.diff(s_sample))) if sel.size > 1 else 0.0,
                            'resident_s': {k: round(v, 4) for k, v in g_med.items()}, 'spread_s': g_spread, 'slabs_of_the_last_call': slabs,
                            'best': min(g_med, key=g_med.get)}
        cold_r.close()
        return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--host-seconds', type=int, default=2, help='rows of the host path (0: none)')
    ap.add_argument('--sparse', type=int, default=200, help='the gap sweep of the dense list keeps every n-th event')
    ap.add_argument('--dense-sigma', type=float, default=3.5, help='the second event list: this many sigma instead of 5')
    ap.add_argument('--device-only', action='store_true', help='the device entries alone')
    ap.add_argument('--reader-only', action='store_true', help='the Reader alone')
    ap.add_argument('--out', default=None, help='also write the line here (profiles/waveforms.json)')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'waveforms_bench'}
    tmp = Path(tempfile.mkdtemp(prefix='mtswav_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        n_samples, cbytes = bench.build_synth_file(hip, 0, a.seconds, tmp, NC)
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        thr = spike_threshold(r, api.highpass_taps(300, RATE, 101))
        _note('thresholds %.1f .. %.1f' % (thr.min(), thr.max()))
        dense = (thr * (a.dense_sigma / 5.0)).astype(np.float32)
        if not a.device_only:
            line['reader'] = reader_part(tmp, r, thr, n_samples, cbytes, a.seconds, a.host_seconds, a.reps, 1)
            line['reader_dense'] = dict(sigma=a.dense_sigma, **reader_part(tmp, r, dense, n_samples, cbytes, a.seconds, a.host_seconds, a.reps, a.sparse))
        r.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if not a.reader_only:
        hip.release()
        line['device'] = dict(sigma=a.dense_sigma, **device_part(a.reps, a.warmup, a.seconds, dense))
    print(json.dumps(line))
    if a.out:
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
