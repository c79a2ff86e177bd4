"""Spike positions and channel amplitudes on the device against what a user does today; prints one JSON line and writes it to --out.

  reader  the 60 s x 385 int16 recording of the synthetic generator as a .cbin on tmpfs.  The events are those of
          detect(3.5 * mad / 0.6745, taps=highpass_taps(300, 30000, 101), reference='median', exclude=30, spread=5) (the thresholds of
          tools/waveforms_bench.py at its dense setting), the snippets 20 before and 41 after, 17 wide (neighbours=8) and full width,
          the positions a two-column staggered grid (probe_positions below), the amplitude peak to peak.  In one process, the runs
          alternated, medians of --reps runs: localize cold and resident (their bytes are compared for equality), and the path users
          have today: waveforms(...) resident, then nanmax - nanmin and the weighted mean in numpy (compared with the device's
          amplitudes for equality and with its locations to float32 accuracy).  At full width the host path holds every snippet in
          memory (8.6 GB for 92 000 events), so it runs on the first --host-full-events events and the device path is timed on those
          and on all.
  device  mts_dev_localize against mts_dev_waveforms without its snippets (the extrema-only call reads the same entries of z and is
          the gather's floor) on the recording's chunks in HBM: they share the filter and the median, so the difference is the
          gather; and the gather kernels' own time (MTS_WAVEFORMS_TIME: events around each launch)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
import mtscomp_amd  # noqa: E402
from mtscomp_amd import api, hip  # noqa: E402
from tools.waveforms_bench import AFTER, BEFORE, EXCLUDE, K, NC, RATE, SPREAD, _median_times, spike_threshold  # noqa: E402

T = BEFORE + AFTER
MODE = 'ptp'


def probe_positions(n):
    """A two-column staggered grid in micrometres: x alternates between 11 and 43, y rises by 20 every second channel."""
    k = np.arange(n)
    return np.stack([np.where(k % 2, 43.0, 11.0), 20.0 * (k // 2)], axis=1).astype(np.float32)


def _note(*what):
    print('localize_bench:', *what, file=sys.stderr, flush=True)


def host_localize(w, col0, pos):
    """What a user computes from Reader.waveforms' snippets: peak-to-peak amplitudes and their weighted mean position, in numpy."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                   # (all-NaN columns: positions outside the selection)
        amp = np.nanmax(w, axis=1) - np.nanmin(w, axis=1)
    g = np.where(amp > 0, amp, np.float32(0.0))
    c = np.clip(col0[:, None] + np.arange(w.shape[2])[None, :], 0, pos.shape[0] - 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return amp, (g[:, :, None] * pos[c]).sum(axis=1) / g.sum(axis=1)[:, None]


def reader_part(tmp, r, thr, reps, host_full_events):
    cold_r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
    cold_r._dev_cache_bytes = 0                                           # never resident: every call decodes
    taps = api.highpass_taps(300, RATE, 101)
    for k in range(r.n_chunks):                                          # every chunk into the device cache
        r[r.chunk_bounds[k]:r.chunk_bounds[k] + 1]
    ev = r.detect(thr, taps=taps, reference='median', exclude=EXCLUDE, spread=SPREAD)
    _note('%d events' % ev.sample.size)
    pos = probe_positions(NC)
    res = {'events': int(ev.sample.size), 'amplitude': MODE}
    for width, neighbours, n_host in (('17', K, ev.sample.size), ('full', None, min(host_full_events, ev.sample.size))):
        kw = dict(before=BEFORE, after=AFTER, neighbours=neighbours, taps=taps, reference='median')
        keep = {}
        s, c = ev.sample[:n_host], ev.channel[:n_host]

        def host():
            got = r.waveforms(s, c, **kw)
            keep['host_wave_bytes'] = int(got.waveforms.nbytes)
            keep['host'] = host_localize(got.waveforms, got.position, pos)
        runs = {'localize_cold': lambda: keep.__setitem__('cold', cold_r.localize(ev.sample, pos, ev.channel, amplitude=MODE, **kw)),
                'localize_resident': lambda: keep.__setitem__('res', r.localize(ev.sample, pos, ev.channel, amplitude=MODE, **kw)),
                'waveforms_resident_plus_host_numpy': host}
        if n_host < ev.sample.size:
            runs['localize_resident_host_events'] = lambda: keep.__setitem__('sub', r.localize(s, pos, c, amplitude=MODE, **kw))
        med, spread = _median_times(runs, reps)
        dev = keep.get('sub', keep['res'])
        names = ('amplitude', 'weight', 'moment', 'best', 'location')
        h_amp, h_loc = keep['host']
        ok = np.isfinite(dev.location).all(axis=1)
        out = {k + '_s': round(v, 4) for k, v in med.items()}
        out.update(spread_s=spread, host_events=int(n_host), host_snippet_bytes=keep['host_wave_bytes'],
                   result_bytes=int(sum(keep['res'][k].nbytes for k in names)), nan_amplitudes=int(np.isnan(dev.amplitude).sum()),
                   cold_equals_resident=bool(all(keep['cold'][k].tobytes() == keep['res'][k].tobytes() for k in names)),
                   host_amplitudes_equal=bool(np.array_equal(h_amp, dev.amplitude, equal_nan=True)),
                   host_location_max_abs_diff=float(np.abs(h_loc[ok] - dev.location[ok]).max()) if ok.any() else 0.0,
                   location_max_abs=float(np.abs(dev.location[ok]).max()) if ok.any() else 0.0)
        assert out['cold_equals_resident'] and out['host_amplitudes_equal'], out
        assert out['host_location_max_abs_diff'] <= 1e-4 * out['location_max_abs'], out
        res['width_%s' % width] = out
        _note(width, out)
    cold_r.close()
    return res


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
    taps = api.highpass_taps(300, RATE, 101)
    cols = np.arange(NC)
    cap = n * RATE * NC // 256
    table = (cbuf, slots, sizes, bounds[:-1], np.diff(bounds), NC, np.int16, flags, 0, n * RATE)
    st, n_ev, ev, det_out = hip.dev_detect(*table, 0, n * RATE, taps, cols, thr, 0, 1, EXCLUDE, SPREAD, cap)
    assert st == [0] * n and n_ev <= cap
    det_out.free()
    _note('device: %d events' % n_ev)
    res = {'events': int(n_ev), 'workload': '%d s x 385 int16 in HBM, 101 taps, median reference; %d runs after %d warm-ups, median' % (n, reps, warmup)}
    pos = probe_positions(NC)
    mode = hip.LOCALIZE_MODES[MODE]
    for width, W, col0 in (('17', 2 * K + 1, ev[1].astype(np.int64) - K), ('full', NC, np.zeros(n_ev, np.int64))):
        state = {'loc': None, 'wav': None}

        def loc(want_amp):
            st, _, state['loc'] = hip.dev_localize(*table, taps, cols, 1, ev[0], col0, BEFORE, AFTER, W, mode, pos, want_amp, out=state['loc'],
                                                   download=False)
            assert st == [0] * n

        def wav():
            st, _, state['wav'] = hip.dev_waveforms(*table, taps, cols, 1, ev[0], col0, BEFORE, AFTER, W, False, out=state['wav'], download=False)
            assert st == [0] * n
        runs = {'dev_localize': lambda: loc(True), 'dev_localize_no_amplitudes': lambda: loc(False), 'dev_waveforms_extrema_only': wav}
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
        out = {k + '_ms': round(float(np.median(v)), 3) for k, v in times.items()}
        os.environ['MTS_WAVEFORMS_TIME'] = '1'
        try:
            gather = {}
            for name, f in runs.items():
                us = []
                for _ in range(reps + 1):
                    f()
                    us.append(hip.waveforms_last_plan(0)['gather_us'])
                gather[name + '_kernel_ms'] = round(float(np.median(us[1:])) / 1e3, 3)
            gather['slabs'] = hip.waveforms_last_plan(0)['slabs']
            out['gather'] = gather
        finally:
            os.environ.pop('MTS_WAVEFORMS_TIME', None)
        out['result_bytes'] = 4 * n_ev * (W + pos.shape[1] + 2)
        out['snippet_bytes'] = 4 * n_ev * T * W
        for b in state.values():
            if b is not None:
                b.free()
        res['width_%s' % width] = out
        _note('device', width, out)
    cbuf.free()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--sigma', type=float, default=3.5)
    ap.add_argument('--host-full-events', type=int, default=8000, help='events of the host path at full width (it holds their snippets in memory)')
    ap.add_argument('--device-only', action='store_true', help='the device entries alone')
    ap.add_argument('--reader-only', action='store_true', help='the Reader alone')
    ap.add_argument('--out', default=None, help='also write the line here (profiles/localize.json)')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'localize_bench', 'measured': True, 'sigma': a.sigma, 'seconds': a.seconds, 'reps': a.reps,
            'positions': 'two-column staggered grid: x = 11 / 43, y = 20 * (channel // 2)'}
    tmp = Path(tempfile.mkdtemp(prefix='mtsloc_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
    try:
        bench.build_synth_file(hip, 0, a.seconds, tmp, NC)
        r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
        thr = (spike_threshold(r, api.highpass_taps(300, RATE, 101)) * (a.sigma / 5.0)).astype(np.float32)
        if not a.device_only:
            line['reader'] = reader_part(tmp, r, thr, a.reps, a.host_full_events)
        r.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if not a.reader_only:
        hip.release()
        line['device'] = device_part(a.reps, a.warmup, a.seconds, thr)
    print(json.dumps(line))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
