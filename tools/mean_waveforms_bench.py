"""Per-unit mean snippets on the device against what a user does today; prints one JSON line and writes it to --out.

  reader  the 60 s x 385 int16 recording of the synthetic generator as a .cbin on tmpfs.  The events are those of
          detect(3.5 * mad / 0.6745, taps=highpass_taps(300, 30000, 101), reference='median', exclude=30, spread=5) (the thresholds of
          tools/waveforms_bench.py at its dense setting), the labels channel % 8 and channel % 128, the snippets 20 before and 41 after,
          17 wide (neighbours=8) and full width.  In one process, the runs alternated, medians of --reps runs:
            mean_waveforms cold and resident, and the path users have today: waveforms(...) resident, then the same fixed-point sums
            on the host (the snippets sorted by label, rint, one integer sum per label).  The sums of the two paths are compared for
            equality.  At full width the host path holds every snippet in memory (8.6 GB for 92 000 events), so it runs on the first
            --host-full-events events and the device path is timed on those and on all.
  device  mts_dev_mean_waveforms against mts_dev_waveforms (with snippets and extrema only) on the recording's chunks in HBM: they
          share the filter and the median, so the difference is the gather; and the gather kernels' own time (MTS_WAVEFORMS_TIME:
          events around each launch) for MTS_MEAN_PART_EVENTS of 16, 64 and 256."""
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
from tools.waveforms_bench import AFTER, BEFORE, EXCLUDE, K, NC, RATE, SPREAD, _median_times, spike_threshold  # noqa: E402

RESOLUTION = 2.0 ** -16
PARTS = (16, 64, 256)
# the part size kept after the sweep of profiles/mean_waveforms.json, and why (written into every line)
MEAN_PART_KEPT = ('64 (MEAN_PART_EVENTS, reduce.hip): swept at 16 / 64 / 256 under MTS_WAVEFORMS_TIME.  At full width (61 x 385, the case the op exists for) 64 is the best or within 0.1 ms of it (2.2 / 2.5 ms against 5.6 / 5.3 at 16 and 3.2 / 2.5 at 256, labels 8 / 128); at width 17 smaller parts win (0.56 / 0.46 ms at 16 against 1.02 / 0.91 at 64) but the whole gather is 1 ms of a 36 ms call there.  64-bit integer atomics were not measured on their own.')
T = BEFORE + AFTER


def _note(*what):
    print('mean_waveforms_bench:', *what, file=sys.stderr, flush=True)


def host_sums(wave, label, n_labels):
    """The fixed-point sums and counts of the definition from waveforms' snippets, on the host."""
    order = np.argsort(label, kind='stable')
    first = np.searchsorted(label[order], np.arange(n_labels + 1))
    total = np.zeros((n_labels,) + wave.shape[1:], np.int64)
    count = np.zeros((n_labels,) + wave.shape[1:], np.int64)
    for k in range(n_labels):
        w = wave[order[first[k]:first[k + 1]]]
        some = ~np.isnan(w)
        total[k] = np.where(some, np.rint(w.astype(np.float64) / RESOLUTION), 0).astype(np.int64).sum(axis=0)
        count[k] = some.sum(axis=0)
    return total, count


def reader_part(tmp, r, thr, reps, host_full_events):
    cold_r = mtscomp_amd.decompress(tmp / 'data.cbin', tmp / 'data.ch', check_after_decompress=False)
    cold_r._dev_cache_bytes = 0                                           # never resident: every call decodes
    taps = api.highpass_taps(300, RATE, 101)
    for k in range(r.n_chunks):                                          # every chunk into the device cache
        r[r.chunk_bounds[k]:r.chunk_bounds[k] + 1]
    ev = r.detect(thr, taps=taps, reference='median', exclude=EXCLUDE, spread=SPREAD)
    _note('%d events' % ev.sample.size)
    res = {'events': int(ev.sample.size), 'resolution': RESOLUTION}
    for width, neighbours, n_host in (('17', K, ev.sample.size), ('full', None, min(host_full_events, ev.sample.size))):
        kw = dict(before=BEFORE, after=AFTER, neighbours=neighbours, taps=taps, reference='median')
        for n_labels in (8, 128):
            label = ev.channel % n_labels
            keep = {}
            s, c, lab = ev.sample[:n_host], ev.channel[:n_host], label[:n_host]

            def host():
                w = r.waveforms(s, c, **kw).waveforms
                keep['host_wave_bytes'] = int(w.nbytes)
                keep['host'] = host_sums(w, lab, n_labels)
            runs = {'mean_waveforms_cold': lambda: keep.__setitem__('cold', cold_r.mean_waveforms(ev.sample, label, ev.channel, n_labels=n_labels, **kw)),
                    'mean_waveforms_resident': lambda: keep.__setitem__('res', r.mean_waveforms(ev.sample, label, ev.channel, n_labels=n_labels, **kw)),
                    'waveforms_resident_plus_host_sum': host}
            if n_host < ev.sample.size:
                runs['mean_waveforms_resident_host_events'] = lambda: keep.__setitem__('sub', r.mean_waveforms(s, lab, c, n_labels=n_labels, **kw))
            med, spread = _median_times(runs, reps)
            dev = keep.get('sub', keep['res'])
            out = {k + '_s': round(v, 4) for k, v in med.items()}
            out.update(spread_s=spread, host_events=int(n_host), host_snippet_bytes=keep['host_wave_bytes'],
                       result_bytes=int(keep['res'].sum.nbytes + keep['res'].count.nbytes // 2 + keep['res'].skipped.nbytes),
                       skipped=int(keep['res'].skipped.sum()),
                       cold_equals_resident=bool(keep['cold'].sum.tobytes() == keep['res'].sum.tobytes() and keep['cold'].count.tobytes() == keep['res'].count.tobytes()),
                       host_sums_equal_device=bool(dev.sum.tobytes() == keep['host'][0].tobytes() and dev.count.tobytes() == keep['host'][1].tobytes()))
            assert out['cold_equals_resident'] and out['host_sums_equal_device'], out
            res['width_%s_labels_%d' % (width, n_labels)] = out
            _note(width, n_labels, out)
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
    for width, W, col0 in (('17', 2 * K + 1, ev[1].astype(np.int64) - K), ('full', NC, np.zeros(n_ev, np.int64))):
        for n_labels in (8, 128):
            label = ev[1].astype(np.int64) % n_labels
            state = {'mean': None, 'wav': None}

            def mean():
                st, _, state['mean'] = hip.dev_mean_waveforms(*table, taps, cols, 1, ev[0], col0, label, n_labels, BEFORE, AFTER, W, RESOLUTION,
                                                              out=state['mean'], download=False)
                assert st == [0] * n

            def wav(want_wave):
                st, _, state['wav'] = hip.dev_waveforms(*table, taps, cols, 1, ev[0], col0, BEFORE, AFTER, W, want_wave, out=state['wav'], download=False)
                assert st == [0] * n
            runs = {'dev_mean_waveforms': mean, 'dev_waveforms_extrema_only': lambda: wav(False)}
            if 4 * n_ev * T * W <= 12 << 30:                                 # (the snippets of every event in HBM)
                runs['dev_waveforms'] = lambda: wav(True)
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
                for part in PARTS:
                    os.environ['MTS_MEAN_PART_EVENTS'] = str(part)
                    us = []
                    for _ in range(reps + 1):
                        mean()
                        us.append(hip.waveforms_last_plan(0)['gather_us'])
                    gather[str(part)] = {'kernel_ms': round(float(np.median(us[1:])) / 1e3, 3), 'slabs': hip.waveforms_last_plan(0)['slabs']}
                wav(False)
                gather['waveforms_extrema_only_kernel_ms'] = round(hip.waveforms_last_plan(0)['gather_us'] / 1e3, 3)
                out['gather_by_part_events'] = gather
            finally:
                os.environ.pop('MTS_WAVEFORMS_TIME', None)
                os.environ.pop('MTS_MEAN_PART_EVENTS', None)
            for b in state.values():
                if b is not None:
                    b.free()
            res['width_%s_labels_%d' % (width, n_labels)] = out
            _note('device', width, n_labels, out)
    cbuf.free()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--sigma', type=float, default=3.5)
    ap.add_argument('--host-full-events', type=int, default=8000, help='events of the host path at full width (it holds their snippets in memory)')
    ap.add_argument('--device-only', action='store_true', help='the device entries alone')
    ap.add_argument('--reader-only', action='store_true', help='the Reader alone')
    ap.add_argument('--out', default=None, help='also write the line here (profiles/mean_waveforms.json)')
    a = ap.parse_args(argv)
    hip.require_device()
    line = {'tool': 'mean_waveforms_bench', 'measured': True, 'sigma': a.sigma, 'seconds': a.seconds, 'reps': a.reps, 'mean_part_kept': MEAN_PART_KEPT}
    tmp = Path(tempfile.mkdtemp(prefix='mtsmean_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None))
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
